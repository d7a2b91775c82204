/* libpmf_amd.so -- the SemanticKITTI-FOV filter (csrc/project.hip).  Sixth header of the C ABI: pmf_amd.h,
 * pmf_amd_sensat.h, pmf_amd_wide.h, pmf_amd_a2d2.h and pmf_amd_nus.h keep their prototypes, this one adds the one entry point
 * behind the reference's tasks/process_semantickitti_fov/create_fov_dataset.py: the points of every sweep that the left
 * colour camera sees, for a BATCH of frames in one pass.  Its kernels live beside project_point in csrc/project.hip and call
 * it, so the keep rule has one definition: the written tree is exactly the set of points PerspectiveViewLoader keeps.
 * Same conventions as pmf_amd.h (the call enqueues on the given stream and returns without synchronising, 0 / hipError_t /
 * negative PMF_E_*), read by the same strict reader (pmf_amd/_lib.py).  All pointers are DEVICE memory. */
#ifndef PMF_AMD_FOV_H
#define PMF_AMD_FOV_H
#include "pmf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* points per workgroup (one lane per point): blk_cnt holds one count per workgroup */
#define PMF_FOV_BLOCK 1024
/* frames per call */
#define PMF_FOV_MAX_FRAMES 64

/* B frames of one sequence, three launches (count, scan, compact), no memset, no copy, no synchronisation.
 *   in:  points f32[P_total][4]: the B sweeps one behind the other, 16-byte aligned (rows are read as one 16-byte load)
 *        labels u32[P_total]: the raw .label words, or NULL (test sequences): then out_labels is not touched and may be NULL
 *        offsets i64[B + 1]: frame b owns the rows [offsets[b], offsets[b + 1]).  The kernels ASSUME offsets[0] = 0,
 *            offsets[B] = P_total and offsets[b] <= offsets[b + 1] (an empty frame is legal); the caller checks that on the
 *            host before the upload.  Whatever the table holds, nothing is read or written out of bounds: with a table
 *            that breaks the assumption a row is judged by some frame's dims and entries of out_offsets stay unwritten.
 *        dims i32[B][2]: (h, w) of frame b's image
 *        proj f64[12]: the 3 x 4 projection matrix, row-major; one per call, a batch never spans sequences
 *        blk_cnt i32[ceil(P_total / PMF_FOV_BLOCK) + 1]: the only workspace
 *   keep rule: keep[i] = project_point(points + 4 * i, proj, h_b, w_b) of csrc/project.hip for the frame b that owns row i,
 *        bit for bit the mask pmf_project_scatter / pmf_project_scatter2 produce for that frame alone: x > 0.5f, the
 *        k-ordered float64 FMA chain, 0 < u < w, 0 < v < h; a NaN anywhere means "not kept".
 *   out: keep u8[P_total]; out_points f32[K][4] and out_labels u32[K]: the kept rows and their label words in file order,
 *        compacted over the whole batch and copied as bits (the label word of a kept point is its input word, high bit
 *        included); out_offsets i64[B + 1]: frame b's kept rows are [out_offsets[b], out_offsets[b + 1]), out_offsets[B] = K.
 *        The output arrays have capacity P_total and must not overlap the inputs; nothing at or beyond row K is written.
 * PMF_E_ARG without a launch: a null pointer other than labels / out_labels, labels without out_labels, B outside
 * 1..PMF_FOV_MAX_FRAMES, P_total < 1, points or out_points not 16-byte aligned.  PMF_E_UNSUPPORTED without a launch:
 * P_total >= 2^31. */
int pmf_fov_filter(const float* points, const uint32_t* labels, const int64_t* offsets, const int32_t* dims, int32_t B,
                   int64_t P_total, const double* proj, uint8_t* keep, float* out_points, uint32_t* out_labels,
                   int64_t* out_offsets, int32_t* blk_cnt, pmf_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
