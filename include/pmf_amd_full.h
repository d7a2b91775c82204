/* libpmf_amd.so -- full SemanticKITTI sweeps from field-of-view predictions (csrc/project.hip).  Seventh header of the C ABI:
 * pmf_amd.h, pmf_amd_sensat.h, pmf_amd_wide.h, pmf_amd_a2d2.h, pmf_amd_nus.h and pmf_amd_fov.h keep their prototypes, this one
 * adds the inverse of pmf_fov_filter: the label words a camera + LiDAR model wrote for the points the left colour camera sees
 * go back to their rows of the raw sweep, every other row takes the word of a LiDAR-only model, and what neither labels becomes
 * one fixed id (the rule of tasks/pmf_eval_nuscenes/testset_eval, MergePred, stated on annotation ids), for a BATCH of frames
 * in one pass.  Its kernels live beside project_point in csrc/project.hip and call it, so the keep rule has one definition:
 * the rows that receive a main word are exactly the rows pmf_fov_filter keeps.
 * Same conventions as pmf_amd.h (the call enqueues on the given stream and returns without synchronising, 0 / hipError_t /
 * negative PMF_E_*), read by the same strict reader (pmf_amd/_lib.py).  All pointers are DEVICE memory. */
#ifndef PMF_AMD_FULL_H
#define PMF_AMD_FULL_H
#include "pmf_amd_fov.h"
#ifdef __cplusplus
extern "C" {
#endif

/* the workspace: blk_cnt i32[PMF_FULL_WS_PER_BLOCK * ceil(P_total / PMF_FOV_BLOCK) + PMF_FULL_WS_FIXED].  Per workgroup one
 * count and the keep bits of its PMF_FOV_BLOCK rows (32 words); once the total and one entry per frame start. */
#define PMF_FULL_WS_PER_BLOCK 33
#define PMF_FULL_WS_FIXED 66

/* B frames of one sequence, three launches (count, scan, fill), no memset, no copy, no synchronisation.
 *   in:  points f32[P_total][4], offsets i64[B + 1], dims i32[B][2], B (1..PMF_FOV_MAX_FRAMES), proj f64[12]: exactly as
 *            pmf_fov_filter takes them, with the same assumptions on offsets (checked by the caller on the host).
 *        main_ids u32[K_total], main_offsets i64[B + 1]: the camera + LiDAR model's label words as read from its .label files
 *            (annotation ids), one per FOV point in file order, the frames concatenated; frame b owns
 *            [main_offsets[b], main_offsets[b + 1]).  main_ids may be NULL when K_total = 0.
 *        sub_ids u32[P_total]: the LiDAR-only model's label words, one per point.
 *        gt u32[P_total] or NULL: the raw label words of the data set (instance id in the high half).
 *        lut i32[nlut]: annotation id -> class (class_map_lut); fill_id; C: the number of classes (conf is [C][C]).
 *   rule for row i of frame b: every id is word & 0xFFFF, cls(id) = id < nlut ? lut[id] : 0.
 *        kept = project_point(row, proj, h_b, w_b); r = the kept rows of frame b in front of row i;
 *        m = main_ids[main_offsets[b] + r] if kept and r < main_offsets[b + 1] - main_offsets[b], else 0;
 *        cls(m) != 0: pred = m, source 0; else cls(sub) != 0: pred = sub, source 1; else pred = fill_id, source 2.
 *   out: out u32[P_total] = pred (high half zero); keep u8[P_total] or NULL: the mask pmf_fov_filter gives, bit for bit;
 *        kept_count i64[B]: the kept rows of every frame (the host compares it with the length of the frame's main file);
 *        counts i64[3] or NULL: += the rows by source; conf i64[C][C] or NULL (needs gt): conf[cls(pred)][cls(gt)] += 1 over
 *        ALL rows (the orientation of pmf_eval_fill; a class outside 0..C-1 on either side is not counted).
 *        Integer atomics only: two calls give the same bits.
 *   Whatever the two offset tables hold, nothing is read or written out of bounds: an index into main_ids outside
 *   [0, K_total) reads as m = 0, and with a points table that breaks the assumptions rows are judged by some frame and
 *   kept_count holds unspecified values.
 * PMF_E_ARG without a launch: a null pointer other than main_ids (with K_total = 0), gt, keep, counts, conf; conf without gt;
 * B outside 1..PMF_FOV_MAX_FRAMES, P_total < 1, K_total < 0, C outside 1..64, nlut < 1, points not 16-byte aligned.
 * PMF_E_UNSUPPORTED without a launch: P_total >= 2^31. */
int pmf_kitti_full_fill(const float* points, const int64_t* offsets, const int32_t* dims, int32_t B, int64_t P_total,
                        const double* proj, const uint32_t* main_ids, const int64_t* main_offsets, int64_t K_total,
                        const uint32_t* sub_ids, const uint32_t* gt, const int32_t* lut, int32_t nlut, uint32_t fill_id,
                        int32_t C, uint32_t* out, uint8_t* keep, int64_t* kept_count, int64_t* counts, int64_t* conf,
                        int32_t* blk_cnt, pmf_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
