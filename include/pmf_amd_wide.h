/* libpmf_amd.so -- 33 to 64 classes in the heads and in the fused objective (csrc/elementwise.hip, csrc/loss.hip).  Third
 * header of the C ABI: pmf_amd.h keeps its prototypes and their 32-class contract (every entry point there still refuses
 * C > 32 with the code it always had); this one adds the entry points that go up to pmf_wide_max_classes() = 64.  Same
 * conventions as pmf_amd.h (caller-owned DEVICE pointers, every call enqueues on the given stream and returns without
 * synchronising, 0 / hipError_t / negative PMF_E_*), read by the same strict reader (pmf_amd/_lib.py).
 *
 * Every function below
 *   - checks its arguments before the first HIP call;
 *   - routes C <= 32 to the very kernels the pmf_amd.h entry point launches (same grid, same bits);
 *   - refuses C > 64 with the code of its pmf_amd.h counterpart (softmax pair: PMF_E_UNSUPPORTED, loss: PMF_E_ARG);
 *   - keeps every other guard of that counterpart.
 * Above 32 classes the kernels are their own instantiations (template parameter MAXC = 64), none of which needs scratch
 * memory: the softmax pair keeps the pixel's 64-float row(s) in registers under a launch bound of 256 threads (the 32-class
 * kernels compile under the default bound, where 64 floats spill), and the per-pixel loss kernel keeps no class-sized array
 * at all -- it reads p_c, q_c again in its second class loop.  The float32 operations and their order are those of the
 * 32-class kernels.
 * Callers (plan.cpp, pmf_amd/loss/fused.py) take these entry points only when C > 32. */
#ifndef PMF_AMD_WIDE_H
#define PMF_AMD_WIDE_H
#include "pmf_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* the class limit of this header: 64 */
int pmf_wide_max_classes(void);

/* pmf_softmax_nhwc_to_nchw (ident = 0) / pmf_logits_nhwc_to_nchw (ident != 0) for 1 <= C <= 64; otherwise
 * PMF_E_UNSUPPORTED.  One thread per pixel, no grid cap: more than 2^31 - 1 blocks of 256 pixels is PMF_E_UNSUPPORTED. */
int pmf_softmax_wide(const float* logits, int32_t ldc, int32_t N, int32_t HW, int32_t C, int32_t ident, float* out_nchw,
                     pmf_stream_t s);
/* pmf_softmax_bwd_nchw_to_nhwc (ident = 0) / pmf_logits_bwd_nchw_to_nhwc (ident != 0; prob_nchw is not read and may be
 * null) for C <= 64 and ldc <= 64; otherwise PMF_E_UNSUPPORTED.  Channels C .. ldc - 1 of dlogits are written as 0. */
int pmf_softmax_wide_bwd(const float* prob_nchw, const float* g_nchw, int32_t N, int32_t HW, int32_t C, int32_t ident,
                         float* dlogits, int32_t ldc, pmf_stream_t s);

/* Step 1 of the fused objective for 2 <= C <= 64: the argument list of pmf_loss_pixel_dice plus w6.
 *   w6 null, parts and dice null   pmf_loss_pixel      (lambda / gamma_per form)
 *   w6 given, parts and dice null  pmf_loss_pixel_w    (gamma_per is ignored)
 *   w6 null, parts and dice given  pmf_loss_pixel_dice
 * PMF_E_ARG: C outside [2, 64]; w6 together with dice; ONE of parts / dice null without the other; every guard of
 * pmf_loss_pixel (null pointers, a lone confusion matrix, N < 1, HW < 1).  The block-count limit is PMF_E_UNSUPPORTED. */
int pmf_loss_pixel_wide(const float* lidar_prob, const float* camera_prob, const int64_t* label, const float* alpha,
                        int32_t N, int32_t C, int64_t HW, float focal_gamma, float tau, float gamma_per,
                        unsigned long long* cnt, float* grad_lidar, float* grad_camera, float* key, double* rows,
                        unsigned long long* conf_lidar, unsigned long long* conf_camera, double* parts, double* dice,
                        const float* w6, pmf_stream_t s);

/* Step 2 for 2 <= C <= 64: pmf_loss_lovasz_sort (w6 null) or pmf_loss_lovasz_sort_w (w6 given; lambda and gamma_per are
 * ignored).  The stage has no class capacity of its own -- the radix sort, the Jaccard kernels and the fold are generic in
 * C -- so above 32 classes the same kernels run on 2C rows.  PMF_E_ARG: C outside [2, 64], N < 1, HW < 1, workspace null;
 * PMF_E_UNSUPPORTED: N * HW > 2^24.  pmf_loss_rows, _chunks, _dice_parts and _sort_workspace have no class limit. */
int pmf_loss_lovasz_sort_wide(const float* key, const int64_t* label, int32_t N, int32_t C, int64_t HW,
                              const unsigned long long* cnt, float lambda, float gamma_per, void* workspace, float* bsum,
                              double* dots, const double* rows, float* grad_lidar, float* grad_camera, float* out8,
                              const float* w6, pmf_stream_t s);

/* pmf_loss_dice_finish for 2 <= C <= 64 */
int pmf_loss_dice_finish_wide(const double* dice, int32_t C, float* out10, pmf_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
