// KNN post-processing vote (pc_processor/postproc/knn.py:55-143) as one lane per point on gfx950.
// The reference materialises two [1, S*S, H*W] unfolds and four [1, S*S, P] gathers; here each lane keeps its
// S*S window (weighted |range difference| and neighbour labels) in registers, selects the k smallest by
// repeated first-minimum (ties -> smaller window index, the rule the CPU oracle pins) and votes.
// HBM-bound: algorithmic bytes 12*H*W + 28*P per call.
// The vote itself (window, selection, majority) is the set of device functions of knn_vote.h; the kernels here resolve the
// frame and the point and store int64 labels.
#include "common.h"
#pragma clang fp contract(off)
#include "knn_vote.h"

template <int S>
__global__ __launch_bounds__(256) void knn_k(const float* __restrict__ pr, const float* __restrict__ ur,
                                             const int64_t* __restrict__ am, const int64_t* __restrict__ px,
                                             const int64_t* __restrict__ py, int H, int W, int64_t P, int knn,
                                             const float* __restrict__ invg, float cutoff, int nclasses,
                                             int64_t* __restrict__ labels, const int32_t* __restrict__ am32 = nullptr) {
  constexpr int S2 = S * S;
  __shared__ float wsh[S2];
  if (threadIdx.x < S2) wsh[threadIdx.x] = invg[threadIdx.x];
  __syncthreads();
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= P) return;
  labels[i] = knn_vote_gather<S>(pr, am, am32, (int)px[i], (int)py[i], ur[i], H, W, knn, wsh, cutoff, nclasses);
}

// ---- any odd window (search = 1, 9, 11, ...; the reference accepts every odd size, knn.py:73-74; the nuScenes config ships
// search 11, tasks/pmf_eval_nuscenes/config_server_nus.yaml) -------------------------------------------------------------
// One lane per point, window size at run time (knn_vote_any): bit-identical labels to knn_k where both apply (tests).
// Frames of a batch through the offsets table (nullptr: one frame).
__global__ __launch_bounds__(64) void knn_any_k(const float* __restrict__ pr, const float* __restrict__ ur,
                                                const int64_t* __restrict__ am, const int64_t* __restrict__ px,
                                                const int64_t* __restrict__ py, const int64_t* __restrict__ offsets, int B,
                                                int H, int W, int64_t P, int knn, int S, const float* __restrict__ invg,
                                                float cutoff, int nclasses, int64_t* __restrict__ labels,
                                                const int32_t* __restrict__ am32 = nullptr) {
  const int64_t i = blockIdx.x * (int64_t)64 + threadIdx.x;
  if (i >= P) return;
  int b = 0;
  if (offsets) for (int k = 1; k < B; ++k) b += offsets[k] <= i;
  const float* __restrict__ prb = pr + (size_t)b * H * W;
  const int64_t* __restrict__ amb = am + (size_t)b * H * W;
  const int32_t* __restrict__ amb32 = am32 ? am32 + (size_t)b * H * W : nullptr;
  labels[i] = knn_vote_any(prb, amb, amb32, (int)px[i], (int)py[i], ur[i], H, W, knn, S, invg, cutoff, nclasses);
}

template <int S>
__global__ void knn_batch_lds_k(const float* __restrict__ pr, const float* __restrict__ ur, const int64_t* __restrict__ am,
                                const int64_t* __restrict__ px, const int64_t* __restrict__ py,
                                const int64_t* __restrict__ offsets, int B, int H, int W, int64_t P1, int knn,
                                const float* __restrict__ invg, float cutoff, int nclasses, int64_t* __restrict__ labels,
                                const int32_t* __restrict__ am32 = nullptr);

extern "C" int pmf_knn_vote(const float* proj_range, const float* unproj_range, const int64_t* proj_argmax,
                            const int64_t* px, const int64_t* py, int32_t H, int32_t W, int64_t P, int32_t knn,
                            int32_t search, const float* inv_gauss, float cutoff, int32_t nclasses, int64_t* labels,
                            pmf_stream_t s) {
  if (search % 2 == 0) return PMF_E_ARG;  // knn.py:73-74 raises ValueError
  if (knn < 1 || knn > 8 || knn > search * search) return PMF_E_UNSUPPORTED;
  if (P <= 0) return 0;
  dim3 grid((unsigned)cdiv64(P, 256)), block(256);
  hipStream_t st = (hipStream_t)s;
  constexpr bool no_lds = false;
  if (search < 1 || search > 255) return PMF_E_ARG;
  if (!no_lds && (search == 3 || search == 5)) {        // the LDS-staged form (below), one frame, no offsets table
    if (search == 3) hipLaunchKernelGGL(knn_batch_lds_k<3>, grid, block, 0, st, proj_range, unproj_range, proj_argmax, px, py, (const int64_t*)nullptr, 1, H, W, P, knn, inv_gauss, cutoff, nclasses, labels);
    else hipLaunchKernelGGL(knn_batch_lds_k<5>, grid, block, 0, st, proj_range, unproj_range, proj_argmax, px, py, (const int64_t*)nullptr, 1, H, W, P, knn, inv_gauss, cutoff, nclasses, labels);
    PMF_LAUNCH_CHECK();
    return 0;
  }
  switch (search) {
    case 3: hipLaunchKernelGGL(knn_k<3>, grid, block, 0, st, proj_range, unproj_range, proj_argmax, px, py, H, W, P, knn, inv_gauss, cutoff, nclasses, labels); break;
    case 5: hipLaunchKernelGGL(knn_k<5>, grid, block, 0, st, proj_range, unproj_range, proj_argmax, px, py, H, W, P, knn, inv_gauss, cutoff, nclasses, labels); break;
    case 7: hipLaunchKernelGGL(knn_k<7>, grid, block, 0, st, proj_range, unproj_range, proj_argmax, px, py, H, W, P, knn, inv_gauss, cutoff, nclasses, labels); break;
    default:     // every other odd window (1, 9, 11, ...): run-time window size
      hipLaunchKernelGGL(knn_any_k, dim3((unsigned)cdiv64(P, 64)), dim3(64), 0, st, proj_range, unproj_range, proj_argmax, px, py, (const int64_t*)nullptr, 1, H, W, P, knn, search, inv_gauss, cutoff, nclasses, labels);
  }
  PMF_LAUNCH_CHECK();
  return 0;
}

// ---- all frames of a batch in ONE launch (BASELINE configs[1]: bs = 4) ------------------------------------------------
// Range images / argmax maps are [B, H, W]; the points of all frames are concatenated, frame b owning
// [offsets[b], offsets[b+1]).  64-thread workgroups (one wave): a 25 k-point frame is 391 workgroups instead of 98, so four
// frames fill the 256 CUs ~6x over and the ~50 dependent-address loads per lane of one wave overlap with its
// neighbours' on the CU.  Same arithmetic as knn_k (bit-identical labels).
template <int S>
__global__ __launch_bounds__(64) void knn_batch_k(const float* __restrict__ pr, const float* __restrict__ ur,
                                                  const int64_t* __restrict__ am, const int64_t* __restrict__ px,
                                                  const int64_t* __restrict__ py, const int64_t* __restrict__ offsets,
                                                  int B, int H, int W, int64_t P, int knn, const float* __restrict__ invg,
                                                  float cutoff, int nclasses, int64_t* __restrict__ labels,
                                                  const int32_t* __restrict__ am32 = nullptr) {
  constexpr int S2 = S * S;
  __shared__ float wsh[S2];
  if (threadIdx.x < S2) wsh[threadIdx.x] = invg[threadIdx.x];
  __syncthreads();
  const int64_t i = blockIdx.x * (int64_t)64 + threadIdx.x;
  if (i >= P) return;
  int b = 0;
  for (int k = 1; k < B; ++k) b += offsets[k] <= i;     // B is small (a batch): wave-uniform scalar loads
  const float* __restrict__ prb = pr + (size_t)b * H * W;
  const int64_t* __restrict__ amb = am + (size_t)b * H * W;
  const int32_t* __restrict__ amb32 = am32 ? am32 + (size_t)b * H * W : nullptr;
  labels[i] = knn_vote_gather<S>(prb, amb, amb32, (int)px[i], (int)py[i], ur[i], H, W, knn, wsh, cutoff, nclasses);
}

// ---- the same vote with the window staged through LDS (knn_vote_lds) ---------------------------------------------------
// A workgroup is 256 consecutive points of ONE frame: frame b owns ceil(n_b / 256) consecutive workgroups (knn_wg_frame).
// (Measured: indexing the concatenated list directly, so that the point loads do not wait for the frame walk, is SLOWER
// -- 13.2 vs 11.7 us -- the per-thread frame search and the mixed-frame handling cost more than the overlap gives.)
template <int S>
__global__ __launch_bounds__(256) void knn_batch_lds_k(const float* __restrict__ pr, const float* __restrict__ ur,
                                                       const int64_t* __restrict__ am, const int64_t* __restrict__ px,
                                                       const int64_t* __restrict__ py, const int64_t* __restrict__ offsets,
                                                       int B, int H, int W, int64_t P1, int knn, const float* __restrict__ invg,
                                                       float cutoff, int nclasses, int64_t* __restrict__ labels,
                                                       const int32_t* __restrict__ am32) {
  int b, wg;
  int64_t lo, hi;
  knn_wg_frame(offsets, B, P1, b, wg, lo, hi);
  if (b < 0) return;                                    // (the grid is an upper bound)
  const int64_t i = lo + (int64_t)wg * 256 + threadIdx.x;
  const bool valid = i < hi;
  const float* __restrict__ prb = pr + (size_t)b * H * W;
  const int64_t* __restrict__ amb = am + (size_t)b * H * W;
  const int32_t* __restrict__ amb32 = am32 ? am32 + (size_t)b * H * W : nullptr;
  int cx = 0, cy = 0;
  float r = 0.f;
  if (valid) { cx = (int)px[i]; cy = (int)py[i]; r = ur[i]; }
  const int lab = knn_vote_lds<S>(prb, amb, amb32, valid, cx, cy, r, H, W, knn, invg, cutoff, nclasses);
  if (valid) labels[i] = lab;
}

int knn_vote_batch_impl(const float* proj_range, const float* unproj_range, const int64_t* proj_argmax,
                               const int32_t* am32, const int64_t* px, const int64_t* py, const int64_t* offsets, int32_t B,
                               int32_t H, int32_t W, int64_t P_total, int32_t knn, int32_t search, const float* inv_gauss,
                               float cutoff, int32_t nclasses, int64_t* labels, pmf_stream_t s) {
  if (search % 2 == 0) return PMF_E_ARG;
  if (B < 1 || B > 1024 || !offsets) return PMF_E_ARG;
  if (knn < 1 || knn > 8 || knn > search * search) return PMF_E_UNSUPPORTED;
  if (P_total <= 0) return 0;
  hipStream_t st = (hipStream_t)s;
  constexpr bool no_lds = false;
  if (search < 1 || search > 255) return PMF_E_ARG;
  if (!no_lds && (search == 3 || search == 5)) {       // (7x7: 49 + 49 window registers next to 32 KB of LDS -- stays on the gather form)
    const dim3 g2((unsigned)(cdiv64(P_total, 256) + B)), b2(256);      // sum_b ceil(n_b / 256) <= ceil(P / 256) + B
    if (search == 3) hipLaunchKernelGGL(knn_batch_lds_k<3>, g2, b2, 0, st, proj_range, unproj_range, proj_argmax, px, py, offsets, B, H, W, (int64_t)0, knn, inv_gauss, cutoff, nclasses, labels, am32);
    else hipLaunchKernelGGL(knn_batch_lds_k<5>, g2, b2, 0, st, proj_range, unproj_range, proj_argmax, px, py, offsets, B, H, W, (int64_t)0, knn, inv_gauss, cutoff, nclasses, labels, am32);
    PMF_LAUNCH_CHECK();
    return 0;
  }
  dim3 grid((unsigned)cdiv64(P_total, 64)), block(64);
  switch (search) {
    case 3: hipLaunchKernelGGL(knn_batch_k<3>, grid, block, 0, st, proj_range, unproj_range, proj_argmax, px, py, offsets, B, H, W, P_total, knn, inv_gauss, cutoff, nclasses, labels, am32); break;
    case 5: hipLaunchKernelGGL(knn_batch_k<5>, grid, block, 0, st, proj_range, unproj_range, proj_argmax, px, py, offsets, B, H, W, P_total, knn, inv_gauss, cutoff, nclasses, labels, am32); break;
    case 7: hipLaunchKernelGGL(knn_batch_k<7>, grid, block, 0, st, proj_range, unproj_range, proj_argmax, px, py, offsets, B, H, W, P_total, knn, inv_gauss, cutoff, nclasses, labels, am32); break;
    default:
      hipLaunchKernelGGL(knn_any_k, grid, block, 0, st, proj_range, unproj_range, proj_argmax, px, py, offsets, B, H, W, P_total, knn, search, inv_gauss, cutoff, nclasses, labels, am32);
  }
  PMF_LAUNCH_CHECK();
  return 0;
}

extern "C" int pmf_knn_vote_batch(const float* proj_range, const float* unproj_range, const int64_t* proj_argmax,
                                  const int64_t* px, const int64_t* py, const int64_t* offsets, int32_t B, int32_t H,
                                  int32_t W, int64_t P_total, int32_t knn, int32_t search, const float* inv_gauss,
                                  float cutoff, int32_t nclasses, int64_t* labels, pmf_stream_t s) {
  if (!proj_argmax) return PMF_E_ARG;
  return knn_vote_batch_impl(proj_range, unproj_range, proj_argmax, nullptr, px, py, offsets, B, H, W, P_total, knn, search,
                             inv_gauss, cutoff, nclasses, labels, s);
}

// ---- the vote straight from the network's probability maps (tasks/pmf_eval_semantickitti/infer.py:96-112: the reference takes
// torch's argmax over the class axis -- an int64 [B, H, W] map -- and hands it to KNN) -------------------------------------------
// Launch 1: channel argmax of the NCHW probabilities into an int32 label map (four pixels per lane, class planes read as
// 16-byte vectors: 4 C H W bytes in, 4 H W out); ties go to the lowest class and a NaN wins, as torch.argmax decides.
// Launch 2: the vote above on that map.  Fusing the argmax INTO the vote would recompute it per window: in sweep order a
// workgroup's bounding box is ~9 x 68 pixels for 256 points, i.e. 2.2 class-axis scans per image pixel on a 120 k-point sweep.
__global__ __launch_bounds__(256) void argmax_nchw_k(const float* __restrict__ prob, int C, int64_t HW, int64_t total4,
                                                     int32_t* __restrict__ out) {
  const int64_t q = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (q >= total4) return;
  const int64_t per = (HW + 3) >> 2, b = q / per, p0 = (q - b * per) * 4;
  const float* base = prob + (size_t)b * C * HW + p0;
  const bool vec = p0 + 3 < HW && (HW & 3) == 0;
  float best[4];
  int bi[4] = {0, 0, 0, 0};
  for (int c = 0; c < C; ++c) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
      const f32x4 t = *(const f32x4*)(base + (size_t)c * HW);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
      for (int k = 0; k < 4; ++k) if (p0 + k < HW) v[k] = base[(size_t)c * HW + k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool take = c == 0 || v[k] > best[k] || (v[k] != v[k] && best[k] == best[k]);
      best[k] = take ? v[k] : best[k];
      bi[k] = take ? c : bi[k];
    }
  }
  for (int k = 0; k < 4; ++k) if (p0 + k < HW) out[(size_t)b * HW + p0 + k] = bi[k];
}
extern "C" int pmf_knn_vote_batch_prob(const float* proj_range, const float* unproj_range, const float* prob_nchw,
                                       const int64_t* px, const int64_t* py, const int64_t* offsets, int32_t B, int32_t H,
                                       int32_t W, int64_t P_total, int32_t knn, int32_t search, const float* inv_gauss,
                                       float cutoff, int32_t nclasses, int32_t* argmax_ws, int64_t* labels, pmf_stream_t s) {
  if (!prob_nchw || !argmax_ws || B < 1 || H < 1 || W < 1 || nclasses < 1) return PMF_E_ARG;
  if (search % 2 == 0) return PMF_E_ARG;
  const int64_t HW = (int64_t)H * W, total4 = (int64_t)B * ((HW + 3) >> 2);
  hipLaunchKernelGGL(argmax_nchw_k, dim3((unsigned)cdiv64(total4, 256)), dim3(256), 0, (hipStream_t)s, prob_nchw, nclasses, HW,
                     total4, argmax_ws);
  PMF_LAUNCH_CHECK();
  return knn_vote_batch_impl(proj_range, unproj_range, nullptr, argmax_ws, px, py, offsets, B, H, W, P_total, knn, search,
                             inv_gauss, cutoff, nclasses, labels, s);
}

// ---- multi-camera merge (tasks/pmf_eval_nuscenes/infer.py:18-38 getMergePred) --------------------------------------
// Per LiDAR point the prediction of the camera with the highest confidence; a camera that does not see the point
// counts as confidence 0 / label -1, torch.argmax breaks ties towards the FIRST camera.  One 64-bit atomicMax per
// (camera, visible point) on key = confidence bits << 32 | (n_cams-1-camera) << 16 | (label+1): confidences are
// probabilities (>= 0), so the float bit pattern orders like the value; every key starts as "camera 0, absent".
// The reference fills a [6, P] table and then walks the P points in a Python loop.
__global__ __launch_bounds__(256) void merge_scatter_k(const int64_t* __restrict__ point_idx, const float* __restrict__ conf,
                                                       const int64_t* __restrict__ label, int64_t n, int cam, int n_cams,
                                                       int64_t pc_size, unsigned long long* __restrict__ keys) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i >= n) return;
  const int64_t p = point_idx[i];
  if (p < 0 || p >= pc_size) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(conf[i]) << 32) |
                                 ((unsigned long long)(n_cams - 1 - cam) << 16) | (unsigned long long)((label[i] + 1) & 0xffff);
  atomicMax(keys + p, key);
}
__global__ __launch_bounds__(256) void merge_init_k(unsigned long long* __restrict__ keys, int64_t pc_size, int n_cams) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i < pc_size) keys[i] = (unsigned long long)(n_cams - 1) << 16;
}
// fallback (optional): label of a LiDAR-only model for every point; it replaces the -1 of points no camera sees
// (more_experiment_config.md:10: "For LiDAR points that are outside the camera view, we use predictions of SalsaNext")
__global__ __launch_bounds__(256) void merge_final_k(const unsigned long long* __restrict__ keys, int64_t pc_size,
                                                     const int64_t* __restrict__ fallback, int64_t* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i >= pc_size) return;
  const int64_t lab = (int64_t)(keys[i] & 0xffffull) - 1;
  out[i] = (lab < 0 && fallback) ? fallback[i] : lab;
}

static int merge_impl(int32_t n_cams, const int64_t* const* point_idx, const float* const* conf,
                      const int64_t* const* label, const int64_t* counts, int64_t pc_size, const int64_t* fallback,
                      uint64_t* keys, int64_t* merged, pmf_stream_t s) {
  if (n_cams < 1 || n_cams > 255 || pc_size < 0 || !counts || (pc_size > 0 && (!keys || !merged))) return PMF_E_ARG;
  for (int j = 0; j < n_cams; ++j)
    if (counts[j] < 0 || (counts[j] > 0 && (!point_idx || !conf || !label || !point_idx[j] || !conf[j] || !label[j])))
      return PMF_E_ARG;
  if (pc_size == 0) return 0;
  hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(merge_init_k, dim3((unsigned)cdiv64(pc_size, 256)), dim3(256), 0, st, (unsigned long long*)keys,
                     pc_size, n_cams);
  for (int j = 0; j < n_cams; ++j)
    if (counts[j] > 0)
      hipLaunchKernelGGL(merge_scatter_k, dim3((unsigned)cdiv64(counts[j], 256)), dim3(256), 0, st, point_idx[j], conf[j],
                         label[j], counts[j], j, n_cams, pc_size, (unsigned long long*)keys);
  hipLaunchKernelGGL(merge_final_k, dim3((unsigned)cdiv64(pc_size, 256)), dim3(256), 0, st,
                     (const unsigned long long*)keys, pc_size, fallback, merged);
  PMF_LAUNCH_CHECK();
  return 0;
}
extern "C" int pmf_merge_pred(int32_t n_cams, const int64_t* const* point_idx, const float* const* conf,
                              const int64_t* const* label, const int64_t* counts, int64_t pc_size, uint64_t* keys,
                              int64_t* merged, pmf_stream_t s) {
  return merge_impl(n_cams, point_idx, conf, label, counts, pc_size, nullptr, keys, merged, s);
}
extern "C" int pmf_merge_pred_fallback(int32_t n_cams, const int64_t* const* point_idx, const float* const* conf,
                                       const int64_t* const* label, const int64_t* counts, int64_t pc_size,
                                       const int64_t* fallback, uint64_t* keys, int64_t* merged, pmf_stream_t s) {
  if (pc_size > 0 && !fallback) return PMF_E_ARG;
  return merge_impl(n_cams, point_idx, conf, label, counts, pc_size, fallback, keys, merged, s);
}
