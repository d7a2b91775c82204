// EPMF point-wise evaluation on SemanticKITTI (tasks/epmf_eval_semantickitti/infer.py of the reference, per frame):
// the device work around the network.  Frames have their own size (the bounding box of the yaw-cropped points), padded
// centred up to multiples of 64; the reference spends ~10 small torch launches and host copies per frame on it.
//   pmf_eval_pre     proj f32[10,h,w] -> pcd f32[5,H,W] = (x - mean) / std * mask, rgb f32[3,H,W], proj_depth f32[h,w]
//   pmf_eval_argmax  class argmax over the (top, left, h, w) window of the padded probability map (row stride W, no
//                    contiguous copy) -> optional int32[h,w] map, optional += [C][C] pixel confusion (pred, label)
//   pmf_eval_points  labels of the K kept points: a gather of the argmax straight from the probability window, or the
//                    KNN vote of knn.hip on the int32 map; += [C][C] point confusion, optional uint32 inverse-mapped ids
//   pmf_eval_range_batch  SalsaNext range images (every sweep 32x2048 on nuScenes), B sweeps per call: section (e)
//   pmf_eval_fill / pmf_eval_sweep_finish_fill  full sweeps: camera labels filled from a LiDAR-only prediction: section (f)
// Ties of the argmax go to the lowest class and a NaN wins (torch.argmax).  Confusion counts are per-workgroup LDS
// histograms flushed with 64-bit global atomics (as loss.hip's fused loss does); all stores are vector stores.
#include "common.h"
#pragma clang fp contract(off)
#include "knn_vote.h"

#define EV_MAXC 64          // classes of an LDS confusion histogram (16 KB)
#define EV_GRID 1024        // workgroup cap of the grid-stride kernels (bounds the histogram flushes)

// ---- (a) frame -> network inputs -------------------------------------------------------------------------------------
// One lane per pixel of the padded canvas; the torch sequence of the reference is ZeroPad2d, then
// (x - mean) / std * mask in float32 (IEEE division: no reciprocal-multiply, no contraction), the same arithmetic here.
__global__ __launch_bounds__(256) void eval_pre_k(const float* __restrict__ proj, int h, int w, int H, int W, int top,
                                                  int left, const float* __restrict__ mean, const float* __restrict__ stds,
                                                  float* __restrict__ pcd, float* __restrict__ rgb,
                                                  float* __restrict__ pdepth) {
  const int64_t HW = (int64_t)H * W, hw = (int64_t)h * w;
  for (int64_t p = blockIdx.x * (int64_t)256 + threadIdx.x; p < HW; p += (int64_t)gridDim.x * 256) {
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    const int r = y - top, c = x - left;
    const bool in = r >= 0 && r < h && c >= 0 && c < w;
    const int64_t q = in ? (int64_t)r * w + c : 0;
    float v[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) v[k] = in ? proj[k * hw + q] : 0.f;
    const float mk = v[8];
#pragma unroll
    for (int k = 0; k < 5; ++k) pcd[k * HW + p] = (v[k] - mean[k]) / stds[k] * mk;
#pragma unroll
    for (int k = 0; k < 3; ++k) rgb[k * HW + p] = v[5 + k];
    if (in) pdepth[q] = v[0] - (v[0] == 0.f ? 1.f : 0.f);        // -1 on empty pixels (proj_depth.eq(0))
  }
}

extern "C" int pmf_eval_pre(const float* proj, int32_t h, int32_t w, int32_t H, int32_t W, int32_t top, int32_t left,
                            const float* mean, const float* stds, float* pcd, float* rgb, float* proj_depth,
                            pmf_stream_t s) {
  if (!proj || !mean || !stds || !pcd || !rgb || !proj_depth) return PMF_E_ARG;
  if (h < 1 || w < 1 || top < 0 || left < 0 || top + h > H || left + w > W) return PMF_E_ARG;
  const int64_t HW = (int64_t)H * W;
  const int64_t g = cdiv64(HW, 256);
  hipLaunchKernelGGL(eval_pre_k, dim3((unsigned)(g < 2048 ? g : 2048)), dim3(256), 0, (hipStream_t)s, proj, h, w, H, W,
                     top, left, mean, stds, pcd, rgb, proj_depth);
  PMF_LAUNCH_CHECK();
  return 0;
}

// ---- (b) window argmax + pixel confusion -----------------------------------------------------------------------------
__device__ __forceinline__ void ev_take(float v, int c, float& best, int& bi) {
  const bool take = c == 0 || v > best || (v != v && best == best);     // torch.argmax: first maximum, NaN wins
  best = take ? v : best;
  bi = take ? c : bi;
}

__device__ __forceinline__ void ev_hist_zero(unsigned* hist, int C) {
  for (int k = threadIdx.x; k < C * C; k += blockDim.x) hist[k] = 0u;
  __syncthreads();
}

__device__ __forceinline__ void ev_hist_flush(const unsigned* hist, int C, unsigned long long* conf) {
  __syncthreads();
  for (int k = threadIdx.x; k < C * C; k += blockDim.x)
    if (hist[k]) atomicAdd(conf + k, (unsigned long long)hist[k]);
}

// Four consecutive pixels of one row per lane, in groups aligned to the ABSOLUTE column (a multiple of 4 at or left of the
// window's first column): with W % 4 == 0 and a 16-byte aligned map every group is one 16-byte load per class plane, for
// any window offset, and stays inside its row of the padded map (columns outside the window are read, not used).  Other
// maps read the four floats one by one.
__global__ __launch_bounds__(256) void eval_argmax_k(const float* __restrict__ prob, int C, int H, int W, int top, int left,
                                                     int h, int w, const float* __restrict__ label,
                                                     int32_t* __restrict__ amap, unsigned long long* __restrict__ conf) {
  __shared__ unsigned hist[EV_MAXC * EV_MAXC];
  if (conf) ev_hist_zero(hist, C);
  const int64_t HW = (int64_t)H * W;
  const int a0 = left & ~3;
  const int wq = (left + w - a0 + 3) >> 2;
  const int64_t n4 = (int64_t)h * wq;
  const bool vec = (W & 3) == 0 && (((uintptr_t)prob) & 15) == 0;
  for (int64_t q = blockIdx.x * (int64_t)256 + threadIdx.x; q < n4; q += (int64_t)gridDim.x * 256) {
    const int r = (int)(q / wq), a = a0 + (int)(q - (int64_t)r * wq) * 4;     // absolute column of the group
    const float* base = prob + (int64_t)(top + r) * W + a;
    float best[4] = {0.f, 0.f, 0.f, 0.f};
    int bi[4] = {0, 0, 0, 0};
    for (int c = 0; c < C; ++c) {
      const float* pc = base + (int64_t)c * HW;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (vec) {
        const f32x4 t = *(const f32x4*)pc;
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) if (a + k >= left && a + k < left + w) v[k] = pc[k];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) ev_take(v[k], c, best[k], bi[k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int col = a + k - left;
      if (col < 0 || col >= w) continue;
      const int64_t o = (int64_t)r * w + col;
      if (amap) amap[o] = bi[k];
      if (conf) {
        const int t = (int)label[o];
        if (t >= 0 && t < C) atomicAdd(&hist[bi[k] * C + t], 1u);
      }
    }
  }
  if (conf) ev_hist_flush(hist, C, conf);
}

static bool ev_window_ok(int C, int H, int W, int top, int left, int h, int w) {
  return C >= 1 && h >= 1 && w >= 1 && top >= 0 && left >= 0 && top + h <= H && left + w <= W;
}

extern "C" int pmf_eval_argmax(const float* prob, int32_t C, int32_t H, int32_t W, int32_t top, int32_t left, int32_t h,
                               int32_t w, const float* label, int32_t* argmax, int64_t* conf, pmf_stream_t s) {
  if (!prob || !ev_window_ok(C, H, W, top, left, h, w)) return PMF_E_ARG;
  if (conf && (!label || C > EV_MAXC)) return PMF_E_ARG;
  if (!argmax && !conf) return 0;
  const int64_t n4 = (int64_t)h * ((left + w - (left & ~3) + 3) >> 2);
  const int64_t g = cdiv64(n4, 256);
  hipLaunchKernelGGL(eval_argmax_k, dim3((unsigned)(g < EV_GRID ? g : EV_GRID)), dim3(256), 0, (hipStream_t)s, prob, C, H,
                     W, top, left, h, w, label, argmax, (unsigned long long*)conf);
  PMF_LAUNCH_CHECK();
  return 0;
}

// ---- (c) point labels + point confusion ------------------------------------------------------------------------------
// KNN path: the vote of knn.hip (knn_vote_batch_impl, one frame) reads int64 pixel coordinates and an offsets table:
// px = column, py = row of the kept point inside the box (the reference's uproj_y_idx / uproj_x_idx).
__global__ __launch_bounds__(256) void eval_knn_prep_k(const int32_t* __restrict__ xd, const int32_t* __restrict__ yd,
                                                       int x_min, int y_min, int64_t K, int64_t* __restrict__ px,
                                                       int64_t* __restrict__ py, int64_t* __restrict__ off) {
  const int64_t k = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (k < K) {
    px[k] = (int64_t)yd[k] - y_min;
    py[k] = (int64_t)xd[k] - x_min;
  }
  if (k == 0) { off[0] = 0; off[1] = K; }
}

// One lane per kept point: its label (the vote's, or the argmax of the C probabilities at its pixel), the inverse-mapped
// annotation id and the (pred, lut[sem[src]]) count.  Box-relative coordinates outside the window (not produced by the
// loader: its box is the points' own) read nothing and give class 0.
__global__ __launch_bounds__(256) void eval_points_k(const float* __restrict__ prob, int C, int H, int W, int top, int left,
                                                     int h, int w, const int32_t* __restrict__ xd,
                                                     const int32_t* __restrict__ yd, int x_min, int y_min, int64_t K,
                                                     const int64_t* __restrict__ voted, const int32_t* __restrict__ sem,
                                                     const int32_t* __restrict__ src, const int32_t* __restrict__ lut,
                                                     int nlut, unsigned long long* __restrict__ conf,
                                                     const int32_t* __restrict__ lut_inv, int nlut_inv,
                                                     int32_t* __restrict__ labels, uint32_t* __restrict__ labels_inv) {
  __shared__ unsigned hist[EV_MAXC * EV_MAXC];
  if (conf) ev_hist_zero(hist, C);
  const int64_t HW = (int64_t)H * W;
  for (int64_t k = blockIdx.x * (int64_t)256 + threadIdx.x; k < K; k += (int64_t)gridDim.x * 256) {
    int pred = 0;
    if (voted) {
      pred = (int)voted[k];
    } else {
      const int r = xd[k] - x_min, c = yd[k] - y_min;
      if (r >= 0 && r < h && c >= 0 && c < w) {
        const float* p = prob + (int64_t)(top + r) * W + left + c;
        float best = 0.f;
        for (int j = 0; j < C; ++j) ev_take(p[(int64_t)j * HW], j, best, pred);
      }
    }
    if (labels) labels[k] = pred;
    if (labels_inv) labels_inv[k] = (uint32_t)((pred >= 0 && pred < nlut_inv) ? lut_inv[pred] : 0);
    if (conf) {
      const int sl = sem[src ? src[k] : k];
      const int t = (sl >= 0 && sl < nlut) ? lut[sl] : 0;
      if (t >= 0 && t < C && pred >= 0 && pred < C) atomicAdd(&hist[pred * C + t], 1u);
    }
  }
  if (conf) ev_hist_flush(hist, C, conf);
}

extern "C" int pmf_eval_points(const float* prob, int32_t C, int32_t H, int32_t W, int32_t top, int32_t left, int32_t h,
                               int32_t w, const int32_t* x_data, const int32_t* y_data, int32_t x_min, int32_t y_min,
                               int64_t K, const int32_t* argmax, const float* proj_range, const float* unproj_range,
                               int32_t knn, int32_t search, const float* inv_gauss, float cutoff, int64_t* knn_ws,
                               const int32_t* sem, const int32_t* src_idx, const int32_t* lut, int32_t nlut,
                               int64_t* conf, const int32_t* lut_inv, int32_t nlut_inv, int32_t* labels,
                               uint32_t* labels_inv, pmf_stream_t s) {
  if (!ev_window_ok(C, H, W, top, left, h, w) || K < 0) return PMF_E_ARG;
  if (K == 0) return 0;
  if (!x_data || !y_data) return PMF_E_ARG;
  if (conf && (!sem || !lut || nlut < 1 || C > EV_MAXC)) return PMF_E_ARG;
  if (labels_inv && (!lut_inv || nlut_inv < 1)) return PMF_E_ARG;
  hipStream_t st = (hipStream_t)s;
  const int64_t* voted = nullptr;
  if (argmax) {                                   // KNN: ws = px[K] | py[K] | offsets[2] | labels[K]
    if (!proj_range || !unproj_range || !inv_gauss || !knn_ws) return PMF_E_ARG;
    int64_t *px = knn_ws, *py = knn_ws + K, *off = knn_ws + 2 * K, *lab = knn_ws + 2 * K + 2;
    hipLaunchKernelGGL(eval_knn_prep_k, dim3((unsigned)cdiv64(K, 256)), dim3(256), 0, st, x_data, y_data, x_min, y_min, K,
                       px, py, off);
    PMF_LAUNCH_CHECK();
    const int rc = knn_vote_batch_impl(proj_range, unproj_range, nullptr, argmax, px, py, off, 1, h, w, K, knn, search,
                                       inv_gauss, cutoff, C, lab, s);
    if (rc != 0) return rc;
    voted = lab;
  } else if (!prob) {
    return PMF_E_ARG;
  }
  const int64_t g = cdiv64(K, 256);
  hipLaunchKernelGGL(eval_points_k, dim3((unsigned)(g < EV_GRID ? g : EV_GRID)), dim3(256), 0, st, prob, C, H, W, top,
                     left, h, w, x_data, y_data, x_min, y_min, K, voted, sem, src_idx, lut, nlut,
                     (unsigned long long*)conf, lut_inv, nlut_inv, labels, labels_inv);
  PMF_LAUNCH_CHECK();
  return 0;
}

// ---- (d) nuScenes: six views per sweep, merged on the device as they arrive ----------------------------------------------
// (tasks/epmf_eval_nuscenes/infer.py of the reference: a running (confidence, label) pair per LiDAR point of the sweep; a
// later view overwrites a point only where it is STRICTLY more confident; after the sixth view the points some camera
// labelled non-zero are scored.)  The state conf_full f32[P] / label_full int32[P] lives on the device, zero at the start of
// a sweep; pmf_eval_sweep_finish zeroes it again.
//
// KNN mode: the reference sends the float confidence map through the same KNN module as the argmax map, and that module
// casts its map to int64 -- so the "confidence" that enters the merge is the vote over trunc(confidence), an integer
// class id cast back to float (1.0 for practically every point of a softmax map: the first view that sees a point keeps
// it).  That is a quirk of the reference, reproduced here so labels agree in both modes; gather mode is its default.
__global__ __launch_bounds__(256) void eval_conf_trunc_k(const float* __restrict__ prob, int C, int H, int W, int top,
                                                         int left, int h, int w, int32_t* __restrict__ cmap) {
  const int64_t HW = (int64_t)H * W, hw = (int64_t)h * w;
  for (int64_t o = blockIdx.x * (int64_t)256 + threadIdx.x; o < hw; o += (int64_t)gridDim.x * 256) {
    const int r = (int)(o / w), c = (int)(o - (int64_t)r * w);
    const float* p = prob + (int64_t)(top + r) * W + left + c;
    float best = 0.f;
    int bi = 0;
    for (int j = 0; j < C; ++j) ev_take(p[(int64_t)j * HW], j, best, bi);
    cmap[o] = (best == best && fabsf(best) < 2.0e9f) ? (int)best : 0;        // .long(): towards zero; NaN -> no class
  }
}

// One lane per kept point of the view: coalesced x / y / src (and vote) reads, C strided plane reads at its pixel.
// No atomics: inside one view src has no duplicates (every kept point is one point of the sweep), and the views of a
// sweep are launched on one stream in order, so each (conf_full[p], label_full[p]) pair has a single writer at a time.
__global__ __launch_bounds__(256) void eval_view_merge_k(const float* __restrict__ prob, int C, int H, int W, int top,
                                                         int left, int h, int w, const int32_t* __restrict__ xd,
                                                         const int32_t* __restrict__ yd, int x_min, int y_min, int64_t K,
                                                         const int32_t* __restrict__ src, int64_t P,
                                                         const int64_t* __restrict__ vlab, const int64_t* __restrict__ vconf,
                                                         float* __restrict__ conf_full, int32_t* __restrict__ label_full) {
  const int64_t HW = (int64_t)H * W;
  const int64_t k = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (k >= K) return;
  float conf = 0.f;
  int pred = 0;
  if (vlab) {
    pred = (int)vlab[k];
    conf = (float)vconf[k];
  } else {
    const int r = xd[k] - x_min, c = yd[k] - y_min;
    if (r >= 0 && r < h && c >= 0 && c < w) {
      const float* p = prob + (int64_t)(top + r) * W + left + c;
      for (int j = 0; j < C; ++j) ev_take(p[(int64_t)j * HW], j, conf, pred);   // pred_output[0].max(dim=0)
    }
  }
  const int64_t p = src[k];
  if (p < 0 || p >= P) return;
  if (conf_full[p] < conf) {          // strict: the earlier view wins a tie, a NaN confidence never wins
    conf_full[p] = conf;
    label_full[p] = pred;
  }
}

extern "C" int pmf_eval_view_merge(const float* prob, int32_t C, int32_t H, int32_t W, int32_t top, int32_t left, int32_t h,
                                   int32_t w, const int32_t* x_data, const int32_t* y_data, int32_t x_min, int32_t y_min,
                                   int64_t K, const int32_t* src_idx, int64_t P, const int32_t* argmax,
                                   const float* proj_range, const float* unproj_range, int32_t knn, int32_t search,
                                   const float* inv_gauss, float cutoff, int64_t* knn_ws, int32_t* conf_ws,
                                   float* conf_full, int32_t* label_full, pmf_stream_t s) {
  if (!ev_window_ok(C, H, W, top, left, h, w) || K < 0 || P < 0 || C > EV_MAXC) return PMF_E_ARG;
  if (K == 0) return 0;
  if (!prob || !x_data || !y_data || !src_idx || !conf_full || !label_full) return PMF_E_ARG;
  hipStream_t st = (hipStream_t)s;
  const int64_t *vlab = nullptr, *vconf = nullptr;
  if (argmax) {                                   // KNN: ws = px[K] | py[K] | offsets[2] | labels[K] | confidences[K]
    if (!proj_range || !unproj_range || !inv_gauss || !knn_ws || !conf_ws) return PMF_E_ARG;
    int64_t *px = knn_ws, *py = knn_ws + K, *off = knn_ws + 2 * K, *lab = knn_ws + 2 * K + 2, *cf = knn_ws + 3 * K + 2;
    hipLaunchKernelGGL(eval_knn_prep_k, dim3((unsigned)cdiv64(K, 256)), dim3(256), 0, st, x_data, y_data, x_min, y_min, K,
                       px, py, off);
    const int64_t g = cdiv64((int64_t)h * w, 256);
    hipLaunchKernelGGL(eval_conf_trunc_k, dim3((unsigned)(g < 2048 ? g : 2048)), dim3(256), 0, st, prob, C, H, W, top, left,
                       h, w, conf_ws);
    PMF_LAUNCH_CHECK();
    int rc = knn_vote_batch_impl(proj_range, unproj_range, nullptr, argmax, px, py, off, 1, h, w, K, knn, search, inv_gauss,
                                 cutoff, C, lab, s);
    if (rc != 0) return rc;
    rc = knn_vote_batch_impl(proj_range, unproj_range, nullptr, conf_ws, px, py, off, 1, h, w, K, knn, search, inv_gauss,
                             cutoff, C, cf, s);
    if (rc != 0) return rc;
    vlab = lab;
    vconf = cf;
  }
  hipLaunchKernelGGL(eval_view_merge_k, dim3((unsigned)cdiv64(K, 256)), dim3(256), 0, st, prob, C, H, W, top, left, h, w,
                     x_data, y_data, x_min, y_min, K, src_idx, P, vlab, vconf, conf_full, label_full);
  PMF_LAUNCH_CHECK();
  return 0;
}

// One lane per point of the sweep: the merged label, the (pred, gt) count over the points some camera labelled non-zero
// (gt = lut[sem] * (pred != 0): the others land in the ignored cell [0][0]), the uint8 label, and the state back to zero.
__global__ __launch_bounds__(256) void eval_sweep_finish_k(float* __restrict__ conf_full, int32_t* __restrict__ label_full,
                                                           int64_t P, const int32_t* __restrict__ sem,
                                                           const int32_t* __restrict__ lut, int nlut, int C,
                                                           unsigned long long* __restrict__ conf,
                                                           uint8_t* __restrict__ out_u8) {
  __shared__ unsigned hist[EV_MAXC * EV_MAXC];
  if (conf) ev_hist_zero(hist, C);
  for (int64_t p = blockIdx.x * (int64_t)256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256) {
    const int pred = label_full[p];
    if (conf) {
      const int sl = sem[p];
      const int t = (pred != 0 && sl >= 0 && sl < nlut) ? lut[sl] : 0;
      if (t >= 0 && t < C && pred >= 0 && pred < C) atomicAdd(&hist[pred * C + t], 1u);
    }
    if (out_u8) out_u8[p] = (uint8_t)pred;
    conf_full[p] = 0.f;
    label_full[p] = 0;
  }
  if (conf) ev_hist_flush(hist, C, conf);
}

extern "C" int pmf_eval_sweep_finish(float* conf_full, int32_t* label_full, int64_t P, const int32_t* sem,
                                     const int32_t* lut, int32_t nlut, int32_t C, int64_t* conf, uint8_t* out_u8,
                                     pmf_stream_t s) {
  if (P < 0 || C < 1 || C > EV_MAXC) return PMF_E_ARG;
  if (P == 0) return 0;
  if (!conf_full || !label_full) return PMF_E_ARG;
  if (conf && (!sem || !lut || nlut < 1)) return PMF_E_ARG;
  const int64_t g = cdiv64(P, 256);
  hipLaunchKernelGGL(eval_sweep_finish_k, dim3((unsigned)(g < EV_GRID ? g : EV_GRID)), dim3(256), 0, (hipStream_t)s,
                     conf_full, label_full, P, sem, lut, nlut, C, (unsigned long long*)conf, out_u8);
  PMF_LAUNCH_CHECK();
  return 0;
}

// ---- (f) full sweeps: the camera labels filled from a LiDAR-only prediction ---------------------------------------------
// (tasks/pmf_eval_nuscenes/testset_eval/main.py of the reference, MergePred: where the camera model said 0 the LiDAR-only
// label is taken, what is still 0 becomes one fixed class, and ALL points are scored: no pred != 0 gate on the ground
// truth.)  ev_fill_point is the one statement of that rule; the batched pass and the online sweep finish both call it.
// n[3] are the lane's running counts by source: taken from the main prediction / from the sub prediction / filled.
__device__ __forceinline__ void ev_fill_point(int main_pred, int sub_pred, int fill_class, int64_t p,
                                              const int32_t* __restrict__ sem,
                                              const int32_t* __restrict__ lut, int nlut, int C, unsigned* hist,
                                              uint8_t* __restrict__ out_u8, unsigned (&n)[3]) {
  int pred = main_pred != 0 ? main_pred : sub_pred;
  int source = main_pred != 0 ? 0 : 1;
  if (pred == 0) { pred = fill_class; source = 2; }
  if (out_u8) out_u8[p] = (uint8_t)pred;                 // modulo 256, as numpy's astype(uint8)
  if (hist) {
    const int sl = sem[p];
    const int t = (sl >= 0 && sl < nlut) ? lut[sl] : 0;
    if (t >= 0 && t < C && pred >= 0 && pred < C) atomicAdd(&hist[pred * C + t], 1u);
  }
  n[0] += source == 0;
  n[1] += source == 1;
  n[2] += source == 2;
}

// The workgroup's three source counts: a shuffle reduction per wave, one LDS slot per wave, then one 64-bit atomic per
// count and workgroup.  Every lane of the workgroup calls it (it holds a barrier).
__device__ __forceinline__ void ev_counts_flush(const unsigned (&n)[3], unsigned (*wave_n)[3], unsigned long long* counts) {
  unsigned v[3] = {n[0], n[1], n[2]};
#pragma unroll
  for (int k = 0; k < 3; ++k)
    for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_down(v[k], d, 64);
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < 3; ++k) wave_n[threadIdx.x >> 6][k] = v[k];
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long t = 0;
    for (int wv = 0; wv < (int)(blockDim.x >> 6); ++wv) t += wave_n[wv][threadIdx.x];
    if (t) atomicAdd(counts + threadIdx.x, t);
  }
}

// One lane per point of the concatenated sweeps: two coalesced int32 reads, one byte out.
__global__ __launch_bounds__(256) void eval_fill_k(const int32_t* __restrict__ main_pred,
                                                   const int32_t* __restrict__ sub_pred, int64_t P, int fill_class,
                                                   const int32_t* __restrict__ sem,
                                                   const int32_t* __restrict__ lut, int nlut, int C,
                                                   unsigned long long* __restrict__ conf,
                                                   unsigned long long* __restrict__ counts, uint8_t* __restrict__ out_u8) {
  __shared__ unsigned hist[EV_MAXC * EV_MAXC];
  __shared__ unsigned wave_n[4][3];
  if (conf) ev_hist_zero(hist, C);
  unsigned n[3] = {0u, 0u, 0u};
  for (int64_t p = blockIdx.x * (int64_t)256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256)
    ev_fill_point(main_pred[p], sub_pred[p], fill_class, p, sem, lut, nlut, C, conf ? hist : nullptr, out_u8, n);
  if (conf) ev_hist_flush(hist, C, conf);
  if (counts) ev_counts_flush(n, wave_n, counts);
}

extern "C" int pmf_eval_fill(const int32_t* main_pred, const int32_t* sub_pred, int64_t P, int32_t fill_class,
                             const int32_t* sem, const int32_t* lut, int32_t nlut, int32_t C, int64_t* conf,
                             int64_t* counts, uint8_t* out_u8, pmf_stream_t s) {
  if (P < 0 || C < 1 || C > EV_MAXC) return PMF_E_ARG;
  if (P == 0) return 0;
  if (!main_pred || !sub_pred) return PMF_E_ARG;
  if (conf && (!sem || !lut || nlut < 1)) return PMF_E_ARG;
  if (!conf && !counts && !out_u8) return 0;
  const int64_t g = cdiv64(P, 256);
  hipLaunchKernelGGL(eval_fill_k, dim3((unsigned)(g < EV_GRID ? g : EV_GRID)), dim3(256), 0, (hipStream_t)s, main_pred,
                     sub_pred, P, fill_class, sem, lut, nlut, C, (unsigned long long*)conf, (unsigned long long*)counts,
                     out_u8);
  PMF_LAUNCH_CHECK();
  return 0;
}

// eval_sweep_finish_k and the fill in one pass over the sweep: the camera-only count keeps its pred != 0 gate and its own
// histogram, the fused count and labels come from ev_fill_point with main_pred = the merged camera label; the state is
// read once and zeroed.  The extra traffic over the plain finish is one int32 read (sub_pred[p]) per point.
__global__ __launch_bounds__(256) void eval_sweep_finish_fill_k(float* __restrict__ conf_full,
                                                                int32_t* __restrict__ label_full,
                                                                int64_t P, const int32_t* __restrict__ sub_pred,
                                                                int fill_class, const int32_t* __restrict__ sem,
                                                                const int32_t* __restrict__ lut, int nlut, int C,
                                                                unsigned long long* __restrict__ conf_cam,
                                                                unsigned long long* __restrict__ conf_fused,
                                                                unsigned long long* __restrict__ counts,
                                                                uint8_t* __restrict__ out_cam_u8,
                                                                uint8_t* __restrict__ out_u8) {
  __shared__ unsigned hist_cam[EV_MAXC * EV_MAXC];
  __shared__ unsigned hist[EV_MAXC * EV_MAXC];
  __shared__ unsigned wave_n[4][3];
  if (conf_cam) ev_hist_zero(hist_cam, C);
  if (conf_fused) ev_hist_zero(hist, C);
  unsigned n[3] = {0u, 0u, 0u};
  for (int64_t p = blockIdx.x * (int64_t)256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256) {
    const int pred = label_full[p];
    if (conf_cam) {
      const int sl = sem[p];
      const int t = (pred != 0 && sl >= 0 && sl < nlut) ? lut[sl] : 0;
      if (t >= 0 && t < C && pred >= 0 && pred < C) atomicAdd(&hist_cam[pred * C + t], 1u);
    }
    if (out_cam_u8) out_cam_u8[p] = (uint8_t)pred;
    ev_fill_point(pred, sub_pred[p], fill_class, p, sem, lut, nlut, C, conf_fused ? hist : nullptr, out_u8, n);
    conf_full[p] = 0.f;
    label_full[p] = 0;
  }
  if (conf_cam) ev_hist_flush(hist_cam, C, conf_cam);
  if (conf_fused) ev_hist_flush(hist, C, conf_fused);
  if (counts) ev_counts_flush(n, wave_n, counts);
}

extern "C" int pmf_eval_sweep_finish_fill(float* conf_full, int32_t* label_full, int64_t P, const int32_t* sub_pred,
                                          int32_t fill_class, const int32_t* sem, const int32_t* lut, int32_t nlut,
                                          int32_t C, int64_t* conf_cam, int64_t* conf_fused, int64_t* counts,
                                          uint8_t* out_cam_u8, uint8_t* out_u8, pmf_stream_t s) {
  if (P < 0 || C < 1 || C > EV_MAXC) return PMF_E_ARG;
  if (P == 0) return 0;
  if (!conf_full || !label_full || !sub_pred) return PMF_E_ARG;
  if ((conf_cam || conf_fused) && (!sem || !lut || nlut < 1)) return PMF_E_ARG;
  const int64_t g = cdiv64(P, 256);
  hipLaunchKernelGGL(eval_sweep_finish_fill_k, dim3((unsigned)(g < EV_GRID ? g : EV_GRID)), dim3(256), 0, (hipStream_t)s,
                     conf_full, label_full, P, sub_pred, fill_class, sem, lut, nlut, C, (unsigned long long*)conf_cam,
                     (unsigned long long*)conf_fused, (unsigned long long*)counts, out_cam_u8, out_u8);
  PMF_LAUNCH_CHECK();
  return 0;
}

// ---- (e) SalsaNext range images: B sweeps per call ---------------------------------------------------------------------
// (tasks/salsanext_eval_nuscenes/infer.py:90-119 of the reference, per sweep: argmax, IOUEval.addBatch on the pixels, KNN or
// pred_argmax[uproj_y_idx, uproj_x_idx], .cpu(), IOUEval.addBatch on the points.)  Every sweep has the same H x W, so the B
// maps of a forward are one [B, C, H, W] tensor and everything behind the network is two launches: the vote reads the
// FINISHED argmax of its neighbours, so the map stage and the point stage cannot share one.
// Map stage: one lane per pixel of the B maps (C coalesced plane reads), int32 argmax + pixel confusion.
__global__ __launch_bounds__(256) void eval_range_map_k(const float* __restrict__ prob, int C, int64_t HW, int64_t total,
                                                        const float* __restrict__ label, int32_t* __restrict__ amap,
                                                        unsigned long long* __restrict__ conf) {
  __shared__ unsigned hist[EV_MAXC * EV_MAXC];
  if (conf) ev_hist_zero(hist, C);
  for (int64_t q = blockIdx.x * (int64_t)256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
    const int64_t b = q / HW;
    const float* p = prob + b * C * HW + (q - b * HW);
    float best = 0.f;
    int bi = 0;
    for (int c = 0; c < C; ++c) ev_take(p[(int64_t)c * HW], c, best, bi);
    amap[q] = bi;
    if (conf) {
      const int t = (int)label[q];
      if (t >= 0 && t < C) atomicAdd(&hist[bi * C + t], 1u);
    }
  }
  if (conf) ev_hist_flush(hist, C, conf);
}

// Point stage: one lane per point, a workgroup is 256 consecutive points of ONE sweep (knn_wg_frame: the offsets table is
// walked once per workgroup with scalar loads, not per lane).  S = 0: the label at the point's pixel; 3 / 5: the vote of
// knn_vote.h with the window staged through LDS; 7: gathered window; -1: any other odd window.  The same device
// functions as pmf_knn_vote: bit-identical labels.  The label goes out as int32 and into the workgroup's histogram.
template <int S>
__global__ __launch_bounds__(256) void eval_range_points_k(const int32_t* __restrict__ amap, const float* __restrict__ pr,
                                                           int B, int H, int W, const int64_t* __restrict__ offsets,
                                                           int64_t P_total, const int32_t* __restrict__ px,
                                                           const int32_t* __restrict__ py, const float* __restrict__ ur,
                                                           int knn, int search, const float* __restrict__ invg, float cutoff,
                                                           int C, const int32_t* __restrict__ sem,
                                                           const int32_t* __restrict__ lut, int nlut,
                                                           int32_t* __restrict__ labels,
                                                           unsigned long long* __restrict__ conf) {
  __shared__ unsigned hist[EV_MAXC * EV_MAXC];
  int b, wg;
  int64_t lo, hi;
  knn_wg_frame(offsets, B, 0, b, wg, lo, hi);
  if (b < 0) return;                                    // (the grid is an upper bound; uniform over the workgroup)
  if (conf) ev_hist_zero(hist, C);
  const int64_t i = lo + (int64_t)wg * 256 + threadIdx.x;
  const bool valid = i < hi && i >= 0 && i < P_total;
  const int32_t* __restrict__ amb = amap + (size_t)b * H * W;
  int cx = 0, cy = 0;
  if (valid) { cx = px[i]; cy = py[i]; }
  int pred = 0;
  if constexpr (S == 0) {
    if (valid && cx >= 0 && cx < W && cy >= 0 && cy < H) pred = amb[(size_t)cy * W + cx];
  } else {
    const float* __restrict__ prb = pr + (size_t)b * H * W;
    const float r = valid ? ur[i] : 0.f;
    if constexpr (S == 3 || S == 5) {
      pred = knn_vote_lds<S>(prb, nullptr, amb, valid, cx, cy, r, H, W, knn, invg, cutoff, C);
    } else if constexpr (S == 7) {
      if (valid) pred = knn_vote_gather<7>(prb, nullptr, amb, cx, cy, r, H, W, knn, invg, cutoff, C);
    } else {
      if (valid) pred = knn_vote_any(prb, nullptr, amb, cx, cy, r, H, W, knn, search, invg, cutoff, C);
    }
  }
  if (valid) {
    labels[i] = pred;
    if (conf) {
      const int sl = sem[i];
      const int t = (sl >= 0 && sl < nlut) ? lut[sl] : 0;
      if (t >= 0 && t < C && pred >= 0 && pred < C) atomicAdd(&hist[pred * C + t], 1u);
    }
  }
  if (conf) ev_hist_flush(hist, C, conf);
}

extern "C" int pmf_eval_range_batch(const float* prob, int32_t B, int32_t C, int32_t H, int32_t W, const float* label,
                                    const float* proj_range, const int64_t* offsets, int64_t P_total, const int32_t* px,
                                    const int32_t* py, const float* unproj_range, const int32_t* sem, const int32_t* lut,
                                    int32_t nlut, int32_t knn, int32_t search, const float* inv_gauss, float cutoff,
                                    int32_t* argmax_ws, int32_t* labels, int64_t* pixel_conf, int64_t* point_conf,
                                    pmf_stream_t s) {
  if (B < 0 || B > 1024 || C < 1 || C > EV_MAXC || H < 1 || W < 1 || P_total < 0 || knn < 0) return PMF_E_ARG;
  if (knn > 0) {
    if (search % 2 == 0 || search < 1 || search > 255) return PMF_E_ARG;      // knn.py:73-74 raises ValueError
    if (knn > 8 || knn > search * search) return PMF_E_UNSUPPORTED;
  }
  if (B == 0) return 0;
  if (!prob || !argmax_ws || (pixel_conf && !label)) return PMF_E_ARG;
  hipStream_t st = (hipStream_t)s;
  const int64_t total = (int64_t)B * H * W;
  const int64_t g = cdiv64(total, 256);
  hipLaunchKernelGGL(eval_range_map_k, dim3((unsigned)(g < EV_GRID ? g : EV_GRID)), dim3(256), 0, st, prob, C,
                     (int64_t)H * W, total, label, argmax_ws, (unsigned long long*)pixel_conf);
  PMF_LAUNCH_CHECK();
  if (P_total == 0) return 0;
  if (!offsets || !px || !py || !labels) return PMF_E_ARG;
  if (point_conf && (!sem || !lut || nlut < 1)) return PMF_E_ARG;
  if (knn > 0 && (!proj_range || !unproj_range || !inv_gauss)) return PMF_E_ARG;
  const dim3 grid((unsigned)(cdiv64(P_total, 256) + B)), block(256);        // sum_b ceil(n_b / 256) <= ceil(P / 256) + B
#define EV_RANGE_POINTS(S)                                                                                                 \
  hipLaunchKernelGGL(eval_range_points_k<S>, grid, block, 0, st, argmax_ws, proj_range, B, H, W, offsets, P_total, px, py, \
                     unproj_range, knn, search, inv_gauss, cutoff, C, sem, lut, nlut, labels,                              \
                     (unsigned long long*)point_conf)
  if (knn == 0) EV_RANGE_POINTS(0);
  else if (search == 3) EV_RANGE_POINTS(3);
  else if (search == 5) EV_RANGE_POINTS(5);
  else if (search == 7) EV_RANGE_POINTS(7);
  else EV_RANGE_POINTS(-1);
#undef EV_RANGE_POINTS
  PMF_LAUNCH_CHECK();
  return 0;
}
