// The KNN vote of one point (pc_processor/postproc/knn.py:55-143) as device functions: the kernels of knn.hip and the batched
// range-image evaluation of eval.hip are built from these, so there is ONE statement of the window, the selection and
// the vote.  The caller resolves the frame (map pointers of the point's frame), the point's pixel (cx = column, cy = row)
// and its range r, and stores the returned label in its own format.
//   knn_vote_gather<S>  window taps gathered from global memory, window in registers (S = 3, 5, 7)
//   knn_vote_lds<S>     256 consecutive points of ONE frame: the bounding box of the workgroup staged through LDS (S = 3, 5)
//   knn_vote_any        any odd window, size at run time
// All three give the same label: k x first-minimum selection, ties -> smaller window index; vote ties -> lower class.
#pragma once
#include "common.h"
#pragma clang fp contract(off)

#define KNN_LDS_PIX 4096

// (range, label) of window tap (y, x): F.unfold zero padding outside the image, a negative range counts as +inf
__device__ __forceinline__ void knn_tap(const float* __restrict__ prb, const int64_t* __restrict__ amb,
                                        const int32_t* __restrict__ amb32, int y, int x, int H, int W, float& v, int& l) {
  v = 0.f;
  l = 0;
  if (y >= 0 && y < H && x >= 0 && x < W) {
    v = prb[(size_t)y * W + x];
    l = amb32 ? amb32[(size_t)y * W + x] : (int)amb[(size_t)y * W + x];
    if (v < 0.f) v = INFINITY;
  }
}

// the vote over the nsel selected labels: the most frequent class of 1 .. nclasses-1, ties -> lower class, none -> 1
__device__ __forceinline__ int knn_majority(const int* sel, int nsel, int nclasses) {
  int best_cnt = 0, best_cls = 1;
  for (int a = 0; a < nsel; ++a) {
    const int cls = sel[a];
    if (cls < 1 || cls >= nclasses) continue;
    int cnt = 0;
    for (int c = 0; c < nsel; ++c) cnt += sel[c] == cls;
    if (cnt > best_cnt || (cnt == best_cnt && cls < best_cls)) { best_cnt = cnt; best_cls = cls; }
  }
  return best_cls;
}

// wts: the S*S inverse-Gaussian weights (LDS or global)
template <int S>
__device__ __forceinline__ int knn_vote_gather(const float* __restrict__ prb, const int64_t* __restrict__ amb,
                                               const int32_t* __restrict__ amb32, int cx, int cy, float r, int H, int W,
                                               int knn, const float* wts, float cutoff, int nclasses) {
  constexpr int S2 = S * S, PAD = (S - 1) / 2, CENTER = (S2 - 1) / 2;
  float dist[S2];
  int lab[S2];
#pragma unroll
  for (int t = 0; t < S2; ++t) {
    float v;
    int l;
    knn_tap(prb, amb, amb32, cy + t / S - PAD, cx + t % S - PAD, H, W, v, l);
    if (t == CENTER) v = r;
    dist[t] = fabsf(v - r) * wts[t];   // |neigh - range| * (1 - gauss), float32, knn.py:97-108
    lab[t] = l;
  }
  // k x first-minimum selection
  unsigned long long used = 0ull;
  int sel[8];
  const int nsel = knn < 8 ? knn : 8;
  for (int k = 0; k < nsel; ++k) {
    float best = 0.f;
    int bi = -1;
#pragma unroll
    for (int t = 0; t < S2; ++t) {
      const bool free_ = !((used >> t) & 1ull);
      if (free_ && (bi < 0 || dist[t] < best)) { best = dist[t]; bi = t; }
    }
    used |= 1ull << bi;
    int l = 0;
#pragma unroll
    for (int t = 0; t < S2; ++t) if (t == bi) l = lab[t];
    if (cutoff > 0.f && best > cutoff) l = nclasses;
    sel[k] = l;
  }
  return knn_majority(sel, nsel, nclasses);
}

// Any odd window, one lane per point.  k x first-minimum with ties -> smaller window index is what a STABLE insertion into
// an ascending list of length k produces (an equal distance seen later never moves in front of an earlier one); the vote
// only counts labels, so the order inside the list does not matter.  Same float32 arithmetic as knn_vote_gather.
__device__ __forceinline__ int knn_vote_any(const float* __restrict__ prb, const int64_t* __restrict__ amb,
                                            const int32_t* __restrict__ amb32, int cx, int cy, float r, int H, int W,
                                            int knn, int S, const float* __restrict__ invg, float cutoff, int nclasses) {
  const int PAD = (S - 1) / 2, CENTER = (S * S - 1) / 2;
  float bd[8];
  int bl[8];
  const int nsel = knn < 8 ? knn : 8;
#pragma unroll
  for (int k = 0; k < 8; ++k) { bd[k] = INFINITY; bl[k] = 0; }
  int filled = 0;
  for (int ty = 0, t = 0; ty < S; ++ty)
    for (int tx = 0; tx < S; ++tx, ++t) {
      float v;
      int l;
      knn_tap(prb, amb, amb32, cy + ty - PAD, cx + tx - PAD, H, W, v, l);
      if (t == CENTER) v = r;
      float d = fabsf(v - r) * invg[t];
      // position = number of kept entries with distance <= d (stable); NaN-free: distances are >= 0 or +inf
      int pos = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) pos += (k < filled && bd[k] <= d) ? 1 : 0;
      if (pos < nsel) {
#pragma unroll
        for (int k = 7; k > 0; --k)
          if (k > pos && k < nsel) { bd[k] = bd[k - 1]; bl[k] = bl[k - 1]; }
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (k == pos) { bd[k] = d; bl[k] = l; }
        filled = filled < nsel ? filled + 1 : filled;
      }
    }
  int sel[8];
  for (int a = 0; a < nsel; ++a) sel[a] = (cutoff > 0.f && bd[a] > cutoff) ? nclasses : bl[a];
  return knn_majority(sel, nsel, nclasses);
}

// The frame of a workgroup when frame b owns ceil(n_b / 256) consecutive workgroups of 256 points (the grid is
// sum_b ceil(n_b / 256) <= ceil(P / 256) + B workgroups).  offsets == nullptr: one frame of P1 points.  B is small; the
// walk has no early exit so that its scalar loads are independent of each other (one memory latency, not one per frame).
// b < 0: the workgroup is beyond the last frame.
__device__ __forceinline__ void knn_wg_frame(const int64_t* __restrict__ offsets, int B, int64_t P1, int& b, int& wg,
                                             int64_t& lo, int64_t& hi) {
  b = -1; wg = 0; lo = 0; hi = 0;
  if (!offsets) { b = 0; wg = (int)blockIdx.x; hi = P1; return; }
  int first = 0;
  int64_t o0 = offsets[0];
  for (int k = 0; k < B; ++k) {
    const int64_t o1 = offsets[k + 1];
    const int nb = (int)((o1 - o0 + 255) >> 8);
    if (b < 0 && (int)blockIdx.x < first + nb) { b = k; wg = (int)blockIdx.x - first; lo = o0; hi = o1; }
    first += nb;
    o0 = o1;
  }
}

// ---- the vote with the window staged through LDS ----------------------------------------------------------------------
// A gather of one window tap touches one cache line PER LANE when the lanes of a wave sit on different image rows -- and in
// sweep-file order (azimuth by azimuth) consecutive points are the lasers of one column: 50 fully divergent gathers per
// point, the texture-address unit processes them line by line (21 us for 102 k points; random order 33 us).  Here a workgroup
// of 256 consecutive points of ONE frame takes the bounding box of its points (+ the window margin): in sweep order that is
// ~5 columns x all rows, a few hundred pixels; (range, label) of the box are staged into LDS once (rows of the box are
// contiguous: ~10 wave loads per map) and all window taps are read from there.  Zero padding / negative-range handling
// happen at staging time with the same rules, the selection and the vote are those of knn_vote_gather: bit-identical
// labels.  A box above KNN_LDS_PIX pixels (points in random order) uses the global gathers as before, decided per workgroup.
// EVERY lane of the 256-lane workgroup calls this (it has barriers); lanes without a point pass valid = false and ignore
// the result.  32 KB of static LDS.
template <int S>
__device__ __forceinline__ int knn_vote_lds(const float* __restrict__ prb, const int64_t* __restrict__ amb,
                                            const int32_t* __restrict__ amb32, bool valid, int cx, int cy, float r, int H,
                                            int W, int knn, const float* __restrict__ invg, float cutoff, int nclasses) {
  constexpr int S2 = S * S, PAD = (S - 1) / 2, CENTER = (S2 - 1) / 2;
  __shared__ float s_v[KNN_LDS_PIX];
  __shared__ int s_l[KNN_LDS_PIX];
  __shared__ int s_wbox[4][4];          // per wave: min x, max x, min y, max y (no initialisation, no atomics: one barrier less)
  {
    // bounding box: butterfly over the wave, one LDS store per wave and bound.  (Points far outside the image only enlarge
    // the box: it then exceeds the LDS budget and the global path, which clips tap by tap, takes over.)
    int mnx = valid ? cx : 0x7fffffff, mxx = valid ? cx : -0x7fffffff, mny = valid ? cy : 0x7fffffff, mxy = valid ? cy : -0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mnx = min(mnx, __shfl_xor(mnx, o)); mxx = max(mxx, __shfl_xor(mxx, o));
      mny = min(mny, __shfl_xor(mny, o)); mxy = max(mxy, __shfl_xor(mxy, o));
    }
    if ((threadIdx.x & 63) == 0) {
      int* wb = s_wbox[threadIdx.x >> 6];
      wb[0] = mnx; wb[1] = mxx; wb[2] = mny; wb[3] = mxy;
    }
  }
  __syncthreads();
  const int bx0 = min(min(s_wbox[0][0], s_wbox[1][0]), min(s_wbox[2][0], s_wbox[3][0]));
  const int bx1 = max(max(s_wbox[0][1], s_wbox[1][1]), max(s_wbox[2][1], s_wbox[3][1]));
  const int by0 = min(min(s_wbox[0][2], s_wbox[1][2]), min(s_wbox[2][2], s_wbox[3][2]));
  const int by1 = max(max(s_wbox[0][3], s_wbox[1][3]), max(s_wbox[2][3], s_wbox[3][3]));
  const int x0 = bx0 - PAD, y0 = by0 - PAD;
  const long bw = (long)bx1 - bx0 + 1 + 2 * PAD, bh = (long)by1 - by0 + 1 + 2 * PAD;
  const bool staged = bw > 0 && bh > 0 && bw * bh <= KNN_LDS_PIX;
  if (staged) {
    // all loads of the box first (up to 16 pixels per thread, independent), then the LDS stores: one memory latency
    constexpr int PER = KNN_LDS_PIX / 256;
    const int n = (int)(bw * bh), w_ = (int)bw;
    const float inv_w = 1.f / (float)w_;
    float vv[PER];
    int ll[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int j = threadIdx.x + u * 256;
      vv[u] = 0.f; ll[u] = 0;   // F.unfold zero padding: range 0, label 0
      if (j < n) {
        int yy = (int)(((float)j + 0.5f) * inv_w);       // j < 4096, w_ >= S: exact up to one step, corrected below
        int xx = j - yy * w_;
        if (xx < 0) { --yy; xx += w_; } else if (xx >= w_) { ++yy; xx -= w_; }
        const int y = y0 + yy, x = x0 + xx;
        if (y >= 0 && y < H && x >= 0 && x < W) {
          vv[u] = prb[(size_t)y * W + x];
          ll[u] = amb32 ? amb32[(size_t)y * W + x] : (int)amb[(size_t)y * W + x];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int j = threadIdx.x + u * 256;
      if (j < n) { s_v[j] = vv[u] < 0.f ? INFINITY : vv[u]; s_l[j] = ll[u]; }
    }
  }
  __syncthreads();
  if (!valid) return 0;
  float dist[S2];
  int lab[S2];
  if (staged) {
    const int w_ = (int)bw, base = (cy - PAD - y0) * w_ + (cx - PAD - x0);
#pragma unroll
    for (int t = 0; t < S2; ++t) {
      const int j = base + (t / S) * w_ + (t % S);
      float v = s_v[j];
      if (t == CENTER) v = r;
      dist[t] = fabsf(v - r) * invg[t];
      lab[t] = s_l[j];
    }
  } else {
#pragma unroll
    for (int t = 0; t < S2; ++t) {
      float v;
      int l;
      knn_tap(prb, amb, amb32, cy + t / S - PAD, cx + t % S - PAD, H, W, v, l);
      if (t == CENTER) v = r;
      dist[t] = fabsf(v - r) * invg[t];
      lab[t] = l;
    }
  }
  // k x first-minimum selection (ties -> smaller window index), the same rule as knn_vote_gather with a 32-bit taken mask
  // (S2 <= 25 on this path) and the label carried along the scan
  static_assert(S2 <= 32, "taken mask");
  unsigned used = 0u;
  int sel[8];
  const int nsel = knn < 8 ? knn : 8;
  for (int k = 0; k < nsel; ++k) {
    float best = 0.f;
    int bi = -1, l = 0;
#pragma unroll
    for (int t = 0; t < S2; ++t) {
      const bool take = !(used & (1u << t)) && (bi < 0 || dist[t] < best);
      best = take ? dist[t] : best; l = take ? lab[t] : l; bi = take ? t : bi;
    }
    used |= 1u << bi;
    if (cutoff > 0.f && best > cutoff) l = nclasses;
    sel[k] = l;
  }
  return knn_majority(sel, nsel, nclasses);
}
