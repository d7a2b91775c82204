// Dataset preparation of SensatUrban (tasks/sensat_urban/dataset_prepare/compute_bev_feature.py of the reference): the points
// of one block (x y z float32, red green blue uint8[, class uint8]) -> the bird's-eye-view frame the dataset class loads:
// feature_map f64[8,h,w] (max z, min z, mean z, log10(count + 1), mask, RGB of the highest point), label_map f64[h,w] (class of
// the highest point, -1 = empty) and the pixel h_idx / w_idx int32[P] of every point.  The reference is a per-point Python
// loop over a float64 map; every value here equals that loop bit for bit, which fixes three things:
//   * the pixel arithmetic is the reference's numpy promotion: float32 subtraction and a correctly rounded float32 division
//     on the labelled splits, float64 on the test split (both offered, F64 below); no reciprocal, no contraction;
//   * "the first point that attains the maximum wins" and the float64 sum of z are defined by ASCENDING POINT INDEX inside
//     a cell, so a cell's points are put in that order before the update rule is replayed over them -- no floating-point
//     atomics anywhere, integer atomics only for counts and slots (their results do not depend on arrival order);
//   * log10(count + 1) is read from a table the host filled with numpy's log10 (nothing else reproduces it to the bit).
// Passes (the reproducible scatter: store once, then reduce per destination through an inverted index in a fixed order):
//   extent  min / max of x and y (+ a flag for non-finite x y z) -> h, w with the points' own arithmetic (the index is
//           monotone in the coordinate)                                                    (pmf_bev_prepare_extent)
//   bin     per point h_idx, w_idx; counts[cell] += 1                                       (pmf_bev_prepare_bin)
//   scan    exclusive prefix of the counts -> offsets[h*w + 1], the maximum count           (pmf_bev_prepare_scan)
//   place   list[offsets[cell] + slot] = point, slot from an integer atomic (arrival order) (pmf_bev_prepare_place)
//   cells   one lane per cell (the nine float64 rows are written coalesced): the lane walks its points in ascending index
//           by repeated selection (cells hold one to ten points) and replays the update rule in float64.  Cells above
//           BP_LANE_MAX points are queued for one workgroup each: a bitonic network (ascending-only form, so any count
//           works without padding) sorts the cell's index list, in LDS up to BP_LDS_MAX points and in place in the list
//           beyond, then z is gathered 1024 values at a time by all lanes and replayed by one    (pmf_bev_prepare_cells)
// All stores are vector stores.
#include "common.h"
#pragma clang fp contract(off)

#define BP_THREADS 256
#define BP_GRID 1024                            // workgroups of the grid-stride passes (and rows of extent partials)
#define BP_SCAN_ITEMS 8
#define BP_SCAN_BLOCK (BP_THREADS * BP_SCAN_ITEMS)
#define BP_LANE_MAX 32                          // more points than this in a cell: the workgroup path
#define BP_LDS_MAX 4096                         // ... whose index list is sorted in LDS up to this many points
#define BP_CHUNK 1024                           // z values gathered per replay step of the workgroup path

struct BpLayout {                               // byte offsets into the workspace
  int64_t part, counts, offsets, psum, pmax, list, heavy, heavy_n, total;
};

static inline int64_t bp_align(int64_t b) { return (b + 255) & ~(int64_t)255; }

static BpLayout bp_layout(int64_t P, int64_t ncells) {
  BpLayout l;
  int64_t o = 0;
  const int64_t nb = cdiv64(ncells, BP_SCAN_BLOCK);
  l.part = o;     o += bp_align((int64_t)BP_GRID * 4 * sizeof(float));
  l.counts = o;   o += bp_align(ncells * 4);
  l.offsets = o;  o += bp_align((ncells + 1) * 4);
  l.psum = o;     o += bp_align(nb * 4);
  l.pmax = o;     o += bp_align(nb * 4);
  l.list = o;     o += bp_align(ncells ? P * 4 : 0);
  l.heavy = o;    o += bp_align(ncells ? (P / (BP_LANE_MAX + 1) + 1) * 4 : 0);
  l.heavy_n = o;  o += bp_align(4);
  l.total = o;
  return l;
}

static inline bool bp_sizes_ok(int64_t P, int64_t h, int64_t w) {
  return P >= 1 && P < 2147483647LL && h >= 1 && w >= 1 && h <= 2147483646LL / w;
}

__device__ __forceinline__ bool bp_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// the pixel index of a coordinate: trunc((v - vmin) / grid) in the arithmetic of the reference's stacked array; false when
// the quotient does not fit an int32 (numpy's cast is undefined there)
template <bool F64>
__device__ __forceinline__ bool bp_index(float v, float vmin, double grid, float gridf, int32_t* out) {
  double q;
  if (F64) {
    q = ((double)v - (double)vmin) / grid;
  } else {
    const float d = v - vmin;
    q = (double)(d / gridf);
  }
  if (!(q >= 0.0 && q < 2147483647.0)) return false;
  *out = (int32_t)q;
  return true;
}

// ---- extent --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BP_THREADS) void bp_extent_k(const float* __restrict__ x, const float* __restrict__ y,
                                                          const float* __restrict__ z, int P, float* __restrict__ part,
                                                          pmf_bev_extent_t* __restrict__ ext) {
  __shared__ float s[4][BP_THREADS];
  float mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * BP_THREADS + threadIdx.x; i < P; i += (int64_t)gridDim.x * BP_THREADS) {
    const float a = x[i], b = y[i], c = z[i];
    bad |= !(bp_finite(a) && bp_finite(b) && bp_finite(c));
    mnx = fminf(mnx, a); mxx = fmaxf(mxx, a);
    mny = fminf(mny, b); mxy = fmaxf(mxy, b);
  }
  if (bad) atomicOr(&ext->flags, PMF_BEV_NONFINITE);
  const int t = threadIdx.x;
  s[0][t] = mnx; s[1][t] = mny; s[2][t] = mxx; s[3][t] = mxy;
  __syncthreads();
  for (int d = BP_THREADS / 2; d > 0; d >>= 1) {
    if (t < d) {
      s[0][t] = fminf(s[0][t], s[0][t + d]); s[1][t] = fminf(s[1][t], s[1][t + d]);
      s[2][t] = fmaxf(s[2][t], s[2][t + d]); s[3][t] = fmaxf(s[3][t], s[3][t + d]);
    }
    __syncthreads();
  }
  if (t < 4) part[blockIdx.x * 4 + t] = s[t][0];
}

template <bool F64>
__global__ __launch_bounds__(BP_THREADS) void bp_extent_final_k(const float* __restrict__ part, int nparts, double grid,
                                                                float gridf, pmf_bev_extent_t* __restrict__ ext) {
  __shared__ float s[4][BP_THREADS];
  const int t = threadIdx.x;
  float mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
  for (int i = t; i < nparts; i += BP_THREADS) {
    mnx = fminf(mnx, part[i * 4 + 0]); mny = fminf(mny, part[i * 4 + 1]);
    mxx = fmaxf(mxx, part[i * 4 + 2]); mxy = fmaxf(mxy, part[i * 4 + 3]);
  }
  s[0][t] = mnx; s[1][t] = mny; s[2][t] = mxx; s[3][t] = mxy;
  __syncthreads();
  for (int d = BP_THREADS / 2; d > 0; d >>= 1) {
    if (t < d) {
      s[0][t] = fminf(s[0][t], s[0][t + d]); s[1][t] = fminf(s[1][t], s[1][t + d]);
      s[2][t] = fmaxf(s[2][t], s[2][t + d]); s[3][t] = fmaxf(s[3][t], s[3][t + d]);
    }
    __syncthreads();
  }
  if (t == 0) {
    ext->min_x = s[0][0]; ext->min_y = s[1][0]; ext->max_x = s[2][0]; ext->max_y = s[3][0];
    int32_t hi = 0, wi = 0;
    int flags = 0;
    if (!(ext->flags & PMF_BEV_NONFINITE)) {
      if (!bp_index<F64>(s[3][0], s[1][0], grid, gridf, &hi) || !bp_index<F64>(s[2][0], s[0][0], grid, gridf, &wi) ||
          hi >= 2147483646 || wi >= 2147483646)
        flags = PMF_BEV_RANGE;
    }
    ext->h = flags ? 0 : hi + 1;
    ext->w = flags ? 0 : wi + 1;
    if (flags) atomicOr(&ext->flags, flags);
  }
}

// ---- bin -----------------------------------------------------------------------------------------------------------------
template <bool F64>
__global__ __launch_bounds__(BP_THREADS) void bp_bin_k(const float* __restrict__ x, const float* __restrict__ y, int P,
                                                       double grid, float gridf, pmf_bev_extent_t* __restrict__ ext, int h,
                                                       int w, int32_t* __restrict__ h_idx, int32_t* __restrict__ w_idx,
                                                       int32_t* __restrict__ counts) {
  const float min_x = ext->min_x, min_y = ext->min_y;
  for (int64_t i = (int64_t)blockIdx.x * BP_THREADS + threadIdx.x; i < P; i += (int64_t)gridDim.x * BP_THREADS) {
    int32_t hi = 0, wi = 0;
    const bool ok = bp_index<F64>(y[i], min_y, grid, gridf, &hi) && bp_index<F64>(x[i], min_x, grid, gridf, &wi) &&
                    hi < h && wi < w;
    if (!ok) {                                  // cannot happen with the extent of these points: refuse, never write outside
      atomicOr(&ext->flags, PMF_BEV_INTERNAL);
      hi = wi = 0;
    }
    h_idx[i] = hi;
    w_idx[i] = wi;
    if (ok) atomicAdd(&counts[(int64_t)hi * w + wi], 1);
  }
}

// ---- scan ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BP_THREADS) void bp_scan_part_k(const int32_t* __restrict__ counts, int n,
                                                             int32_t* __restrict__ psum, int32_t* __restrict__ pmax) {
  __shared__ int32_t ss[BP_THREADS], sm[BP_THREADS];
  const int t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * BP_SCAN_BLOCK;
  int32_t sum = 0, mx = 0;
#pragma unroll
  for (int e = 0; e < BP_SCAN_ITEMS; ++e) {
    const int64_t i = base + e * BP_THREADS + t;
    const int32_t v = i < n ? counts[i] : 0;
    sum += v;
    mx = max(mx, v);
  }
  ss[t] = sum; sm[t] = mx;
  __syncthreads();
  for (int d = BP_THREADS / 2; d > 0; d >>= 1) {
    if (t < d) { ss[t] += ss[t + d]; sm[t] = max(sm[t], sm[t + d]); }
    __syncthreads();
  }
  if (t == 0) { psum[blockIdx.x] = ss[0]; pmax[blockIdx.x] = sm[0]; }
}

// inclusive scan of one value per lane of a workgroup of N lanes (Hillis-Steele in LDS); returns the lane's prefix
template <int N>
__device__ __forceinline__ int32_t bp_block_scan(int32_t v, int32_t* s) {
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int d = 1; d < N; d <<= 1) {
    const int32_t u = t >= d ? s[t - d] : 0;
    __syncthreads();
    s[t] += u;
    __syncthreads();
  }
  return s[t];
}

// one workgroup: the block sums -> their exclusive prefix (in place), the maximum count, offsets[n] = the total
__global__ __launch_bounds__(1024) void bp_scan_top_k(int32_t* __restrict__ psum, const int32_t* __restrict__ pmax, int nb,
                                                      int32_t* __restrict__ offsets, int n,
                                                      pmf_bev_extent_t* __restrict__ ext) {
  __shared__ int32_t s[1024];
  const int t = threadIdx.x;
  int32_t carry = 0, mx = 0;
  for (int base = 0; base < nb; base += 1024) {
    const int i = base + t;
    const int32_t v = i < nb ? psum[i] : 0;
    if (i < nb) mx = max(mx, pmax[i]);
    const int32_t inc = bp_block_scan<1024>(v, s);
    if (i < nb) psum[i] = carry + inc - v;
    carry += s[1023];
    __syncthreads();
  }
  s[t] = mx;
  __syncthreads();
  for (int d = 512; d > 0; d >>= 1) {
    if (t < d) s[t] = max(s[t], s[t + d]);
    __syncthreads();
  }
  if (t == 0) {
    ext->max_count = s[0];
    offsets[n] = carry;
  }
}

__global__ __launch_bounds__(BP_THREADS) void bp_scan_apply_k(const int32_t* __restrict__ counts, int n,
                                                              const int32_t* __restrict__ psum,
                                                              int32_t* __restrict__ offsets) {
  __shared__ int32_t s[BP_THREADS];
  const int t = threadIdx.x;
  const int64_t first = (int64_t)blockIdx.x * BP_SCAN_BLOCK + (int64_t)t * BP_SCAN_ITEMS;
  int32_t v[BP_SCAN_ITEMS], sum = 0;
#pragma unroll
  for (int e = 0; e < BP_SCAN_ITEMS; ++e) {
    v[e] = first + e < n ? counts[first + e] : 0;
    sum += v[e];
  }
  int32_t run = psum[blockIdx.x] + bp_block_scan<BP_THREADS>(sum, s) - sum;
#pragma unroll
  for (int e = 0; e < BP_SCAN_ITEMS; ++e) {
    if (first + e < n) offsets[first + e] = run;
    run += v[e];
  }
}

// ---- place ---------------------------------------------------------------------------------------------------------------
// counts doubles as the cursor: it is counted down to zero (the cell pass takes a cell's count from the offsets)
__global__ __launch_bounds__(BP_THREADS) void bp_place_k(const int32_t* __restrict__ h_idx, const int32_t* __restrict__ w_idx,
                                                         int P, int h, int w, const int32_t* __restrict__ offsets,
                                                         int32_t* __restrict__ counts, int32_t* __restrict__ list,
                                                         pmf_bev_extent_t* __restrict__ ext) {
  for (int64_t i = (int64_t)blockIdx.x * BP_THREADS + threadIdx.x; i < P; i += (int64_t)gridDim.x * BP_THREADS) {
    const int32_t hi = h_idx[i], wi = w_idx[i];
    bool ok = hi >= 0 && hi < h && wi >= 0 && wi < w;
    int64_t slot = -1;
    if (ok) {
      const int64_t cell = (int64_t)hi * w + wi;
      slot = (int64_t)offsets[cell] + atomicSub(&counts[cell], 1) - 1;
      ok = slot >= offsets[cell] && slot < offsets[cell + 1] && slot < P;
    }
    if (ok) list[slot] = (int32_t)i;
    else atomicOr(&ext->flags, PMF_BEV_INTERNAL);
  }
}

// ---- cells ---------------------------------------------------------------------------------------------------------------
// the reference's running state of one cell; add() is its loop body for the next point of the cell in index order
struct BpCell {
  double zmax, zmin, sum;
  int32_t win;
  __device__ __forceinline__ void add(bool first, double v, int32_t id) {
    if (first || zmax < v) { zmax = v; win = id; }
    if (first || zmin > v) zmin = v;
    sum += v;
  }
};

__device__ __forceinline__ void bp_write(int64_t cell, int64_t ncells, int32_t n, const BpCell& c, int32_t win,
                                         const uint8_t* __restrict__ red, const uint8_t* __restrict__ green,
                                         const uint8_t* __restrict__ blue, const uint8_t* __restrict__ label,
                                         const double* __restrict__ log10_tab, int64_t tab_n,
                                         double* __restrict__ fmap, double* __restrict__ lmap) {
  double o[8] = {0, 0, 0, 0, 0, 0, 0, 0}, lab = -1.0;
  if (n > 0) {
    o[0] = c.zmax;
    o[1] = c.zmin;
    o[2] = c.sum / ((double)n + 1e-6);
    o[3] = n + 1 < tab_n ? log10_tab[n + 1] : NAN;     // (the entry point refuses a table that short)
    o[4] = 1.0;
    o[5] = (double)red[win];
    o[6] = (double)green[win];
    o[7] = (double)blue[win];
    lab = label ? (double)label[win] : 0.0;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) fmap[k * ncells + cell] = o[k];
  lmap[cell] = lab;
}

__global__ __launch_bounds__(BP_THREADS) void bp_cells_k(const float* __restrict__ z, const uint8_t* __restrict__ red,
                                                         const uint8_t* __restrict__ green, const uint8_t* __restrict__ blue,
                                                         const uint8_t* __restrict__ label, const int32_t* __restrict__ list,
                                                         const int32_t* __restrict__ offsets, int ncells,
                                                         const double* __restrict__ log10_tab, int64_t tab_n,
                                                         double* __restrict__ fmap, double* __restrict__ lmap,
                                                         int32_t* __restrict__ heavy,
                                                         int32_t* __restrict__ heavy_n, int heavy_cap) {
  const int64_t cell = (int64_t)blockIdx.x * BP_THREADS + threadIdx.x;
  if (cell >= ncells) return;
  const int32_t o = offsets[cell], n = offsets[cell + 1] - o;
  if (n > BP_LANE_MAX) {
    const int32_t k = atomicAdd(heavy_n, 1);
    if (k < heavy_cap) heavy[k] = (int32_t)cell;
    return;
  }
  BpCell c = {0.0, 0.0, 0.0, 0};
  int32_t prev = -1;
  for (int k = 0; k < n; ++k) {                 // the next larger point index of the cell
    int32_t cur = 2147483647;
    for (int j = 0; j < n; ++j) {
      const int32_t v = list[o + j];
      if (v > prev && v < cur) cur = v;
    }
    c.add(k == 0, (double)z[cur], cur);
    prev = cur;
  }
  bp_write(cell, ncells, n, c, c.win, red, green, blue, label, log10_tab, tab_n, fmap, lmap);
}

// workgroup per queued cell.  The network: for merge size k = 2, 4, ... the first step pairs i with its mirror in the
// block of k (i ^ (k - 1)), the following steps pair i with i ^ j, j = k/4 ... 1; every exchange puts the smaller value at
// the lower index, so positions >= n behave as +infinity that never moves and pairs reaching past n are simply skipped.
__global__ __launch_bounds__(BP_THREADS) void bp_heavy_k(const float* __restrict__ z, const uint8_t* __restrict__ red,
                                                         const uint8_t* __restrict__ green, const uint8_t* __restrict__ blue,
                                                         const uint8_t* __restrict__ label, int32_t* list,
                                                         const int32_t* __restrict__ offsets, int ncells,
                                                         const double* __restrict__ log10_tab, int64_t tab_n,
                                                         double* __restrict__ fmap, double* __restrict__ lmap,
                                                         const int32_t* __restrict__ heavy,
                                                         const int32_t* __restrict__ heavy_n, int heavy_cap) {
  __shared__ int32_t s_idx[BP_LDS_MAX];
  __shared__ double s_z[BP_CHUNK];
  const int t = threadIdx.x;
  const int nh = min(*heavy_n, heavy_cap);
  for (int q = blockIdx.x; q < nh; q += gridDim.x) {
    const int64_t cell = heavy[q];
    const int32_t o = offsets[cell], n = offsets[cell + 1] - o;
    int32_t* a = list + o;
    if (n <= BP_LDS_MAX) {
      for (int i = t; i < n; i += BP_THREADS) s_idx[i] = list[o + i];
      a = s_idx;
    }
    __syncthreads();
    for (int64_t k = 2; (k >> 1) < n; k <<= 1) {
      for (int64_t j = k - 1; j > 0; j = (j == k - 1) ? (k >> 2) : (j >> 1)) {
        for (int64_t i = t; i < n; i += BP_THREADS) {
          const int64_t l = i ^ j;
          if (l > i && l < n) {
            const int32_t u = a[i], v = a[l];
            if (u > v) { a[i] = v; a[l] = u; }
          }
        }
        __syncthreads();
      }
    }
    BpCell c = {0.0, 0.0, 0.0, 0};
    for (int base = 0; base < n; base += BP_CHUNK) {
      const int m = min(BP_CHUNK, n - base);
      for (int i = t; i < m; i += BP_THREADS) s_z[i] = (double)z[a[base + i]];
      __syncthreads();
      if (t == 0)
        for (int i = 0; i < m; ++i) c.add(base + i == 0, s_z[i], base + i);
      __syncthreads();
    }
    if (t == 0) bp_write(cell, ncells, n, c, a[c.win], red, green, blue, label, log10_tab, tab_n, fmap, lmap);
    __syncthreads();                            // s_idx is reused by the next cell
  }
}

// ---- entry points --------------------------------------------------------------------------------------------------------
static inline bool bp_grid_ok(double grid) { return grid > 0.0 && grid <= 1.7976931348623157e308 && (float)grid > 0.f; }
static inline int bp_blocks(int64_t P) { return (int)(cdiv64(P, BP_THREADS) < BP_GRID ? cdiv64(P, BP_THREADS) : BP_GRID); }

extern "C" int64_t pmf_bev_prepare_workspace(int64_t P, int64_t h, int64_t w) {
  if (h == 0 && w == 0) return P >= 1 && P < 2147483647LL ? bp_layout(P, 0).total : PMF_E_ARG;
  if (!bp_sizes_ok(P, h, w)) return PMF_E_ARG;
  return bp_layout(P, h * w).total;
}

extern "C" int pmf_bev_prepare_extent(const float* x, const float* y, const float* z, int64_t P, double grid, int32_t f64,
                                      void* workspace, pmf_bev_extent_t* ext, pmf_stream_t s) {
  if (!x || !y || !z || !workspace || !ext || P < 1 || P >= 2147483647LL || !bp_grid_ok(grid) || (f64 != 0 && f64 != 1))
    return PMF_E_ARG;
  hipStream_t st = (hipStream_t)s;
  float* part = (float*)((char*)workspace + bp_layout(P, 0).part);
  const int nb = bp_blocks(P);
  hipError_t e = hipMemsetAsync(ext, 0, sizeof(pmf_bev_extent_t), st);
  if (e != hipSuccess) return (int)e;
  bp_extent_k<<<nb, BP_THREADS, 0, st>>>(x, y, z, (int)P, part, ext);
  PMF_LAUNCH_CHECK();
  if (f64) bp_extent_final_k<true><<<1, BP_THREADS, 0, st>>>(part, nb, grid, (float)grid, ext);
  else bp_extent_final_k<false><<<1, BP_THREADS, 0, st>>>(part, nb, grid, (float)grid, ext);
  PMF_LAUNCH_CHECK();
  return 0;
}

extern "C" int pmf_bev_prepare_bin(const float* x, const float* y, int64_t P, double grid, int32_t f64,
                                   pmf_bev_extent_t* ext, int32_t h, int32_t w, void* workspace, int32_t* h_idx,
                                   int32_t* w_idx, pmf_stream_t s) {
  if (!x || !y || !ext || !workspace || !h_idx || !w_idx || !bp_sizes_ok(P, h, w) || !bp_grid_ok(grid) ||
      (f64 != 0 && f64 != 1))
    return PMF_E_ARG;
  hipStream_t st = (hipStream_t)s;
  const int64_t ncells = (int64_t)h * w;
  const BpLayout l = bp_layout(P, ncells);
  int32_t* counts = (int32_t*)((char*)workspace + l.counts);
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)ncells * 4, st);
  if (e != hipSuccess) return (int)e;
  if (f64) bp_bin_k<true><<<bp_blocks(P), BP_THREADS, 0, st>>>(x, y, (int)P, grid, (float)grid, ext, h, w, h_idx, w_idx, counts);
  else bp_bin_k<false><<<bp_blocks(P), BP_THREADS, 0, st>>>(x, y, (int)P, grid, (float)grid, ext, h, w, h_idx, w_idx, counts);
  PMF_LAUNCH_CHECK();
  return 0;
}

extern "C" int pmf_bev_prepare_scan(int64_t P, int32_t h, int32_t w, void* workspace, pmf_bev_extent_t* ext,
                                    pmf_stream_t s) {
  if (!workspace || !ext || !bp_sizes_ok(P, h, w)) return PMF_E_ARG;
  hipStream_t st = (hipStream_t)s;
  const int64_t ncells = (int64_t)h * w;
  const BpLayout l = bp_layout(P, ncells);
  char* ws = (char*)workspace;
  int32_t *counts = (int32_t*)(ws + l.counts), *offsets = (int32_t*)(ws + l.offsets);
  int32_t *psum = (int32_t*)(ws + l.psum), *pmax = (int32_t*)(ws + l.pmax);
  const int nb = (int)cdiv64(ncells, BP_SCAN_BLOCK);
  bp_scan_part_k<<<nb, BP_THREADS, 0, st>>>(counts, (int)ncells, psum, pmax);
  PMF_LAUNCH_CHECK();
  bp_scan_top_k<<<1, 1024, 0, st>>>(psum, pmax, nb, offsets, (int)ncells, ext);
  PMF_LAUNCH_CHECK();
  bp_scan_apply_k<<<nb, BP_THREADS, 0, st>>>(counts, (int)ncells, psum, offsets);
  PMF_LAUNCH_CHECK();
  return 0;
}

extern "C" int pmf_bev_prepare_place(const int32_t* h_idx, const int32_t* w_idx, int64_t P, int32_t h, int32_t w,
                                     void* workspace, pmf_bev_extent_t* ext, pmf_stream_t s) {
  if (!h_idx || !w_idx || !workspace || !ext || !bp_sizes_ok(P, h, w)) return PMF_E_ARG;
  hipStream_t st = (hipStream_t)s;
  const BpLayout l = bp_layout(P, (int64_t)h * w);
  char* ws = (char*)workspace;
  bp_place_k<<<bp_blocks(P), BP_THREADS, 0, st>>>(h_idx, w_idx, (int)P, h, w, (const int32_t*)(ws + l.offsets),
                                                  (int32_t*)(ws + l.counts), (int32_t*)(ws + l.list), ext);
  PMF_LAUNCH_CHECK();
  return 0;
}

extern "C" int pmf_bev_prepare_cells(const float* z, const uint8_t* red, const uint8_t* green, const uint8_t* blue,
                                     const uint8_t* label, int64_t P, int32_t h, int32_t w, void* workspace,
                                     const double* log10_tab, int64_t tab_n, int64_t max_count, double* feature_map,
                                     double* label_map, pmf_stream_t s) {
  if (!z || !red || !green || !blue || !workspace || !log10_tab || !feature_map || !label_map || !bp_sizes_ok(P, h, w) ||
      max_count < 1 || max_count > P || tab_n < max_count + 2)
    return PMF_E_ARG;
  hipStream_t st = (hipStream_t)s;
  const int64_t ncells = (int64_t)h * w;
  const BpLayout l = bp_layout(P, ncells);
  char* ws = (char*)workspace;
  int32_t *list = (int32_t*)(ws + l.list), *offsets = (int32_t*)(ws + l.offsets);
  int32_t *heavy = (int32_t*)(ws + l.heavy), *heavy_n = (int32_t*)(ws + l.heavy_n);
  const int heavy_cap = (int)(P / (BP_LANE_MAX + 1) + 1);
  hipError_t e = hipMemsetAsync(heavy_n, 0, 4, st);
  if (e != hipSuccess) return (int)e;
  bp_cells_k<<<(unsigned)cdiv64(ncells, BP_THREADS), BP_THREADS, 0, st>>>(z, red, green, blue, label, list, offsets,
                                                                           (int)ncells, log10_tab, tab_n, feature_map,
                                                                           label_map,                                                                            heavy, heavy_n, heavy_cap);
  PMF_LAUNCH_CHECK();
  if (max_count > BP_LANE_MAX) {
    bp_heavy_k<<<BP_GRID, BP_THREADS, 0, st>>>(z, red, green, blue, label, list, offsets, (int)ncells, log10_tab, tab_n,
                                               feature_map, label_map, heavy, heavy_n, heavy_cap);
    PMF_LAUNCH_CHECK();
  }
  return 0;
}
