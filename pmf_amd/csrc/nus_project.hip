// The nuScenes projection chain (include/pmf_amd_nus.h): lidar -> ego -> global -> ego at image time -> camera, pinhole,
// keep mask, order-preserving crop and bounding box of one camera view, as count / scan / compact on the caller's stream
// (the scheme of pmf_project_v2_index, project.hip).  The frame itself is then written by pmf_project_v2_scatter.
#include "common.h"
#include "../../include/pmf_amd_nus.h"

// The outputs are compared bit for bit with element-wise numpy float64 arithmetic: every product and sum of the header's
// formula stays one operation under a file-wide contract(off), as in a2d2.hip.
#pragma clang fp contract(off)

#define NB PMF_NUS_BLOCK

// chain_host by value: R1 0, t1 9, R2 12, t2 21, t3 24, R3 27, t4 36, R4 39, K 48
struct NusChain { double v[PMF_NUS_CHAIN]; };

struct NusArgs {
  int mode, stride;
  float min_dist, fov_lo, fov_hi;
  double bound_h, bound_w, row_scale, col_scale, img_scale;
};

__device__ __forceinline__ void nus_rot(const double* __restrict__ R, float& x, float& y, float& z) {
  const double px = (double)x, py = (double)y, pz = (double)z;
  x = (float)((R[0] * px + R[1] * py) + R[2] * pz);
  y = (float)((R[3] * px + R[4] * py) + R[5] * pz);
  z = (float)((R[6] * px + R[7] * py) + R[8] * pz);
}

__device__ __forceinline__ void nus_tr(const double* __restrict__ t, float& x, float& y, float& z) {
  x = (float)((double)x + t[0]);
  y = (float)((double)y + t[1]);
  z = (float)((double)z + t[2]);
}

// one point: camera-frame (x, y, z), scaled (row, col) and depth; returns the keep bit
__device__ __forceinline__ bool nus_point(const float* __restrict__ pt, const NusChain& ch, const NusArgs& a, float& x,
                                          float& y, float& z, double& fr, double& fc, float& dep) {
  const double* c = ch.v;
  const float lx = pt[0], ly = pt[1], lz = pt[2];
  x = lx; y = ly; z = lz;
  nus_rot(c + 0, x, y, z);  nus_tr(c + 9, x, y, z);
  nus_rot(c + 12, x, y, z); nus_tr(c + 21, x, y, z);
  nus_tr(c + 24, x, y, z);  nus_rot(c + 27, x, y, z);
  nus_tr(c + 36, x, y, z);  nus_rot(c + 39, x, y, z);
  const double dx = (double)x, dy = (double)y, dz = (double)z;
  const double* K = c + 48;
  const double pa = (K[0] * dx + K[1] * dy) + K[2] * dz;
  const double pb = (K[3] * dx + K[4] * dy) + K[5] * dz;
  const double pc = (K[6] * dx + K[7] * dy) + K[8] * dz;
  const double u = pa / pc, v = pb / pc;
  fr = (v * a.row_scale) * a.img_scale;
  fc = (u * a.col_scale) * a.img_scale;
  if (!(z > a.min_dist)) return false;
  if (a.mode == PMF_NUS_YAW) {
    dep = sqrtf((x * x + y * y) + z * z);
    const float yaw = -atan2f(z, x);
    return (double)yaw >= (double)a.fov_lo && (double)yaw <= (double)a.fov_hi;
  }
  dep = sqrtf((lx * lx + ly * ly) + lz * lz);
  return u > 1.0 && u < a.bound_h - 1.0 && v > 1.0 && v < a.bound_w - 1.0;
}

__global__ __launch_bounds__(NB) void nus_count_k(const float* __restrict__ pts, int P, const NusChain ch, const NusArgs a,
                                                  uint8_t* __restrict__ keep, int32_t* __restrict__ blk_cnt) {
  const int64_t i = blockIdx.x * (int64_t)NB + threadIdx.x;
  int k = 0;
  if (i < P) {
    float x, y, z, d; double fr, fc;
    k = nus_point(pts + (size_t)i * a.stride, ch, a, x, y, z, fr, fc, d) ? 1 : 0;
    keep[i] = (uint8_t)k;
  }
  const int cnt = __syncthreads_count(k);
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = cnt;
}

// exclusive scan of the nblk workgroup counts in place; meta[0] = K and, when K > 0, the bounding box's starting values
__global__ __launch_bounds__(NB) void nus_scan_k(int32_t* __restrict__ blk_cnt, int nblk, int32_t* __restrict__ meta) {
  __shared__ int sh[NB];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < nblk; base += NB) {
    const int i = base + threadIdx.x;
    const int v = i < nblk ? blk_cnt[i] : 0;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < NB; off <<= 1) {
      const int t = (int)threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
      __syncthreads();
      sh[threadIdx.x] += t;
      __syncthreads();
    }
    if (i < nblk) blk_cnt[i] = carry + sh[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == NB - 1) carry += sh[NB - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    meta[0] = carry;
    if (carry > 0) {
      meta[1] = 2147483647; meta[2] = -2147483647 - 1; meta[3] = 2147483647; meta[4] = -2147483647 - 1;
    }
  }
}

__global__ __launch_bounds__(NB) void nus_compact_k(const float* __restrict__ pts, int P, const NusChain ch, const NusArgs a,
                                                    const int32_t* __restrict__ blk_off, int32_t* __restrict__ src_idx,
                                                    float* __restrict__ crop, double* __restrict__ xy,
                                                    int32_t* __restrict__ x_data, int32_t* __restrict__ y_data,
                                                    float* __restrict__ depth, int32_t* __restrict__ meta) {
  __shared__ int wave_cnt[NB / 64];
  const int64_t i = blockIdx.x * (int64_t)NB + threadIdx.x;
  float x = 0.f, y = 0.f, z = 0.f, d = 0.f; double fr = 0.0, fc = 0.0;
  const float* pt = pts + (size_t)(i < P ? i : 0) * a.stride;
  const bool k = i < P && nus_point(pt, ch, a, x, y, z, fr, fc, d);
  const unsigned long long bal = __ballot(k);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int before = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) wave_cnt[wv] = __popcll(bal);
  __syncthreads();
  int woff = 0;
  for (int j = 0; j < wv; ++j) woff += wave_cnt[j];
  if (k) {
    const size_t dst = (size_t)(blk_off[blockIdx.x] + woff + before);      // < K <= P
    const int r = (int)fr, c = (int)fc;
    src_idx[dst] = (int)i;
    crop[4 * dst] = x; crop[4 * dst + 1] = y; crop[4 * dst + 2] = z; crop[4 * dst + 3] = pt[3];
    xy[2 * dst] = fr; xy[2 * dst + 1] = fc;
    x_data[dst] = r; y_data[dst] = c;
    depth[dst] = d;
    atomicMin(meta + 1, r); atomicMax(meta + 2, r); atomicMin(meta + 3, c); atomicMax(meta + 4, c);
  }
}

static inline bool nus_scale_ok(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }

extern "C" int pmf_nus_project(const float* points, int32_t P, int32_t stride, const double* chain_host, int32_t mode,
                               double min_dist, float fov_lo, float fov_hi, double bound_h, double bound_w,
                               double row_scale, double col_scale, double img_scale, uint8_t* keep, int32_t* src_idx,
                               float* crop, double* xy, int32_t* x_data, int32_t* y_data, float* depth, int32_t* meta,
                               int32_t* blk_cnt, pmf_stream_t s) {
  if (!points || !chain_host || !keep || !src_idx || !crop || !xy || !x_data || !y_data || !depth || !meta || !blk_cnt)
    return PMF_E_ARG;
  if (P < 1 || (stride != 4 && stride != 5) || (mode != PMF_NUS_IMAGE && mode != PMF_NUS_YAW)) return PMF_E_ARG;
  if (!nus_scale_ok(row_scale) || !nus_scale_ok(col_scale) || !nus_scale_ok(img_scale)) return PMF_E_ARG;
  NusChain ch;
  for (int j = 0; j < PMF_NUS_CHAIN; ++j) ch.v[j] = chain_host[j];
  NusArgs a;
  a.mode = mode; a.stride = stride;
  a.min_dist = (float)min_dist; a.fov_lo = fov_lo; a.fov_hi = fov_hi;
  a.bound_h = bound_h; a.bound_w = bound_w; a.row_scale = row_scale; a.col_scale = col_scale; a.img_scale = img_scale;
  hipStream_t st = (hipStream_t)s;
  const int nblk = (int)cdiv64(P, NB);
  hipLaunchKernelGGL(nus_count_k, dim3(nblk), dim3(NB), 0, st, points, P, ch, a, keep, blk_cnt);
  hipLaunchKernelGGL(nus_scan_k, dim3(1), dim3(NB), 0, st, blk_cnt, nblk, meta);
  hipLaunchKernelGGL(nus_compact_k, dim3(nblk), dim3(NB), 0, st, points, P, ch, a, blk_cnt, src_idx, crop, xy, x_data,
                     y_data, depth, meta);
  PMF_LAUNCH_CHECK();
  return 0;
}
