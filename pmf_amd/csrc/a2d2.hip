// Per-point pass of the A2D2 loader (include/pmf_amd_a2d2.h): float32 point rows, float64 depth rounded once, scaled pixel
// coordinates with their truncation and bounding box, and the colour -> class lookup of the label image
// (dataset_a2d2.py:244-254 as a table search).  The frame itself is then written by pmf_project_v2_scatter (project.hip).
#include "common.h"
#include "../../include/pmf_amd_a2d2.h"

// The outputs are compared bit for bit with numpy's float64.  __dmul_rn / __dadd_rn are a plain `*` / `+` inside this
// toolchain's headers, compiled under the default contraction, and come out as v_fmac_f64 once inlined; so the products and
// sums below are written out under a file-wide contract(off), which does keep them apart (checked in the ISA: five
// v_mul_f64, two v_add_f64, fused operations only inside the correctly rounded square root).
#pragma clang fp contract(off)

#define A2_PB 256
#define A2_MAXKEYS 64

__global__ __launch_bounds__(A2_PB) void a2d2_index_k(const double* __restrict__ points, const double* __restrict__ refl,
                                                      const int32_t* __restrict__ rows, const int32_t* __restrict__ cols,
                                                      const uint8_t* __restrict__ rgb, int P,
                                                      const uint32_t* __restrict__ keys, const int32_t* __restrict__ cls,
                                                      int n, double sc, float* __restrict__ pts,
                                                      float* __restrict__ depth, double* __restrict__ xy,
                                                      int32_t* __restrict__ x_data, int32_t* __restrict__ y_data,
                                                      int32_t* __restrict__ sem, int32_t* __restrict__ meta) {
  __shared__ uint32_t s_key[A2_MAXKEYS];
  __shared__ int32_t s_cls[A2_MAXKEYS];
  if (rgb && (int)threadIdx.x < n) {
    s_key[threadIdx.x] = keys[threadIdx.x];
    s_cls[threadIdx.x] = cls[threadIdx.x];
  }
  __syncthreads();
  const int i = blockIdx.x * A2_PB + threadIdx.x;
  if (i >= P) return;
  const double x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
  f32x4 q;
  q.x = (float)x; q.y = (float)y; q.z = (float)z; q.w = (float)refl[i];
  *(f32x4*)(pts + 4 * (size_t)i) = q;
  const double xx = x * x, yy = y * y, zz = z * z;
  depth[i] = (float)__dsqrt_rn((xx + yy) + zz);
  const double fr = (double)rows[i] * sc, fc = (double)cols[i] * sc;
  xy[2 * (size_t)i] = fr; xy[2 * (size_t)i + 1] = fc;
  const int r = (int)fr, c = (int)fc;
  x_data[i] = r; y_data[i] = c;
  atomicMin(meta + 0, r); atomicMax(meta + 1, r); atomicMin(meta + 2, c); atomicMax(meta + 3, c);
  int label = 0;
  if (rgb) {
    const uint8_t* px = rgb + 3 * (size_t)i;
    const uint32_t key = ((uint32_t)px[0] << 16) | ((uint32_t)px[1] << 8) | (uint32_t)px[2];
    int hit = -1;
    for (int k = 0; k < n; ++k)
      if (s_key[k] == key) { hit = k; break; }
    if (hit >= 0) {
      label = s_cls[hit];
    } else {
      atomicAdd(meta + 4, 1);
      atomicMin(meta + 5, i);
    }
  }
  sem[i] = label;
}

extern "C" int pmf_a2d2_index(const double* points, const double* reflectance, const int32_t* rows, const int32_t* cols,
                              const uint8_t* rgb, int32_t P, const uint32_t* keys, const int32_t* cls, int32_t n,
                              double img_scale, float* pts, float* depth, double* xy, int32_t* x_data, int32_t* y_data,
                              int32_t* sem, int32_t* meta, pmf_stream_t s) {
  if (!points || !reflectance || !rows || !cols || !pts || !depth || !xy || !x_data || !y_data || !sem || !meta)
    return PMF_E_ARG;
  if (P < 1 || !(img_scale > 0.0) || !(img_scale <= 1.7976931348623157e308)) return PMF_E_ARG;
  if (rgb && (!keys || !cls || n < 1 || n > A2_MAXKEYS)) return PMF_E_ARG;
  if ((uintptr_t)pts & 15) return PMF_E_ARG;      // one 16-byte store per point
  hipStream_t st = (hipStream_t)s;
  static const int32_t init[6] = {2147483647, -2147483647 - 1, 2147483647, -2147483647 - 1, 0, 2147483647};
  hipError_t e = hipMemcpyAsync(meta, init, sizeof(init), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(a2d2_index_k, dim3(cdiv(P, A2_PB)), dim3(A2_PB), 0, st, points, reflectance, rows, cols, rgb, P, keys,
                     cls, rgb ? n : 0, img_scale, pts, depth, xy, x_data, y_data, sem, meta);
  PMF_LAUNCH_CHECK();
  return 0;
}
