// Camera undistortion of the A2D2 loader (include/pmf_amd_a2d2.h): the per-camera map and the per-frame fixed-point remap.
// Follows OpenCV's published algorithm (initUndistortRectifyMap / fisheye::initUndistortRectifyMap, remap INTER_LINEAR with
// BORDER_CONSTANT 0 on 5 fractional bits); see the header for the arithmetic and the one known deviation.
#include "common.h"
#include "../../include/pmf_amd_a2d2.h"

struct UndistArgs {
  double ir[9];
  double fx, fy, cx, cy;
  double d[5];
};

// rint (half to even) saturated to int32; NaN -> INT32_MIN
__device__ __forceinline__ int32_t ud_fix(double t) {
  const double r = rint(t);
  if (!(r > -2147483648.0)) return -2147483647 - 1;
  if (r >= 2147483647.0) return 2147483647;
  return (int32_t)r;
}

template <int LENS>
__global__ __launch_bounds__(256) void undist_map_k(const UndistArgs A, int w, int64_t n, int32_t* __restrict__ map) {
  const int64_t p = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (p >= n) return;
  const int i = (int)(p / w), j = (int)(p - (int64_t)i * w);
  const double dj = (double)j, di = (double)i;
  double x = A.ir[0] * dj + A.ir[1] * di + A.ir[2];
  double y = A.ir[3] * dj + A.ir[4] * di + A.ir[5];
  const double ww = A.ir[6] * dj + A.ir[7] * di + A.ir[8];
  x /= ww; y /= ww;
  double xd, yd;
  if (LENS == PMF_LENS_TELECAM) {
    const double k1 = A.d[0], k2 = A.d[1], p1 = A.d[2], p2 = A.d[3], k3 = A.d[4];
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = 2.0 * x * y;
    const double kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
    xd = x * kr + p1 * xy2 + p2 * (r2 + 2.0 * x2);
    yd = y * kr + p1 * (r2 + 2.0 * y2) + p2 * xy2;
  } else {
    const double r = sqrt(x * x + y * y), t = atan(r), t2 = t * t;
    const double t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
    const double td = t * (1.0 + A.d[0] * t2 + A.d[1] * t4 + A.d[2] * t6 + A.d[3] * t8);
    const double sc = r == 0.0 ? 1.0 : td / r;
    xd = x * sc; yd = y * sc;
  }
  const double u = A.fx * xd + A.cx, v = A.fy * yd + A.cy;
  int2 o;
  o.x = ud_fix(u * 32.0); o.y = ud_fix(v * 32.0);
  *(int2*)(map + 2 * p) = o;
}

extern "C" int pmf_undistort_map(int32_t lens, const double* ir_host, double fx, double fy, double cx, double cy,
                                 const double* dist_host, int32_t h, int32_t w, int32_t* map, pmf_stream_t s) {
  if (!ir_host || !dist_host || !map || h < 1 || w < 1) return PMF_E_ARG;
  if (lens != PMF_LENS_TELECAM && lens != PMF_LENS_FISHEYE) return PMF_E_ARG;
  const int64_t n = (int64_t)h * w;
  if (n > 2147483647ll) return PMF_E_UNSUPPORTED;
  UndistArgs A;
  for (int k = 0; k < 9; ++k) A.ir[k] = ir_host[k];
  for (int k = 0; k < 5; ++k) A.d[k] = dist_host[k];
  A.fx = fx; A.fy = fy; A.cx = cx; A.cy = cy;
  const dim3 grid((unsigned)cdiv64(n, 256));
  if (lens == PMF_LENS_TELECAM)
    hipLaunchKernelGGL(undist_map_k<PMF_LENS_TELECAM>, grid, dim3(256), 0, (hipStream_t)s, A, w, n, map);
  else
    hipLaunchKernelGGL(undist_map_k<PMF_LENS_FISHEYE>, grid, dim3(256), 0, (hipStream_t)s, A, w, n, map);
  PMF_LAUNCH_CHECK();
  return 0;
}

// ---- remap ------------------------------------------------------------------------------------------------------------
// dst and map are dense, so the destination is a flat run of n = h * w pixels and the image width plays no part: a lane
// takes RG = 4 consecutive pixels = 32 bytes of map (two 16-byte loads) and 12 bytes of output (three whole dwords, every
// group starts on a dword since dst does).  The n % 4 pixels of the last group are stored byte by byte.  The gathered source
// bytes are shared by neighbouring lanes and come through the caches; every source read is inside [0,sh) x [0,sw).
#define RG 4

struct Rgb3 { uint32_t r, g, b; };

__device__ __forceinline__ Rgb3 rm_px(const uint8_t* __restrict__ src, int sh, int sw, int sy, int sx) {
  Rgb3 o = {0u, 0u, 0u};
  if ((unsigned)sy < (unsigned)sh && (unsigned)sx < (unsigned)sw) {
    const uint8_t* q = src + ((size_t)sy * sw + sx) * 3;
    o.r = q[0]; o.g = q[1]; o.b = q[2];
  }
  return o;
}

// one destination pixel -> its three bytes in bits 0..23
__device__ __forceinline__ uint32_t rm_one(const uint8_t* __restrict__ src, int sh, int sw, int iu, int iv) {
  const int sx = iu >> 5, sy = iv >> 5;
  const uint32_t a = (uint32_t)(iu & 31), b = (uint32_t)(iv & 31);
  const uint32_t w00 = (32u - b) * (32u - a), w01 = (32u - b) * a, w10 = b * (32u - a), w11 = b * a;
  const Rgb3 p00 = rm_px(src, sh, sw, sy, sx), p01 = rm_px(src, sh, sw, sy, sx + 1);
  const Rgb3 p10 = rm_px(src, sh, sw, sy + 1, sx), p11 = rm_px(src, sh, sw, sy + 1, sx + 1);
  const uint32_t r = (p00.r * w00 + p01.r * w01 + p10.r * w10 + p11.r * w11 + 512u) >> 10;
  const uint32_t g = (p00.g * w00 + p01.g * w01 + p10.g * w10 + p11.g * w11 + 512u) >> 10;
  const uint32_t bl = (p00.b * w00 + p01.b * w01 + p10.b * w10 + p11.b * w11 + 512u) >> 10;
  return r | (g << 8) | (bl << 16);
}

__global__ __launch_bounds__(256) void remap_u8c3_k(const uint8_t* __restrict__ src, int sh, int sw,
                                                    const int32_t* __restrict__ map, int64_t n, uint8_t* __restrict__ dst) {
  const int64_t g = blockIdx.x * (int64_t)256 + threadIdx.x;
  const int64_t p0 = g * RG;
  if (p0 >= n) return;
  if (p0 + RG <= n) {
    const int4 m0 = *(const int4*)(map + 2 * p0), m1 = *(const int4*)(map + 2 * p0 + 4);
    const uint32_t c0 = rm_one(src, sh, sw, m0.x, m0.y), c1 = rm_one(src, sh, sw, m0.z, m0.w);
    const uint32_t c2 = rm_one(src, sh, sw, m1.x, m1.y), c3 = rm_one(src, sh, sw, m1.z, m1.w);
    uint32_t* o = (uint32_t*)(dst + 3 * p0);
    o[0] = c0 | (c1 << 24);
    o[1] = (c1 >> 8) | (c2 << 16);
    o[2] = (c2 >> 16) | (c3 << 8);
  } else {
    for (int64_t p = p0; p < n; ++p) {
      const uint32_t c = rm_one(src, sh, sw, map[2 * p], map[2 * p + 1]);
      dst[3 * p] = (uint8_t)c; dst[3 * p + 1] = (uint8_t)(c >> 8); dst[3 * p + 2] = (uint8_t)(c >> 16);
    }
  }
}

extern "C" int pmf_remap_u8c3(const uint8_t* src, int32_t sh, int32_t sw, const int32_t* map, int32_t h, int32_t w,
                              uint8_t* dst, pmf_stream_t s) {
  if (!src || !map || !dst || sh < 1 || sw < 1 || h < 1 || w < 1) return PMF_E_ARG;
  const int64_t n = (int64_t)h * w;
  if (n > 2147483647ll || (int64_t)sh * sw > 2147483647ll) return PMF_E_UNSUPPORTED;
  // the vector path needs map on 16 bytes and dst on 4: device allocations are; a caller's offset view is refused
  if (((uintptr_t)map & 15) || ((uintptr_t)dst & 3)) return PMF_E_ARG;
  const int64_t groups = cdiv64(n, RG);
  hipLaunchKernelGGL(remap_u8c3_k, dim3((unsigned)cdiv64(groups, 256)), dim3(256), 0, (hipStream_t)s, src, sh, sw, map, n,
                     dst);
  PMF_LAUNCH_CHECK();
  return 0;
}
