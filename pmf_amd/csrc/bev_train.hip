// SensatUrban training loader on the device (pc_processor/dataset/sensat_urban/sensat_loader.py:17-27,57-73 of the reference).
// Per item the reference converts the whole float64 frame to float32 on the host, concatenates the label plane and runs
//   RandomCrop(2H,2W) -> RandomRotation(360) -> RandomCrop(H,W) -> RandomHorizontalFlip -> RandomVerticalFlip
// over nine planes until at least 10 % of the label plane is >= 0, then applies two scalar jitters.  The chain is one map
// from an output pixel to one frame pixel or to zero, so here the frames are converted once and stay on the device:
//   pmf_bev_sample_count    n candidate draws -> int32[n] output pixels with label >= 0 (label planes only)
//   pmf_bev_sample_gather   B accepted draws  -> f32[B,8,H,W] features (jittered) + f32[B,H,W] labels, one launch
// Resident layout: features pixel-major f32[h][w][8] -- a gathered pixel is 32 aligned bytes, two 16-byte loads, where eight
// planes would cost eight cache lines -- and the label as a separate int8[h][w] plane, which is all the count reads.
// Coordinates follow aug_gather_k (project.hip), i.e. torchvision's tensor rotation in float32, with w := 2W, h := 2H.
// A workgroup covers a 32 x 8 tile of output pixels: its source footprint is a rotated 32 x 8 rectangle at any angle, a
// few cache lines of the pixel-major frame, and every plane row it writes is one 128-byte segment along ox.
// Plain C++ and vector stores only; the one atomic is an integer add per workgroup into the count.
#include "common.h"
#include "../../include/pmf_amd_sensat.h"
#pragma clang fp contract(off)

#define BT_TX 32
#define BT_TY 8
#define BT_COUNT_WG 256     // workgroups per candidate of the count

// output pixel (cy, cx) of the second crop -> pixel (fy, fx) of the frame; false: zero fill (outside the rotated first crop,
// or -- for a struct the host did not validate -- outside the frame)
__device__ __forceinline__ bool bt_source(const pmf_bev_sample_t& sm, int H, int W, int cy, int cx, int64_t* fy, int64_t* fx) {
  const float w = 2.f * (float)W, h = 2.f * (float)H;
  const float xg = (float)((int64_t)sm.left2 + cx) - 0.5f * w + 0.5f, yg = (float)((int64_t)sm.top2 + cy) - 0.5f * h + 0.5f;
  const float gx = fmaf(yg, sm.m1 / (0.5f * w), xg * (sm.m0 / (0.5f * w)));
  const float gy = fmaf(yg, sm.m4 / (0.5f * h), xg * (sm.m3 / (0.5f * h)));
  const float ix = ((gx + 1.f) * w - 1.f) / 2.f, iy = ((gy + 1.f) * h - 1.f) / 2.f;
  const float rx = rintf(ix), ry = rintf(iy);
  if (!(rx >= 0.f && rx <= w - 1.f && ry >= 0.f && ry <= h - 1.f)) return false;       // (a NaN matrix lands here too)
  *fx = (int64_t)sm.left1 + (int64_t)rx;
  *fy = (int64_t)sm.top1 + (int64_t)ry;
  return *fx >= 0 && *fx < sm.w && *fy >= 0 && *fy < sm.h;
}

// A workgroup walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ... of its candidate: the atomics of one candidate all
// land on one address, so there are at most BT_COUNT_WG of them (one per tile took longer than the whole gather).
__global__ __launch_bounds__(BT_TX* BT_TY) void bev_sample_count_k(const pmf_bev_sample_t* __restrict__ samples, int H,
                                                                    int W, int tiles_x, int tiles, int* __restrict__ counts) {
  __shared__ int part[BT_TX * BT_TY / 64];
  const pmf_bev_sample_t sm = samples[blockIdx.y];
  int mine = 0;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int cx = (tile % tiles_x) * BT_TX + (threadIdx.x & (BT_TX - 1));
    const int cy = (tile / tiles_x) * BT_TY + (threadIdx.x / BT_TX);
    if (cx < W && cy < H) {
      int64_t fy, fx;
      mine += !bt_source(sm, H, W, cy, cx, &fy, &fx) || sm.label[fy * sm.w + fx] >= 0;       // the zero fill is >= 0
    }
  }
  int wave_sum = mine;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) wave_sum += __shfl_down(wave_sum, d, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = wave_sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int k = 0; k < BT_TX * BT_TY / 64; ++k) t += part[k];
    if (t) atomicAdd(&counts[blockIdx.y], t);
  }
}

__global__ __launch_bounds__(BT_TX* BT_TY) void bev_sample_gather_k(const pmf_bev_sample_t* __restrict__ samples, int H,
                                                                     int W, int tiles_x, float* __restrict__ feature_out,
                                                                     float* __restrict__ label_out) {
  const pmf_bev_sample_t sm = samples[blockIdx.y];
  const int ox = (int)(blockIdx.x % tiles_x) * BT_TX + (threadIdx.x & (BT_TX - 1));
  const int oy = (int)(blockIdx.x / tiles_x) * BT_TY + (threadIdx.x / BT_TX);
  if (ox >= W || oy >= H) return;
  const int cx = (sm.flags & PMF_BEV_HFLIP) ? W - 1 - ox : ox, cy = (sm.flags & PMF_BEV_VFLIP) ? H - 1 - oy : oy;
  float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
  float lab = 0.f;
  int64_t fy, fx;
  if (bt_source(sm, H, W, cy, cx, &fy, &fx)) {
    const int64_t p = fy * sm.w + fx;
    const float4* __restrict__ px = reinterpret_cast<const float4*>(sm.feat) + 2 * p;
    lo = px[0];
    hi = px[1];
    lab = (float)sm.label[p];
  }
  const float m = hi.x;                                          // channel 4: the occupancy mask
  const int64_t HW = (int64_t)H * W, at = (int64_t)oy * W + ox;
  float* __restrict__ f = feature_out + (int64_t)blockIdx.y * 8 * HW + at;
  // sensat_loader.py:70-71 in float32: an add, then a multiply (contraction is off)
  f[0 * HW] = (lo.x + sm.jit_h) * m;
  f[1 * HW] = (lo.y + sm.jit_h) * m;
  f[2 * HW] = (lo.z + sm.jit_h) * m;
  f[3 * HW] = lo.w;
  f[4 * HW] = m;
  f[5 * HW] = (hi.y + sm.jit_rgb) * m;
  f[6 * HW] = (hi.z + sm.jit_rgb) * m;
  f[7 * HW] = (hi.w + sm.jit_rgb) * m;
  label_out[(int64_t)blockIdx.y * HW + at] = lab;
}

// tiles of one sample, or 0 when H x W is out of range
static int64_t bt_tiles(int32_t H, int32_t W, int* tiles_x) {
  if (H <= 0 || W <= 0 || (int64_t)H * W > (int64_t)INT32_MAX) return 0;
  *tiles_x = cdiv(W, BT_TX);
  return (int64_t)*tiles_x * cdiv(H, BT_TY);              // <= H * W: fits the x dimension of a grid
}

extern "C" int pmf_sizeof_sensat(void) { return (int)sizeof(pmf_bev_sample_t); }

extern "C" int pmf_bev_sample_count(const pmf_bev_sample_t* samples_dev, int32_t n, int32_t H, int32_t W,
                                    int32_t* counts_dev, pmf_stream_t s) {
  int tiles_x = 0;
  const int64_t tiles = bt_tiles(H, W, &tiles_x);
  if (!samples_dev || !counts_dev || n <= 0 || n > 65535 || tiles == 0) return PMF_E_ARG;
  hipStream_t st = (hipStream_t)s;
  hipError_t e = hipMemsetAsync(counts_dev, 0, (size_t)n * sizeof(int32_t), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(bev_sample_count_k, dim3((unsigned)(tiles < BT_COUNT_WG ? tiles : BT_COUNT_WG), n),
                     dim3(BT_TX * BT_TY), 0, st, samples_dev, H, W, tiles_x, (int)tiles, counts_dev);
  PMF_LAUNCH_CHECK();
  return 0;
}

extern "C" int pmf_bev_sample_gather(const pmf_bev_sample_t* samples_dev, int32_t B, int32_t H, int32_t W,
                                     float* feature_out, float* label_out, pmf_stream_t s) {
  int tiles_x = 0;
  const int64_t tiles = bt_tiles(H, W, &tiles_x);
  if (!samples_dev || !feature_out || !label_out || B <= 0 || B > 65535 || tiles == 0) return PMF_E_ARG;
  if ((int64_t)H * W > INT64_MAX / 4 / 8 / B) return PMF_E_ARG;          // B * 8 * H * W * 4 bytes past an int64 offset
  hipLaunchKernelGGL(bev_sample_gather_k, dim3((unsigned)tiles, B), dim3(BT_TX * BT_TY), 0, (hipStream_t)s, samples_dev, H,
                     W, tiles_x, feature_out, label_out);
  PMF_LAUNCH_CHECK();
  return 0;
}
