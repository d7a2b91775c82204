// PMF evaluation on SensatUrban bird's-eye-view frames (tasks/sensat_urban/pmf_eval/infer.py of the reference, per frame):
// the device work around the network.  A frame f32[8,h,w] (three heights, a density, a mask, RGB) is cut into S x S tiles at
// several S; every tile goes through the network alone or with its six same-size test-time variants and a 16-pixel padded
// one, and the probabilities are summed into a confidence map of the frame.  The reference crops on the host, permutes with
// separate torch ops and accumulates on the host; here the frame and the confidence map stay on the device:
//   pmf_bev_tile_pre    frame window -> (x - mean) / std * mask -> pcd f32[T*V,5,S,S], rgb f32[T*V,3,S,S] (+ padded)
//   pmf_bev_tile_accum  prob f32[T*V,C,S,S] (+ padded) -> variants undone, summed in the reference's order, += the map
//   pmf_bev_points      class map int32[h,w] (or KNN votes) -> uint8 labels, += point confusion, zero count
// The variants, v = 0..5: identity, rot90(1), rot90(2), flip along W, flip along H, transpose (rot90(1): out[i][j] =
// in[j][S-1-i]).  Work is dealt in 32 x 32 pixel blocks; the two transposing variants go through a [32][33] LDS tile so
// that the global side is read and written along rows in both directions.  All stores are vector stores, no atomics on
// floating-point data: every map element has one writer per launch and the tiles are launched in list order on one stream.
#include "common.h"
#pragma clang fp contract(off)

#define BEV_MAXT 64         // tiles per call (their origins travel as kernel arguments)
#define BEV_MAXC 64         // classes of an LDS confusion histogram (16 KB)
#define BEV_GRID 1024
#define BEV_PAD 16          // border of the padded variant

struct BevOrigins {
  int32_t hs[BEV_MAXT];
  int32_t ws[BEV_MAXT];
};

// ---- (a) frame -> network inputs --------------------------------------------------------------------------------------
// Workgroup = one 32 x 32 block of one channel of one tile (256 lanes, four rows each).  The normalised block is written
// as v0 (and into the padded canvas) straight from registers, mirrored for v2 / v3 / v4 (a reversed row is still one
// contiguous segment per wave), and through the LDS tile for v1 / v5.
__global__ __launch_bounds__(256) void bev_tile_pre_k(const float* __restrict__ frame, int h, int w, BevOrigins org, int S,
                                                      int V, const float* __restrict__ mean,
                                                      const float* __restrict__ stds, float* __restrict__ pcd,
                                                      float* __restrict__ rgb, float* __restrict__ pcd_pad,
                                                      float* __restrict__ rgb_pad) {
  __shared__ float tile[32][33];
  const int nb = (S + 31) >> 5;
  const int i0 = (int)(blockIdx.x / nb) * 32, j0 = (int)(blockIdx.x % nb) * 32;
  const int c = blockIdx.y, t = blockIdx.z;
  const int hs = org.hs[t], ws = org.ws[t];
  const int tx = threadIdx.x & 31, ty0 = threadIdx.x >> 5;
  const int64_t hw = (int64_t)h * w, SS = (int64_t)S * S;
  const float m = mean[c], sd = stds[c];
  const int nch = c < 5 ? 5 : 3, cc = c < 5 ? c : c - 5;
  float* __restrict__ dst = c < 5 ? pcd : rgb;
  float val[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ty = ty0 + 8 * k;
    const int i = i0 + ty, j = j0 + tx;
    const int r = hs + i, q = ws + j;
    const bool in = i < S && j < S && r < h && q < w;         // past the frame: the zero-initialised crop of the reference
    const float x = in ? frame[c * hw + (int64_t)r * w + q] : 0.f;
    const float mk = in ? frame[4 * hw + (int64_t)r * w + q] : 0.f;
    val[k] = (x - m) / sd * mk;
    tile[ty][tx] = val[k];
  }
  __syncthreads();
  float* __restrict__ base = dst + ((int64_t)t * V * nch + cc) * SS;      // variant v: + v * nch * SS
  const int64_t vs = (int64_t)nch * SS;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ty = ty0 + 8 * k;
    const int i = i0 + ty, j = j0 + tx;
    if (i < S && j < S) {
      base[(int64_t)i * S + j] = val[k];
      if (V == 6) {
        base[2 * vs + (int64_t)(S - 1 - i) * S + (S - 1 - j)] = val[k];
        base[3 * vs + (int64_t)i * S + (S - 1 - j)] = val[k];
        base[4 * vs + (int64_t)(S - 1 - i) * S + j] = val[k];
      }
      if (pcd_pad) {
        const int SP = S + 2 * BEV_PAD;
        float* __restrict__ pp = (c < 5 ? pcd_pad : rgb_pad) + ((int64_t)t * nch + cc) * SP * SP;
        pp[(int64_t)(i + BEV_PAD) * SP + j + BEV_PAD] = val[k];
      }
    }
    if (V == 6) {
      // in[a][b] with a = i0 + tx, b = j0 + ty (the LDS tile read across): v1 puts it at [S-1-b][a], v5 at [b][a]
      const int a = i0 + tx, b = j0 + ty;
      if (a < S && b < S) {
        const float u = tile[tx][ty];
        base[1 * vs + (int64_t)(S - 1 - b) * S + a] = u;
        base[5 * vs + (int64_t)b * S + a] = u;
      }
    }
  }
}

// The 16-pixel border of the padded canvases: exactly 0 (the reference pads after normalising).  One lane per border
// element of one plane: 16 rows on top, 16 at the bottom, then 16 + 16 columns beside each of the S rows between them.
__global__ __launch_bounds__(256) void bev_pad_border_k(float* __restrict__ pcd_pad, float* __restrict__ rgb_pad, int S,
                                                        int T) {
  const int SP = S + 2 * BEV_PAD;
  const int n_rows = 2 * BEV_PAD * SP, n_border = n_rows + 2 * BEV_PAD * S;
  const int plane = blockIdx.y;                                  // t * 8 + c
  const int t = plane >> 3, c = plane & 7;
  if (t >= T) return;
  float* __restrict__ pp = (c < 5 ? pcd_pad + ((int64_t)t * 5 + c) * SP * SP : rgb_pad + ((int64_t)t * 3 + c - 5) * SP * SP);
  for (int e = blockIdx.x * 256 + threadIdx.x; e < n_border; e += gridDim.x * 256) {
    int r, q;
    if (e < n_rows) {
      r = e / SP;
      q = e - r * SP;
      if (r >= BEV_PAD) r += S;
    } else {
      const int f = e - n_rows;
      r = BEV_PAD + f / (2 * BEV_PAD);
      q = f % (2 * BEV_PAD);
      if (q >= BEV_PAD) q += S;
    }
    pp[(int64_t)r * SP + q] = 0.f;
  }
}

static bool bev_tiles_ok(int h, int w, const int32_t* origins, int T, int S, int V) {
  if (h < 1 || w < 1 || !origins || T < 1 || T > BEV_MAXT || S < 16 || S % 16 != 0 || (V != 1 && V != 6)) return false;
  for (int t = 0; t < T; ++t)
    if (origins[2 * t] < 0 || origins[2 * t] >= h || origins[2 * t + 1] < 0 || origins[2 * t + 1] >= w) return false;
  return true;
}

extern "C" int pmf_bev_tile_pre(const float* frame, int32_t h, int32_t w, const float* mean, const float* stds,
                                const int32_t* origins, int32_t T, int32_t S, int32_t V, float* pcd, float* rgb,
                                float* pcd_pad, float* rgb_pad, pmf_stream_t s) {
  if (!frame || !mean || !stds || !pcd || !rgb || (pcd_pad == nullptr) != (rgb_pad == nullptr)) return PMF_E_ARG;
  if (!bev_tiles_ok(h, w, origins, T, S, V)) return PMF_E_ARG;
  BevOrigins org;
  for (int t = 0; t < T; ++t) { org.hs[t] = origins[2 * t]; org.ws[t] = origins[2 * t + 1]; }
  const int nb = (S + 31) / 32;
  hipLaunchKernelGGL(bev_tile_pre_k, dim3(nb * nb, 8, T), dim3(256), 0, (hipStream_t)s, frame, h, w, org, S, V, mean, stds,
                     pcd, rgb, pcd_pad, rgb_pad);
  PMF_LAUNCH_CHECK();
  if (pcd_pad) {
    const int n_border = 2 * BEV_PAD * (S + 2 * BEV_PAD) + 2 * BEV_PAD * S;
    hipLaunchKernelGGL(bev_pad_border_k, dim3(cdiv(n_border, 256), 8 * T), dim3(256), 0, (hipStream_t)s, pcd_pad, rgb_pad,
                       S, T);
    PMF_LAUNCH_CHECK();
  }
  return 0;
}

// ---- (b) network outputs -> confidence map ----------------------------------------------------------------------------
// One launch per tile, in list order on the stream (tiles overlap where the last row / column is shifted back, and the
// per-pixel order of the additions is part of the result).  Workgroup = one 32 x 32 block of one class of the tile; each
// lane owns its four map elements: no two lanes of a launch write the same one.  p1 (undone by rot90(3): d1[i][j] =
// p1[S-1-j][i]) and p5 (d5[i][j] = p5[j][i]) are read along their rows into the LDS tiles and picked up across.
__global__ __launch_bounds__(256) void bev_tile_accum_k(const float* __restrict__ prob, const float* __restrict__ prob_pad,
                                                        int C, int S, int V, int hs, int ws, int hv, int wv,
                                                        float* __restrict__ cmap, int h, int w) {
  __shared__ float t1[32][33];
  __shared__ float t5[32][33];
  const int nb = (S + 31) >> 5;
  const int i0 = (int)(blockIdx.x / nb) * 32, j0 = (int)(blockIdx.x % nb) * 32;
  const int c = blockIdx.y;
  const int tx = threadIdx.x & 31, ty0 = threadIdx.x >> 5;
  const int64_t SS = (int64_t)S * S, vs = (int64_t)C * SS;
  const float* __restrict__ p = prob + (int64_t)c * SS;             // variant v: + v * vs
  if (V == 6) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int ty = ty0 + 8 * k;
      const int j = j0 + ty, i = i0 + tx;                           // the element that output [i][j] needs
      const bool in = i < S && j < S;
      t1[ty][tx] = in ? p[1 * vs + (int64_t)(S - 1 - j) * S + i] : 0.f;
      t5[ty][tx] = in ? p[5 * vs + (int64_t)j * S + i] : 0.f;
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ty = ty0 + 8 * k;
    const int i = i0 + ty, j = j0 + tx;
    if (i >= hv || j >= wv) continue;                               // only the part of the tile the frame filled
    float sum = p[(int64_t)i * S + j];
    if (V == 6) {
      sum = sum + t1[tx][ty];
      sum = sum + p[2 * vs + (int64_t)(S - 1 - i) * S + (S - 1 - j)];
      sum = sum + p[3 * vs + (int64_t)i * S + (S - 1 - j)];
      sum = sum + p[4 * vs + (int64_t)(S - 1 - i) * S + j];
      sum = sum + t5[tx][ty];
      if (prob_pad) {
        const int SP = S + 2 * BEV_PAD;
        sum = sum + prob_pad[(int64_t)c * SP * SP + (int64_t)(i + BEV_PAD) * SP + j + BEV_PAD];
      }
    }
    float* __restrict__ o = cmap + (int64_t)c * h * w + (int64_t)(hs + i) * w + ws + j;
    *o = *o + sum;
  }
}

extern "C" int pmf_bev_tile_accum(const float* prob, const float* prob_pad, int32_t C, const int32_t* origins, int32_t T,
                                  int32_t S, int32_t V, float* conf_map, int32_t h, int32_t w, pmf_stream_t s) {
  if (!prob || !conf_map || C < 1 || C > 65535) return PMF_E_ARG;
  if (!bev_tiles_ok(h, w, origins, T, S, V)) return PMF_E_ARG;
  if (prob_pad && V != 6) return PMF_E_ARG;
  const int nb = (S + 31) / 32;
  const int64_t SS = (int64_t)S * S, SP2 = (int64_t)(S + 2 * BEV_PAD) * (S + 2 * BEV_PAD);
  for (int t = 0; t < T; ++t) {
    const int hs = origins[2 * t], ws = origins[2 * t + 1];
    const int hv = h - hs < S ? h - hs : S, wv = w - ws < S ? w - ws : S;
    hipLaunchKernelGGL(bev_tile_accum_k, dim3(nb * nb, C), dim3(256), 0, (hipStream_t)s, prob + (int64_t)t * V * C * SS,
                       prob_pad ? prob_pad + (int64_t)t * C * SP2 : nullptr, C, S, V, hs, ws, hv, wv, conf_map, h, w);
    PMF_LAUNCH_CHECK();
  }
  return 0;
}

// ---- (c) class map -> point labels ------------------------------------------------------------------------------------
// One lane per point: pred = the class at its pixel (or the KNN vote handed in), 0 -> 1 (counted), the (pred, label + 1)
// count into the workgroup's LDS histogram (flushed with 64-bit integer atomics, as eval.hip does), pred - 1 out as uint8.
// label + 1 wraps in uint8 as the reference's numpy addition does.  A point outside the map reads class 0.
__global__ __launch_bounds__(256) void bev_points_k(const int32_t* __restrict__ cmap, int h, int w,
                                                    const int64_t* __restrict__ h_idx, const int64_t* __restrict__ w_idx,
                                                    int64_t P, const int64_t* __restrict__ pred_in,
                                                    const uint8_t* __restrict__ label, int C,
                                                    unsigned long long* __restrict__ conf,
                                                    unsigned long long* __restrict__ n_zero, uint8_t* __restrict__ out) {
  __shared__ unsigned hist[BEV_MAXC * BEV_MAXC];
  __shared__ unsigned wave_z[4];
  if (conf) {
    for (int k = threadIdx.x; k < C * C; k += 256) hist[k] = 0u;
    __syncthreads();
  }
  unsigned nz = 0;
  for (int64_t k = blockIdx.x * (int64_t)256 + threadIdx.x; k < P; k += (int64_t)gridDim.x * 256) {
    int pred = 0;
    if (pred_in) {
      pred = (int)pred_in[k];
    } else {
      const int64_t r = h_idx[k], q = w_idx[k];
      if (r >= 0 && r < h && q >= 0 && q < w) pred = cmap[r * w + q];
    }
    if (pred == 0) { pred = 1; ++nz; }
    if (conf) {
      const int t = (uint8_t)(label[k] + 1);
      if (t < C && pred >= 0 && pred < C) atomicAdd(&hist[pred * C + t], 1u);
    }
    out[k] = (uint8_t)(pred - 1);
  }
  if (conf) {
    __syncthreads();
    for (int k = threadIdx.x; k < C * C; k += 256)
      if (hist[k]) atomicAdd(conf + k, (unsigned long long)hist[k]);
  }
  if (n_zero) {
    for (int d = 32; d >= 1; d >>= 1) nz += __shfl_down(nz, d, 64);
    if ((threadIdx.x & 63) == 0) wave_z[threadIdx.x >> 6] = nz;
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned long long tot = (unsigned long long)wave_z[0] + wave_z[1] + wave_z[2] + wave_z[3];
      if (tot) atomicAdd(n_zero, tot);
    }
  }
}

extern "C" int pmf_bev_points(const int32_t* class_map, int32_t h, int32_t w, const int64_t* h_idx, const int64_t* w_idx,
                              int64_t P, const int64_t* pred_in, const uint8_t* label, int32_t C, int64_t* conf,
                              int64_t* n_zero, uint8_t* out, pmf_stream_t s) {
  if (P < 0 || C < 1 || h < 1 || w < 1) return PMF_E_ARG;
  if (P == 0) return 0;
  if (!out) return PMF_E_ARG;
  if (!pred_in && (!class_map || !h_idx || !w_idx)) return PMF_E_ARG;
  if (conf && (!label || C > BEV_MAXC)) return PMF_E_ARG;
  const int64_t g = cdiv64(P, 256);
  hipLaunchKernelGGL(bev_points_k, dim3((unsigned)(g < BEV_GRID ? g : BEV_GRID)), dim3(256), 0, (hipStream_t)s, class_map, h,
                     w, h_idx, w_idx, P, pred_in, label, C, (unsigned long long*)conf, (unsigned long long*)n_zero, out);
  PMF_LAUNCH_CHECK();
  return 0;
}
