// Weight re-layout: PyTorch OIHW parameters -> packed implicit-GEMM slabs [tap][k][n] (gfx950).
// One batched launch re-packs every conv of the network (weights change every optimiser step), tiled through
// LDS so both the OIHW reads and the packed writes are coalesced.
//
// A workgroup stages one 32 x (CT * KHW) weight tile: 32 lanes per output-channel row, 16-byte loads over the aligned
// body of the row (scalar head and tail), then writes it in the job's layout with 16-byte stores wherever the layout
// has 16 contiguous bytes.  KHW is a template parameter (1, 4, 9, 49; 0 = any), rows and columns come from the thread
// index, and the quotients by run-time tile extents go through pack_div: no integer division in the loops of formats 0
// and 1 (the stem's format 2 is one small job and stays element by element).
#include "common.h"

// floats of one co-row slice held in LDS: 20.6 KB per workgroup.  Measured against 320 (41 KB) on the network's tables,
// every table alone: 156 us against 194 us per step (docs/rounds/r17.md) -- twice the workgroups in flight per CU hide
// the stage / barrier / write sequence of one another, and the guest leaves the main lanes more LDS
#define PACK_L 160
#define PACK_NB ((PACK_L / 4 + 31) / 32)   // 16-byte loads one lane issues per row, at most

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// a / d for 0 <= a < 2^20, d >= 1, with inv = 1.0f / d: the float product is within one of the quotient, one
// correction step makes it exact
__device__ __forceinline__ int pack_div(int a, int d, float inv) {
  int q = (int)((float)a * inv);
  if (q * d > a) --q;
  else if ((q + 1) * d <= a) ++q;
  return q;
}

// RNE three-way bf16 split of x: x ~ u0 + u1 + u2 (conv_fwd.hip consumes the planes in this order)
__device__ __forceinline__ void pack_split3(float x, unsigned& u0, unsigned& u1, unsigned& u2) {
  u0 = __builtin_bit_cast(unsigned short, (__bf16)x);
  const float r1 = x - __builtin_bit_cast(float, u0 << 16);
  u1 = __builtin_bit_cast(unsigned short, (__bf16)r1);
  const float r2 = r1 - __builtin_bit_cast(float, u1 << 16);
  u2 = __builtin_bit_cast(unsigned short, (__bf16)r2);
}

// the first `cnt` (1..8) bf16 of the four dwords p -> d (16-byte aligned); exactly 2 * cnt bytes are written
__device__ __forceinline__ void pack_store_oct(unsigned short* d, const unsigned* p, int cnt) {
  if (cnt >= 8) { *(u32x4*)d = u32x4{p[0], p[1], p[2], p[3]}; return; }
  int o = 0;
  if (cnt & 4) { *(u32x2*)d = u32x2{p[0], p[1]}; o = 2; }
  if (cnt & 2) { *(unsigned*)(d + 2 * o) = p[o]; ++o; }
  if (cnt & 1) d[2 * o] = (unsigned short)p[o];
}

template <int KHW_T>
__device__ __forceinline__ void pack_tile(const pmf_pack_job_t& J, float (*T)[PACK_L + 1], int* taps) {
  const int KHW = KHW_T ? KHW_T : J.KHW;
  const int tid = threadIdx.x;
  const int b = blockIdx.x - J.block_start;
  const int tco = b / J.tiles_ci, tci = b - tco * J.tiles_ci;      // (once per workgroup, on the scalar unit)
  const int co0 = tco * 32, ci0 = tci * J.CT;
  const int nco = min(32, J.Cout - co0), ct = min(J.CT, J.Cin - ci0);
  const int L = ct * KHW, wld = J.w_ld ? J.w_ld : J.Cin;
  const int ntaps = J.ntaps, transpose = J.transpose, format = J.format, K_pad = J.K_pad, ldw = J.ldw;
  if (tid < ntaps) taps[tid] = J.tap_idx[tid];
  {
    // stage: 32 lanes per co row, eight rows per pass; the row's `ct * KHW` floats are contiguous in OIHW
    const int lane = tid & 31;
    for (int col = tid >> 5; col < nco; col += 8) {
      const float* __restrict__ src = J.w + ((size_t)(co0 + col) * wld + ci0) * KHW;
      const int head = min(L, (int)((0u - (unsigned)((uintptr_t)src >> 2)) & 3u));   // floats up to the 16-byte boundary
      const int nv = (L - head) >> 2, tail0 = head + 4 * nv;
      f32x4 v[PACK_NB];
#pragma unroll
      for (int u = 0; u < PACK_NB; ++u)
        if (lane + 32 * u < nv) v[u] = *(const f32x4*)(src + head + 4 * (lane + 32 * u));
      if (lane < head) T[col][lane] = src[lane];
      if (tail0 + lane < L) T[col][tail0 + lane] = src[tail0 + lane];
#pragma unroll
      for (int u = 0; u < PACK_NB; ++u)
        if (lane + 32 * u < nv) {
          float* t = &T[col][head + 4 * (lane + 32 * u)];
          t[0] = v[u].x; t[1] = v[u].y; t[2] = v[u].z; t[3] = v[u].w;
        }
    }
  }
  __syncthreads();
  if (format >= 1) {
    // split-bf16 fragments: GEMM element (tap t, k, n) -> plane p of fragment (t, k/16, n/32) at lane (n%32) + 32 ((k%16)/8),
    // element k%8 (the B-operand layout of v_mfma_f32_32x32x16_bf16); planes are 512 bf16 apart
    unsigned short* __restrict__ dst = (unsigned short*)J.dst;
    const int KS = K_pad >> 4, CTL = ldw >> 5;
    const int kdim = transpose ? nco : ct, ndim = transpose ? ct : nco;
    const int kbase = transpose ? co0 : ci0, nbase = transpose ? ci0 : co0;
    if (format == 1 && (kbase & 7) == 0 && ((uintptr_t)dst & 15) == 0) {
      // one thread builds the 16 bytes a lane of the fragment holds (8 consecutive k of one n): three 16-byte stores,
      // consecutive threads -> consecutive lanes of the fragment (coalesced).  The last octet of a tile whose k extent
      // is no multiple of 8 is written in 8 / 4 / 2-byte pieces up to the extent: the padding behind it is the caller's
      const int noct = (kdim + 7) >> 3, totalv = ntaps * noct * ndim;
      const float inv_noct = 1.0f / (float)noct, inv_ndim = 1.0f / (float)ndim;
      for (int i = tid; i < totalv; i += 256) {
        const int r = pack_div(i, ndim, inv_ndim), nl = i - r * ndim;
        const int t = pack_div(r, noct, inv_noct), oc = r - t * noct;
        const int tap = taps[t], cnt = min(8, kdim - oc * 8);
        // (both operand orders: T[n][k * KHW + tap] forward, T[k][n * KHW + tap] transposed)
        const float* x0 = transpose ? &T[oc * 8][nl * KHW + tap] : &T[nl][oc * 8 * KHW + tap];
        const int xs = transpose ? PACK_L + 1 : KHW;
        unsigned p0[4], p1[4], p2[4];
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
          unsigned u[2][3];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const float x = e + h < cnt ? x0[(e + h) * xs] : 0.f;
            pack_split3(x, u[h][0], u[h][1], u[h][2]);
          }
          p0[e >> 1] = u[0][0] | (u[1][0] << 16); p1[e >> 1] = u[0][1] | (u[1][1] << 16); p2[e >> 1] = u[0][2] | (u[1][2] << 16);
        }
        const int k = kbase + oc * 8, nn = nbase + nl;
        const size_t e0 = ((((size_t)t * KS + (k >> 4)) * CTL + (nn >> 5)) * 3) * 512 + ((nn & 31) + 32 * ((k & 15) >> 3)) * 8;
        pack_store_oct(dst + e0, p0, cnt);
        pack_store_oct(dst + e0 + 512, p1, cnt);
        pack_store_oct(dst + e0 + 1024, p2, cnt);
      }
      return;
    }
    // format 2 (few-channel stem, conv_fwd.hip PIPE 14): ONE virtual tap whose K index is tap * 8 + channel, so that a
    // 16-deep MFMA step holds the 8 padded channels of TWO taps.  One small job: element by element (as is a format 1
    // tile whose k origin is no multiple of 8)
    const int total = ntaps * nco * ct;
    for (int i = tid; i < total; i += 256) {
      int col, cil, t;
      if (!transpose) { col = i % nco; const int r = i / nco; cil = r % ct; t = r / ct; }
      else { cil = i % ct; const int r = i / ct; col = r % nco; t = r / nco; }
      const float x = T[col][cil * KHW + taps[t]];
      int k = transpose ? co0 + col : ci0 + cil;
      const int nn = transpose ? ci0 + cil : co0 + col;
      if (format == 2) { k += t * 8; t = 0; }
      unsigned u0, u1, u2;
      pack_split3(x, u0, u1, u2);
      const size_t e = ((((size_t)t * KS + (k >> 4)) * CTL + (nn >> 5)) * 3) * 512 + ((nn & 31) + 32 * ((k & 15) >> 3)) * 8 + (k & 7);
      dst[e] = (unsigned short)u0; dst[e + 512] = (unsigned short)u1; dst[e + 1024] = (unsigned short)u2;
    }
    return;
  }
  // format 0, fp32 slabs dst[t][k][n]: four consecutive n per thread, one 16-byte store where dst, ldw and the tile's n origin
  // allow it (co0 is a multiple of 32; ci0 of CT, which is a multiple of 8 unless KHW > PACK_L / 8), element by element
  // otherwise; the last group of a row stores its 1..3 floats one by one
  float* __restrict__ dst = J.dst;
  const int vec_ok = ((uintptr_t)dst & 15) == 0 && (ldw & 3) == 0 && ((transpose ? ci0 : co0) & 3) == 0;
  if (!transpose) {
    // k = ci, n = co: eight 4-wide groups per (t, ci) row
    const int c4 = (tid & 7) * 4, rows = ntaps * ct;
    const float inv_ct = 1.0f / (float)ct;
    if (c4 < nco)
      for (int r = tid >> 3; r < rows; r += 32) {
        const int t = pack_div(r, ct, inv_ct), cil = r - t * ct;
        const int j = cil * KHW + taps[t], n = min(4, nco - c4);
        float* d = dst + ((size_t)t * K_pad + ci0 + cil) * ldw + co0 + c4;
        if (n == 4 && vec_ok) *(f32x4*)d = f32x4{T[c4][j], T[c4 + 1][j], T[c4 + 2][j], T[c4 + 3][j]};
        else for (int e = 0; e < n; ++e) d[e] = T[c4 + e][j];
      }
  } else {
    // k = co, n = ci: (ct + 3) / 4 groups per (t, co) row
    const int ng = (ct + 3) >> 2, total = ntaps * nco * ng;
    const float inv_ng = 1.0f / (float)ng, inv_nco = 1.0f / (float)nco;
    for (int i = tid; i < total; i += 256) {
      const int r = pack_div(i, ng, inv_ng), c4 = (i - r * ng) * 4;
      const int t = pack_div(r, nco, inv_nco), col = r - t * nco;
      const int j = c4 * KHW + taps[t], n = min(4, ct - c4);
      float* d = dst + ((size_t)t * K_pad + co0 + col) * ldw + ci0 + c4;
      if (n == 4 && vec_ok) *(f32x4*)d = f32x4{T[col][j], T[col][j + KHW], T[col][j + 2 * KHW], T[col][j + 3 * KHW]};
      else for (int e = 0; e < n; ++e) d[e] = T[col][j + e * KHW];
    }
  }
}

__global__ __launch_bounds__(256) void pack_k(const pmf_pack_job_t* __restrict__ jobs, int njobs) {
  __shared__ float T[32][PACK_L + 1];
  __shared__ int taps[PMF_MAX_TAPS + 3];
  // locate the job of this block (block_start is ascending)
  int lo = 0, hi = njobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].block_start <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const pmf_pack_job_t& J = jobs[lo];
  switch (J.KHW) {
    case 1: pack_tile<1>(J, T, taps); break;
    case 4: pack_tile<4>(J, T, taps); break;
    case 9: pack_tile<9>(J, T, taps); break;
    case 49: pack_tile<49>(J, T, taps); break;
    default: pack_tile<0>(J, T, taps);
  }
}

extern "C" int pmf_pack_tile_ci(int32_t Cin, int32_t KHW) {
  int ct = PACK_L / KHW;
  if (ct < 1) ct = 1;
  if (ct > Cin) ct = Cin;
  if (ct >= 8) ct &= ~7;      // whole k-octets per tile (the vectorised split-bf16 writer)
  return ct;
}

extern "C" int pmf_pack_weights_batched(const pmf_pack_job_t* jobs_dev, int32_t njobs, int32_t total_blocks,
                                        pmf_stream_t s) {
  if (njobs < 1 || total_blocks < 1) return PMF_E_ARG;
  hipLaunchKernelGGL(pack_k, dim3(total_blocks), dim3(256), 0, (hipStream_t)s, jobs_dev, njobs);
  PMF_LAUNCH_CHECK();
  return 0;
}
