// Implicit-GEMM convolution, NHWC, LDS halo staging, fp32 in / out / accumulate.  gfx950 only.
//
// Arithmetic: the pipelined layer classes (PIPE 5-12: ~99 % of the forward / input-gradient flops) compute every fp32
// product as SIX v_mfma_f32_32x32x16_bf16 products of three-way bf16-split operands with fp32 accumulation (fp32-class
// error, see "PIPE 5" below); the generic loops (PIPE 0/1/4: the 7x7 stem, ragged channel counts, PMF_CONV_F32=1) use
// v_mfma_f32_32x32x2_f32.
// GEMM view:  M = output pixels (32-pixel row segments), N = Cout, K = taps x concatenated input channels.
// A 256-thread workgroup (4 waves) owns a TH x TW output tile = 4*MT segments of 32 pixels and BN output
// channels; wave w owns segments [w*MT, w*MT+MT) x all BN channels  ->  MT x BN/32 accumulators of 32x32.
// K loop: for every 16-channel chunk of every operand, the input tile INCLUDING ITS HALO is staged once in
// LDS (with BatchNorm-apply / ReLU / Dropout2d multiplier folded into the load and zero padding applied
// after it) and reused by all taps; the matching weight slab / weight fragments are staged next to it (LDS-DMA).
// fp32-MFMA operands: A[i=lane&31][k=lane>>5] = one ds_read_b128 per 8 channels (pixel pitch 20 floats ->
// conflict-free), B[k][j=lane&31] = ds_read_b32 from the [k][BN] slab (32 consecutive banks).
// Epilogue (conv_epi.h): + bias, activation, optional (n,c) multiplier / ReLU mask (input-gradient form), optional
// per-channel sum / sum-of-squares for the BatchNorm that follows, coalesced 128-B row stores.
#include "conv_epi.h"
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>

#define KC 16
#define APITCH 20
#define TAPG 9

#ifdef PMF_CONV_TRACE
extern "C" int pmf_conv_trace_set(void* p) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(pmf_trace_buf), &p, sizeof(p)); }
#endif


// NTAPS taps x 16 channels of one staged chunk, fully unrolled and branch-free.  The LDS operands of step i+1 (one
// ds_read_b128 per M tile + 4 ds_read_b32 per N tile) are issued BEFORE the 4*MT*NT MFMAs of step i (explicit double
// buffer + sched_barrier): left alone hipcc emits read -> wait -> 2 mfma groups, four exposed LDS round trips per step.
struct NoFill { __device__ __forceinline__ void operator()(int, int) const {} };

// NTAPS taps x 16 channels of one staged chunk, fully unrolled and branch-free.  The LDS operands of step i+1 (one
// ds_read_b128 per M tile + 4 ds_read_b32 per N tile) are issued BEFORE the 4*MT*NT MFMAs of step i (explicit double
// buffer + sched_barrier): left alone hipcc emits read -> wait -> 2 mfma groups, four exposed LDS round trips per step.

// scheduling recipe of one MFMA step: MFMA i is followed by its share of the NR LDS reads of the NEXT step (and, behind
// the first two, one global load of the staging slice): the builtin wants literal counts, hence the recursion
template <int I, int NM, int NR>
__device__ __forceinline__ void pmf_sgb_seq() {
  if constexpr (I < NM) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    constexpr int k = (NR * (I + 1)) / NM - (NR * I) / NM;
    if constexpr (k > 0) __builtin_amdgcn_sched_group_barrier(0x100, k, 0);
    if constexpr (I < 2) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    pmf_sgb_seq<I + 1, NM, NR>();
  }
}

template <int BN, int MT, int NTAPS, class Fill = NoFill>
__device__ __forceinline__ void conv_steps(f32x16 (&acc)[MT][BN / 32], const float* __restrict__ As,
                                           const float* __restrict__ Bs, const int (&abase)[MT],
                                           const int (&aoff)[TAPG], int kca, int li, int lh, Fill fill = Fill()) {
  constexpr int NT = BN / 32, NS = NTAPS * 2;
  f32x4 a[2][MT];
  float b[2][NT][4];
  const float* bp0 = Bs + (lh * 4) * BN + li;
#pragma unroll
  for (int m = 0; m < MT; ++m) a[0][m] = *(const f32x4*)(As + abase[m] + aoff[0]);
#pragma unroll
  for (int u = 0; u < NT; ++u)
#pragma unroll
    for (int q = 0; q < 4; ++q) b[0][u][q] = bp0[q * BN + u * 32];
#pragma unroll
  for (int st = 0; st < NS; ++st) {
    const int cur = st & 1, nxt = cur ^ 1;
    if (st + 1 < NS) {
      const int tl = (st + 1) >> 1, kg = ((st + 1) & 1) * 8;
      const float* bp = bp0 + (tl * kca + kg) * BN;
#pragma unroll
      for (int m = 0; m < MT; ++m) a[nxt][m] = *(const f32x4*)(As + abase[m] + aoff[tl] + kg);
#pragma unroll
      for (int u = 0; u < NT; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q) b[nxt][u][q] = bp[q * BN + u * 32];
    }
    fill(st, NS);   // a slice of the NEXT chunk's global loads rides along with every step
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int u = 0; u < NT; ++u)
          acc[m][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][m][q], b[cur][u][q], acc[m][u], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ------------------------------------------------------------------------------------------------------------
// Software-pipelined K loop for the common case (host-checked, conv_simple()): one LDS tile with halo shared by all
// taps, ntaps in {1,4,9}, stride 1, every operand a multiple of 16 channels with the same H x W, no broadcast.
//   * input tile: per-thread slot tables (pixel offset / validity of every float4 this thread stages) are computed
//     ONCE per workgroup; the loads of chunk i+1 (buffer_load_dwordx4, 32-bit offsets) are issued into registers during
//     the first MFMA steps of chunk i, so HBM / L2 latency runs under MFMAs; the staging phase between chunks is only
//     BatchNorm-apply / ReLU / mask + ds_write_b128;
//   * weights need no transform: they go global -> LDS by LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave
//     instruction, no VGPRs, no ds_write).  The [taps][16][BN] slab is split into two 8-channel halves that ping-pong:
//     while the MFMAs read half h, the DMA fills the other half.
// One chunk = barrier X | store A | barrier Y | DMA B(h1), loads A(next), MFMA(h0) | barrier Z | DMA B(next,h0), MFMA(h1).
typedef __attribute__((address_space(3))) void* lds_ptr_t;

template <int BN, int MT, int NTAPS, class Fill = NoFill>
__device__ __forceinline__ void conv_half(f32x16 (&acc)[MT][BN / 32], const float* __restrict__ As,
                                          const float* __restrict__ Bh, const int (&abase)[MT], const int (&aoff)[TAPG],
                                          int kg, int li, int lh, Fill fill = Fill()) {
  constexpr int NT = BN / 32;
  f32x4 a[2][MT];
  float b[2][NT][4];
  const float* bp0 = Bh + (lh * 4) * BN + li;
#pragma unroll
  for (int m = 0; m < MT; ++m) a[0][m] = *(const f32x4*)(As + abase[m] + aoff[0] + kg);
#pragma unroll
  for (int u = 0; u < NT; ++u)
#pragma unroll
    for (int q = 0; q < 4; ++q) b[0][u][q] = bp0[q * BN + u * 32];
#pragma unroll
  for (int st = 0; st < NTAPS; ++st) {
    const int cur = st & 1, nxt = cur ^ 1;
    if (st + 1 < NTAPS) {
      const float* bp = bp0 + (st + 1) * 8 * BN;
#pragma unroll
      for (int m = 0; m < MT; ++m) a[nxt][m] = *(const f32x4*)(As + abase[m] + aoff[st + 1] + kg);
#pragma unroll
      for (int u = 0; u < NT; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q) b[nxt][u][q] = bp[q * BN + u * 32];
    }
    fill(st, NTAPS);
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int u = 0; u < NT; ++u)
          acc[m][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][m][q], b[cur][u][q], acc[m][u], 0, 0, 0);
    // the next step's LDS reads (and this step's slice of global loads) go INTO the 64-cycle gaps behind the MFMAs
    // instead of in front of the block (hipcc otherwise waits lgkmcnt(0) right behind the reads it has just issued)
    pmf_sgb_seq<0, 4 * MT * NT, MT + 4 * NT, 2>();
    __builtin_amdgcn_sched_barrier(0);
  }
}

// VT > 1 (1x1 convolutions whose operands are multiples of 16*VT channels): one stage carries VT consecutive
// 16-channel chunks as "virtual taps" (same pixel, channel offset 16*t): a 16-channel stage of a 1x1 layer holds only
// 16 MFMAs per wave between three barriers (latency-bound); 64-channel stages amortise them 4x.
template <int BN, int MT, int VT>
__device__ __forceinline__ void conv_kloop_pipe(const pmf_conv_desc_t& d, const ConvGeom& g, f32x16 (&acc)[MT][BN / 32],
                                                float* __restrict__ As, float* __restrict__ Bs, const int (&segrow)[MT],
                                                const int (&segcol)[MT], int tid, int li, int lh, int n, int n0, int ks,
                                                int oy0, int ox0, int& tri_) {
  constexpr int ASL = VT > 1 ? 2 * VT : (MT == 2 ? 7 : 5);   // float4 slots per thread for the input tile
  constexpr int RPI = 256 / BN;                   // weight rows one 1-KiB DMA wave-instruction covers
  constexpr int NDMA = ((VT > 1 ? VT : TAPG) * 8 / RPI + 3) / 4;  // DMA instructions per wave per half slab
  const int in_cols = g.in_cols;
  const int sH = d.src[0].H, sW = d.src[0].W;
  const int q = tid & 3;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int npixA = g.in_rows * in_cols;
  const int totalA = npixA * 4 * VT;
  const int ntaps_eff = VT > 1 ? VT : d.ntaps;
  const int hrows = ntaps_eff * 8;                // rows of one half slab
  float* __restrict__ Bh1 = Bs + hrows * BN;
  int gA[ASL];
  unsigned okA = 0u;
#pragma unroll
  for (int j = 0; j < ASL; ++j) {
    const int f = tid + 256 * j, pix = VT > 1 ? (f >> 2) - pmf_fdiv(f >> 2, npixA, 1.f / (float)npixA) * npixA : (f >> 2);
    const int r = pmf_fdiv(pix, in_cols, 1.f / (float)in_cols), c = pix - r * in_cols;
    const int iy = oy0 + g.dy_min + r, ix = ox0 + g.dx_min + c;
    const bool ok = f < totalA && iy >= 0 && iy < sH && ix >= 0 && ix < sW;
    gA[j] = ok ? (n * sH + iy) * sW + ix : -1;   // -1: negative byte offset = out of range = the buffer load returns 0
    okA |= ok ? (1u << j) : 0u;
  }
  TR();   // (trace) slot table done
  int offB[NDMA];   // per-lane source offset (floats) of DMA instruction wave + 4*jj, relative to the half's first row
#pragma unroll
  for (int jj = 0; jj < NDMA; ++jj) {
    const int row = (wave + 4 * jj) * RPI + lane / (BN / 4);
    offB[jj] = ((row >> 3) * (VT > 1 ? KC : g.Ktot) + (row & 7)) * d.ldw + (lane % (BN / 4)) * 4;
  }
  int aoff[TAPG];
  {
    int ty[TAPG], tx[TAPG];                                // the first TAPG table entries, fetched as one batch
#pragma unroll
    for (int t = 0; t < TAPG; ++t) { ty[t] = d.tdy[t]; tx[t] = d.tdx[t]; }
    PMF_SGPR_BATCH("s"(ty[0]), "s"(ty[1]), "s"(ty[2]), "s"(ty[3]), "s"(ty[4]), "s"(ty[5]), "s"(ty[6]), "s"(ty[7]),
                   "s"(ty[8]), "s"(tx[0]), "s"(tx[1]), "s"(tx[2]), "s"(tx[3]), "s"(tx[4]), "s"(tx[5]), "s"(tx[6]),
                   "s"(tx[7]), "s"(tx[8]));
#pragma unroll
    for (int t = 0; t < TAPG; ++t) {
      if (VT > 1) aoff[t] = t < VT ? t * g.a_floats : 0;   // virtual tap t = 16-channel chunk t of the stage
      else aoff[t] = t < d.ntaps ? ((ty[t] - g.dy_min) * in_cols + (tx[t] - g.dx_min)) * APITCH : 0;
    }
  }
  int abase[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) abase[m] = (segrow[m] * in_cols + segcol[m] * 32 + li) * APITCH + lh * 4;

  // stage iterator over (operand, 16*VT-channel stage), split-K stages dealt round-robin
  int si = 0, c0 = 0, kb = 0, cn = 0;
  auto settle = [&]() {   // move (si, c0) forward to the next chunk owned by this workgroup; false at the end
    for (;;) {
      if (si >= d.nsrc) return false;
      if (c0 >= d.src[si].C) { kb += d.src[si].C; ++si; c0 = 0; continue; }
      if ((cn % g.ksplit) == ks) return true;
      ++cn; c0 += KC * VT;
    }
  };
  f32x4 rA[ASL], sc4[VT], sh4[VT], cm4[VT];
  int cur_flags = 0;
  bool cur_aff = false;
  __amdgpu_buffer_rsrc_t nrs;           // operand of the stage being fetched
  int nld = 0, ncch = 0;
  const float* __restrict__ nw = nullptr;   // first weight row of the stage being fetched (uniform)
  auto head = [&]() {   // per-stage scalars + the channel transform of stage (si, c0)
    const float* sx = d.src[si].x;
    const float* ssc = d.src[si].scale;
    const float* ssh = d.src[si].shift;
    const float* scm = d.src[si].cmul;
    const int sld = d.src[si].ldc, sfl = d.src[si].flags, scl = d.src[si].cmul_ld;
    PMF_SGPR_BATCH("s"(sx), "s"(ssc), "s"(ssh), "s"(scm), "s"(sld), "s"(sfl), "s"(scl));   // one scalar-cache round trip
    nrs = __builtin_amdgcn_make_buffer_rsrc((void*)sx, 0, d.N * sH * sW * sld * 4, 0x00020000);
    nld = sld; ncch = c0 + q * 4;
    cur_flags = sfl;
    cur_aff = ssc != nullptr;
#pragma unroll
    for (int v = 0; v < VT; ++v) {      // channel transform of virtual tap v (channels ncch + 16 v ...)
      sc4[v] = f32x4{1.f, 1.f, 1.f, 1.f}; sh4[v] = f32x4{0.f, 0.f, 0.f, 0.f}; cm4[v] = f32x4{1.f, 1.f, 1.f, 1.f};
      if (cur_aff) {
        sc4[v] = *(const f32x4*)(ssc + ncch + KC * v);
        sh4[v] = *(const f32x4*)(ssh + ncch + KC * v);
      }
      if (scm) cm4[v] = *(const f32x4*)(scm + (size_t)n * scl + ncch + KC * v);
    }
    nw = d.w + (size_t)(kb + c0) * d.ldw + n0;
  };
  // slot j of the staging tile: VT > 1 lays the tile out [virtual tap][pixel][4 float4]; with 128-pixel tiles
  // (no halo) slots 2v and 2v+1 belong to virtual tap v
  auto loadA = [&](int j) {   // j is a compile-time constant after unrolling; branch-free (see gA)
    const int vch = VT > 1 ? ((tid + 256 * j) >> 2) / npixA * KC : 0;
    rA[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(nrs, (gA[j] * nld + ncch + vch) * 4, 0, 0));
  };
  auto dma_half = [&](const float* __restrict__ wsrc, float* __restrict__ dst) {
#pragma unroll
    for (int jj = 0; jj < NDMA; ++jj) {
      const int i = wave + 4 * jj;                 // wave-uniform
      if (i * RPI < hrows)
        __builtin_amdgcn_global_load_lds(wsrc + offB[jj], (lds_ptr_t)(dst + i * 256), 16, 0, 0);
    }
  };
  TR();   // (trace) tap / weight offsets done
  bool have = settle();
  const float* __restrict__ wcur = nullptr;
  if (have) {
    head();
    TR();   // (trace) stage scalars + channel transform loaded
#pragma unroll
    for (int j = 0; j < ASL; ++j) loadA(j);
    dma_half(nw, Bs);
  }
  TR();
  auto storeA = [&](float* __restrict__ dst) {     // registers -> LDS with the operand's view folded in
#pragma unroll
    for (int j = 0; j < ASL; ++j) {
      const int f = tid + 256 * j;
      if (f < totalA) {
        // VT > 1: the tile has no halo and 128 pixels, so the virtual tap of slot j is the compile-time j / 2
        const int v = VT > 1 ? (j * 256 * VT) / (ASL * 256) : 0;
        f32x4 t = {0.f, 0.f, 0.f, 0.f};
        if ((okA >> j) & 1u) {
          t = rA[j];
          if (cur_aff) t = t * sc4[v] + sh4[v];
          if (cur_flags & PMF_SRC_RELU) {
            t.x = fmaxf(t.x, 0.f); t.y = fmaxf(t.y, 0.f); t.z = fmaxf(t.z, 0.f); t.w = fmaxf(t.w, 0.f);
          }
          t = t * cm4[v];
        }
        if (VT > 1) *(f32x4*)(dst + v * g.a_floats + ((f >> 2) - v * npixA) * APITCH + q * 4) = t;
        else *(f32x4*)(dst + (f >> 2) * APITCH + q * 4) = t;
      }
    }
  };
  auto fill = [&](int st, int ns) {      // the next chunk's input loads ride along with the first MFMA steps
    constexpr int per = 2;
#pragma unroll
    for (int j = 0; j < ASL; ++j)
      if (j >= st * per && j < (st + 1) * per) loadA(j);
    if (st == ns - 1) {
#pragma unroll
      for (int j = 0; j < ASL; ++j)
        if (j >= ns * per) loadA(j);
    }
  };
  auto mfma_half = [&](const float* __restrict__ At, const float* __restrict__ Bt, int kg, bool with_fill) {
    // hipcc would hoist all taps x MT LDS addresses (abase + aoff) out of the chunk loop and keep them in VGPRs for
    // the whole kernel; an opaque copy per half keeps the adds next to their ds_reads
#pragma unroll
    for (int m = 0; m < MT; ++m) asm volatile("" : "+v"(abase[m]));
    __builtin_amdgcn_sched_barrier(0);
    if (with_fill) {
      if (VT > 1) conv_half<BN, MT, VT>(acc, At, Bt, abase, aoff, kg, li, lh, fill);
      else if (d.ntaps == 9) conv_half<BN, MT, 9>(acc, At, Bt, abase, aoff, kg, li, lh, fill);
      else if (d.ntaps == 3) conv_half<BN, MT, 3>(acc, At, Bt, abase, aoff, kg, li, lh, fill);
      else if (d.ntaps == 4) conv_half<BN, MT, 4>(acc, At, Bt, abase, aoff, kg, li, lh, fill);
      else if (d.ntaps == 2) conv_half<BN, MT, 2>(acc, At, Bt, abase, aoff, kg, li, lh, fill);
      else conv_half<BN, MT, 1>(acc, At, Bt, abase, aoff, kg, li, lh, fill);
    } else {
      if (VT > 1) conv_half<BN, MT, VT>(acc, At, Bt, abase, aoff, kg, li, lh);
      else if (d.ntaps == 9) conv_half<BN, MT, 9>(acc, At, Bt, abase, aoff, kg, li, lh);
      else if (d.ntaps == 3) conv_half<BN, MT, 3>(acc, At, Bt, abase, aoff, kg, li, lh);
      else if (d.ntaps == 4) conv_half<BN, MT, 4>(acc, At, Bt, abase, aoff, kg, li, lh);
      else if (d.ntaps == 2) conv_half<BN, MT, 2>(acc, At, Bt, abase, aoff, kg, li, lh);
      else conv_half<BN, MT, 1>(acc, At, Bt, abase, aoff, kg, li, lh);
    }
  };
  while (have) {
    __syncthreads();                       // X: everyone finished the MFMAs of the previous chunk
    TR();
    storeA(As);
    wcur = nw;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of B(h0) has landed in LDS
    __syncthreads();                       // Y: input tile + half 0 visible
    TR();
    ++cn; c0 += KC * VT;
    have = settle();
    if (have) head();
    else nrs = __builtin_amdgcn_make_buffer_rsrc((void*)d.src[0].x, 0, 0, 0x00020000);   // last chunk: loads fetch nothing
    dma_half(wcur + (size_t)8 * d.ldw, Bh1);
    mfma_half(As, Bs, 0, true);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // B(h1) (and the next input tile) landed
    __syncthreads();                       // Z: everyone finished reading half 0
    TR();
    if (have) dma_half(nw, Bs);
    mfma_half(As, Bh1, 8, false);
    TR();
  }
}

// ------------------------------------------------------------------------------------------------------------
// PIPE 5: fp32 convolution on the bf16 matrix pipe by operand splitting (the pipelined class only).
// Every fp32 operand x is written as x = h1 + h2 + h3 with h1 = bf16(x), h2 = bf16(x - h1), h3 = bf16(x - h1 - h2)
// (round-to-nearest-even; both subtractions are exact in fp32 and 3 x 8 significand bits cover the 24 of fp32, so the
// split itself is exact up to 2^-25 |x|).  A product a*b is then the sum of the SIX bf16 products of order <= 2^-16
//      a1 b1 + (a1 b2 + a2 b1) + (a1 b3 + a2 b2 + a3 b1),
// each exact in the fp32 accumulator of v_mfma_f32_32x32x16_bf16; what is dropped (a2 b3 + a3 b2 + a3 b3) is below
// 2^-23 |a b| -- the size of ONE fp32 rounding of the product, so the result carries fp32-class error (pinned against the
// float64 oracle by the same tests and tolerances as the v_mfma_f32_32x32x2_f32 path; PMF_CONV_F32=1 selects that path).
// Six 32-cycle MFMAs cover 16 channels of a 32x32 tile where the fp32 pipe needs eight 64-cycle ones (2.67x).
//   * input tile: staged exactly like PIPE 1 (slot tables, loads a chunk ahead, BatchNorm-apply / ReLU / mask folded
//     in), then split while it is written to LDS as [pixel][plane][16 bf16], pixel pitch 112 B (an odd number of 16-B
//     slots: the 16-lane groups of ds_read_b128 hit 16 distinct slots);
//   * weights: split ONCE per optimiser step by the pack kernel and stored in MFMA B-fragment order
//     [tap][K/16][Cout/32][plane][lane][8 bf16]: one fragment = 1 KiB contiguous = one LDS-DMA wave instruction, and
//     its LDS image is lane-linear (conflict-free reads).  The taps of a chunk are split into two halves that ping-pong
//     like the channel halves of PIPE 1.
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
#define S3_APB 112

__device__ __forceinline__ unsigned s3_pk(f32x2 v) { return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2)); }
__device__ __forceinline__ f32x2 s3_unpk(unsigned u) {
  return f32x2{__builtin_bit_cast(float, u << 16), __builtin_bit_cast(float, u & 0xffff0000u)};
}
__device__ __forceinline__ float s3_vmax(float a, float b) {   // plain v_max_f32 (fmaxf adds a canonicalising v_max)
  float r;
  asm("v_max_f32_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// two floats -> their three bf16 planes (packed pairs)
__device__ __forceinline__ void s3_split2(float a, float b, unsigned& p0, unsigned& p1, unsigned& p2) {
  f32x2 r = {a, b};
  p0 = s3_pk(r);
  r = r - s3_unpk(p0);
  p1 = s3_pk(r);
  r = r - s3_unpk(p1);
  p2 = s3_pk(r);
}

// MFMA i of NM is followed by its share of the NR LDS reads, all of them behind the first NF MFMAs (the tail of the
// step gives the last reads time to land before the next step's first MFMA wants them), and one global load behind
// each of the first NV
template <int I, int NM, int NR, int NF, int NV>
__device__ __forceinline__ void s3_sgb() {
  if constexpr (I < NM) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    if constexpr (I < NF) {
      constexpr int k = (NR * (I + 1)) / NF - (NR * I) / NF;
      if constexpr (k > 0) __builtin_amdgcn_sched_group_barrier(0x100, k, 0);
    }
    if constexpr (I < NV) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    s3_sgb<I + 1, NM, NR, NF, NV>();
  }
}

// NTH taps of one half: A fragments (MT x 3 planes) and B fragments (NT x 3 planes) of tap i+1 are read while the
// 6 MT NT MFMAs of tap i run
template <int BN, int MT, int NTH, class Fill = NoFill>
__device__ __forceinline__ void s3_half(f32x16 (&acc)[MT][BN / 32], const char* __restrict__ As,
                                        const char* __restrict__ Bh, const int (&abase)[MT], const int (&aoff)[TAPG],
                                        int t0, int lane, Fill fill = Fill()) {
  constexpr int NT = BN / 32;
  bf16x8 a[2][MT][3], b[2][NT][3];
  const char* bp0 = Bh + lane * 16;
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int p = 0; p < 3; ++p) a[0][m][p] = *(const bf16x8*)(As + abase[m] + aoff[t0] + p * 32);
#pragma unroll
  for (int u = 0; u < NT; ++u)
#pragma unroll
    for (int p = 0; p < 3; ++p) b[0][u][p] = *(const bf16x8*)(bp0 + (u * 3 + p) * 1024);
  __builtin_amdgcn_sched_barrier(0);   // (keeps the first tap's reads out of the interleave pattern of its MFMAs)
#pragma unroll
  for (int st = 0; st < NTH; ++st) {
    const int cur = st & 1, nxt = cur ^ 1;
    if (st + 1 < NTH) {
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int p = 0; p < 3; ++p) a[nxt][m][p] = *(const bf16x8*)(As + abase[m] + aoff[t0 + st + 1] + p * 32);
#pragma unroll
      for (int u = 0; u < NT; ++u)
#pragma unroll
        for (int p = 0; p < 3; ++p) b[nxt][u][p] = *(const bf16x8*)(bp0 + (((st + 1) * NT + u) * 3 + p) * 1024);
    }
    fill(st, NTH);
    // smallest terms first; product-major so that back-to-back MFMAs hit different accumulators
    constexpr int PA[6] = {0, 1, 2, 0, 1, 0}, PB[6] = {2, 1, 0, 1, 0, 0};
#pragma unroll
    for (int pr = 0; pr < 6; ++pr)
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int u = 0; u < NT; ++u)
          acc[m][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[cur][m][PA[pr]], b[cur][u][PB[pr]], acc[m][u], 0, 0, 0);
    // the next tap's 3 (MT + NT) LDS reads and this step's slice of global loads go into the gaps behind the MFMAs
    s3_sgb<0, 6 * MT * NT, 3 * (MT + NT), (6 * MT * NT * 2 + 2) / 3, 2>();
    __builtin_amdgcn_sched_barrier(0);
  }
}

// SL = 16-channel slabs per stage.  Few-tap convolutions (1x1, 2x2, 1x3) carry SL = 4 / 2 slabs per stage as "virtual
// taps" v = tap * SL + slab (same idea as VT of PIPE 4): a 16-channel stage of a 1x1 layer is 6 MT NT MFMAs between
// three barriers.  Stages are sized so that virtual taps <= 9 and the staging slots per thread <= 8.
// NTAPS: 9 = the 3x3 case with its tap count known at compile time (no dispatch on the half sizes inside the stage
// loop: the branches end scheduling regions and cost accumulator copies at their joins), 0 = read from the descriptor
// ONE: a single operand and no K split (most 3x3 layers): the operand's scalars are fetched once, in front of the loop.
// The generic stage iterator re-reads them from the kernel arguments every stage -- s_load -> s_waitcnt round trips
// (settle: the channel count; head: pointers, pitch, flags) that sit between barrier Y and the first MFMA of the stage,
// on the critical path of a one-wave-per-SIMD schedule.
template <int BN, int MT, int SL, int NTAPS = 0, int IS = 1, bool ONE = false>      // IS: input stride (2: the stride-2 3x3 layers, MT = 1 only)
__device__ __forceinline__ void conv_kloop_s3(const pmf_conv_desc_t& d, const ConvGeom& g, f32x16 (&acc)[MT][BN / 32],
                                              char* __restrict__ As, char* __restrict__ Bs, const int (&segrow)[MT],
                                              const int (&segcol)[MT], int tid, int li, int lh, int n, int n0, int ks,
                                              int oy0, int ox0, int& tri_) {
  constexpr int NT = BN / 32;
  constexpr int ASL = IS == 2 ? 10 : (SL > 1 ? 8 : (MT == 2 ? 7 : 5));   // float4 slots per thread for the input tile
  constexpr int NF = 5 * NT * 3;                  // fragments of the larger half (<= 5 virtual taps)
  constexpr int NDMA = (NF + 3) / 4;              // DMA instructions per wave per half
  const int in_cols = g.in_cols;
  const int sH = d.src[0].H, sW = d.src[0].W;
  const int q = tid & 3;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int npixA = g.in_rows * in_cols;
  const int totalA = npixA * 4 * SL;
  const int a_slab = g.a_floats * 4 / SL;         // bytes of one slab's tile
  const int nv = (NTAPS ? NTAPS : d.ntaps) * SL;  // virtual taps
  const int nt0 = (nv + 1) >> 1, nt1 = nv - nt0;  // ... of half 0 / half 1
  char* __restrict__ Bh1 = Bs + nt0 * NT * 3 * 1024;
  const int KS = g.Ktot >> 4, CT = d.ldw >> 5;
  int gA[ASL];
  unsigned okA = 0u;
#pragma unroll
  for (int j = 0; j < ASL; ++j) {
    const int f = tid + 256 * j, pix = SL > 1 ? (f >> 2) - pmf_fdiv(f >> 2, npixA, 1.f / (float)npixA) * npixA : (f >> 2);
    const int r = pmf_fdiv(pix, in_cols, 1.f / (float)in_cols), c = pix - r * in_cols;
    const int iy = oy0 * IS + g.dy_min + r, ix = ox0 * IS + g.dx_min + c;
    const bool ok = f < totalA && iy >= 0 && iy < sH && ix >= 0 && ix < sW;
    gA[j] = ok ? (n * sH + iy) * sW + ix : -1;
    okA |= ok ? (1u << j) : 0u;
  }
  TR();
  int aoff[TAPG];
  {
    int ty[TAPG], tx[TAPG];
#pragma unroll
    for (int t = 0; t < TAPG; ++t) { ty[t] = d.tdy[t]; tx[t] = d.tdx[t]; }
    PMF_SGPR_BATCH("s"(ty[0]), "s"(ty[1]), "s"(ty[2]), "s"(ty[3]), "s"(ty[4]), "s"(ty[5]), "s"(ty[6]), "s"(ty[7]),
                   "s"(ty[8]), "s"(tx[0]), "s"(tx[1]), "s"(tx[2]), "s"(tx[3]), "s"(tx[4]), "s"(tx[5]), "s"(tx[6]),
                   "s"(tx[7]), "s"(tx[8]));
#pragma unroll
    for (int v = 0; v < TAPG; ++v) {
      const int t = v / SL, sl = v % SL;            // compile-time after unrolling
      aoff[v] = v < nv ? ((ty[t] - g.dy_min) * in_cols + (tx[t] - g.dx_min)) * S3_APB + sl * a_slab : 0;
    }
    // the tap offsets are wave-uniform: left alone they sit in 9 SGPRs for the whole loop, and the kernel is short of
    // SGPRs (spills through v_readlane next to the MFMAs); as VGPRs they cost nothing that is scarce here
    if (NTAPS != 0) {
#pragma unroll
      for (int v = 0; v < TAPG; ++v) asm volatile("" : "+v"(aoff[v]));
    }
  }
  int abase[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) abase[m] = (segrow[m] * IS * in_cols + (segcol[m] * 32 + li) * IS) * S3_APB + lh * 16;

  int si = 0, c0 = 0, kb = 0, cn = 0;
  // ONE: the operand, once
  const float* o_x = nullptr; const float* o_sc = nullptr; const float* o_sh = nullptr; const float* o_cm = nullptr;
  int o_C = 0, o_ld = 0, o_fl = 0;
  if (ONE) {
    o_x = d.src[0].x; o_sc = d.src[0].scale; o_sh = d.src[0].shift; o_cm = d.src[0].cmul;
    o_C = d.src[0].C; o_ld = d.src[0].ldc; o_fl = d.src[0].flags;
    const int o_cl = d.src[0].cmul_ld;
    PMF_SGPR_BATCH("s"(o_x), "s"(o_sc), "s"(o_sh), "s"(o_cm), "s"(o_C), "s"(o_ld), "s"(o_fl), "s"(o_cl));
    if (o_cm) o_cm += (size_t)n * o_cl;
  }
  auto settle = [&]() {
    if (ONE) return c0 < o_C;
    for (;;) {
      if (si >= d.nsrc) return false;
      if (c0 >= d.src[si].C) { kb += d.src[si].C; ++si; c0 = 0; continue; }
      if ((cn % g.ksplit) == ks) return true;
      ++cn; c0 += KC * SL;
    }
  };
  f32x4 rA[ASL], sc4, sh4, cm4;
  int cur_flags = 0;
  bool cur_aff = false, cur_plain = false;
  __amdgpu_buffer_rsrc_t nrs;
  int nld = 0, ncch = 0;
  const float* cur_sc = nullptr; const float* cur_sh = nullptr; const float* cur_cm = nullptr;   // SL > 1: re-read at store time
  const char* __restrict__ nw = nullptr;   // fragment (tap 0, slab 0, plane 0) of the stage being fetched, first output tile
  const size_t tap_stride = (size_t)KS * CT * 3 * 1024, slab_stride = (size_t)CT * 3 * 1024;
  auto head = [&]() {
    if (ONE) {
      nrs = __builtin_amdgcn_make_buffer_rsrc((void*)o_x, 0, d.N * sH * sW * o_ld * 4, 0x00020000);
      nld = o_ld; ncch = c0 + q * 4;
      cur_flags = o_fl;
      cur_aff = o_sc != nullptr;
      cur_plain = !o_sc && !o_cm && !(o_fl & PMF_SRC_RELU);
      if (SL == 1) {
        sc4 = f32x4{1.f, 1.f, 1.f, 1.f}; sh4 = f32x4{0.f, 0.f, 0.f, 0.f}; cm4 = f32x4{1.f, 1.f, 1.f, 1.f};
        if (cur_aff) { sc4 = *(const f32x4*)(o_sc + ncch); sh4 = *(const f32x4*)(o_sh + ncch); }
        if (o_cm) cm4 = *(const f32x4*)(o_cm + ncch);
      } else {
        cur_sc = cur_aff ? o_sc + ncch : nullptr; cur_sh = cur_aff ? o_sh + ncch : nullptr;
        cur_cm = o_cm ? o_cm + ncch : nullptr;
      }
      nw = (const char*)d.w_s3 + ((size_t)(c0 >> 4) * CT + (n0 >> 5)) * 3 * 1024;
      return;
    }
    const float* sx = d.src[si].x;
    const float* ssc = d.src[si].scale;
    const float* ssh = d.src[si].shift;
    const float* scm = d.src[si].cmul;
    const int sld = d.src[si].ldc, sfl = d.src[si].flags, scl = d.src[si].cmul_ld;
    PMF_SGPR_BATCH("s"(sx), "s"(ssc), "s"(ssh), "s"(scm), "s"(sld), "s"(sfl), "s"(scl));
    nrs = __builtin_amdgcn_make_buffer_rsrc((void*)sx, 0, d.N * sH * sW * sld * 4, 0x00020000);
    nld = sld; ncch = c0 + q * 4;
    cur_flags = sfl;
    cur_aff = ssc != nullptr;
    cur_plain = !ssc && !scm && !(sfl & PMF_SRC_RELU);
    if (SL == 1) {
      sc4 = f32x4{1.f, 1.f, 1.f, 1.f}; sh4 = f32x4{0.f, 0.f, 0.f, 0.f}; cm4 = f32x4{1.f, 1.f, 1.f, 1.f};
      if (cur_aff) { sc4 = *(const f32x4*)(ssc + ncch); sh4 = *(const f32x4*)(ssh + ncch); }
      if (scm) cm4 = *(const f32x4*)(scm + (size_t)n * scl + ncch);
    } else {
      cur_sc = cur_aff ? ssc + ncch : nullptr; cur_sh = cur_aff ? ssh + ncch : nullptr;
      cur_cm = scm ? scm + (size_t)n * scl + ncch : nullptr;
    }
    nw = (const char*)d.w_s3 + ((size_t)((kb + c0) >> 4) * CT + (n0 >> 5)) * 3 * 1024;
  };
  auto loadA = [&](int j) {
    const int sch = SL > 1 ? ((tid + 256 * j) >> 2) / npixA * KC : 0;
    rA[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(nrs, (gA[j] * nld + ncch + sch) * 4, 0, 0));
  };
  // fragments ((v - va) NT + u) 3 + p of virtual taps [va, va + nth) -> dst, one 1-KiB DMA instruction each
  auto dma_half = [&](const char* __restrict__ wsrc, char* __restrict__ dst, int va, int nth) {
#pragma unroll
    for (int jj = 0; jj < NDMA; ++jj) {
      const int f = wave + 4 * jj;                 // wave-uniform
      if (f < nth * NT * 3) {
        const int vl = f / (NT * 3), up = f - vl * (NT * 3);
        const int v = va + vl, t = v / SL, sl = v % SL;
        __builtin_amdgcn_global_load_lds((const float*)(wsrc + (size_t)t * tap_stride + sl * slab_stride + up * 1024 + lane * 16),
                                         (lds_ptr_t)(dst + f * 1024), 16, 0, 0);
      }
    }
  };
  TR();
  bool have = settle();
  const char* __restrict__ wcur = nullptr;
  if (have) {
    head();
    TR();
#pragma unroll
    for (int j = 0; j < ASL; ++j) loadA(j);
    dma_half(nw, Bs, 0, nt0);
  }
  TR();
  const float* st_sc = nullptr; const float* st_sh = nullptr; const float* st_cm = nullptr;
  // Straight-line (no exec masking, no uniform branches): seven of these in a row interleave freely.  Out-of-image
  // pixels are zeroed AFTER the transform (zero padding of the transformed map); slots past the end of the tile write
  // to a per-thread scratch word pair instead of being masked off.
  char* const trash = Bs + nv * NT * 3 * 1024 + tid * 8;
  // PLAIN: the operand is a raw tensor (no BatchNorm view, no ReLU, no channel multiplier -- every input-gradient launch
  // reads dz this way): nothing to transform, and out-of-image slots already hold the 0 the buffer load returned
  auto storeA_impl = [&](char* __restrict__ dst, auto plain_c) {
    constexpr bool PLAIN = decltype(plain_c)::value;
    const float relu_lo = (cur_flags & PMF_SRC_RELU) ? 0.f : -__builtin_inff();
#pragma unroll
    for (int j = 0; j < ASL; ++j) {
      const int f = tid + 256 * j;
      const int sl = SL > 1 ? (f >> 2) / npixA : 0, pix = (f >> 2) - sl * npixA;
      f32x4 t = rA[j];
      if (!PLAIN) {
        if (SL == 1) {
          t = t * sc4 + sh4;
        } else if (st_sc) {
          t = t * *(const f32x4*)(st_sc + sl * KC) + *(const f32x4*)(st_sh + sl * KC);
        }
        t.x = s3_vmax(t.x, relu_lo); t.y = s3_vmax(t.y, relu_lo); t.z = s3_vmax(t.z, relu_lo); t.w = s3_vmax(t.w, relu_lo);
        if (SL == 1) t = t * cm4;
        else if (st_cm) t = t * *(const f32x4*)(st_cm + sl * KC);
        const bool ok = (okA >> j) & 1u;
        t.x = ok ? t.x : 0.f; t.y = ok ? t.y : 0.f; t.z = ok ? t.z : 0.f; t.w = ok ? t.w : 0.f;
      }
      unsigned l0, l1, l2, h0, h1, h2;
      s3_split2(t.x, t.y, l0, l1, l2);
      s3_split2(t.z, t.w, h0, h1, h2);
      char* o = f < totalA ? dst + sl * a_slab + pix * S3_APB + q * 8 : trash;
      *(u32x2*)(o) = u32x2{l0, h0};
      *(u32x2*)(o + (f < totalA ? 32 : 0)) = u32x2{l1, h1};
      *(u32x2*)(o + (f < totalA ? 64 : 0)) = u32x2{l2, h2};
    }
  };
  auto storeA = [&](char* __restrict__ dst) {
    if (cur_plain) storeA_impl(dst, std::true_type{});
    else storeA_impl(dst, std::false_type{});
  };
  auto fill = [&](int st, int ns) {
    constexpr int per = 2;
#pragma unroll
    for (int j = 0; j < ASL; ++j)
      if (j >= st * per && j < (st + 1) * per) loadA(j);
    if (st == ns - 1) {
#pragma unroll
      for (int j = 0; j < ASL; ++j)
        if (j >= ns * per) loadA(j);
    }
  };
  auto mfma_half = [&](const char* __restrict__ Bt, int t0, int nth, bool with_fill) {
#pragma unroll
    for (int m = 0; m < MT; ++m) asm volatile("" : "+v"(abase[m]));
    __builtin_amdgcn_sched_barrier(0);
    if (NTAPS != 0) {
      constexpr int NV = (NTAPS ? NTAPS : 1) * SL, N0 = (NV + 1) / 2, N1 = NV - N0;
      if (with_fill) s3_half<BN, MT, N0>(acc, As, Bt, abase, aoff, 0, lane, fill);
      else s3_half<BN, MT, (N1 > 0 ? N1 : 1)>(acc, As, Bt, abase, aoff, N0, lane);
      return;
    }
    if (with_fill) {
      if (nth == 5) s3_half<BN, MT, 5>(acc, As, Bt, abase, aoff, t0, lane, fill);
      else if (nth == 4) s3_half<BN, MT, 4>(acc, As, Bt, abase, aoff, t0, lane, fill);
      else if (nth == 3) s3_half<BN, MT, 3>(acc, As, Bt, abase, aoff, t0, lane, fill);
      else if (nth == 2) s3_half<BN, MT, 2>(acc, As, Bt, abase, aoff, t0, lane, fill);
      else s3_half<BN, MT, 1>(acc, As, Bt, abase, aoff, t0, lane, fill);
    } else {
      if (nth == 4) s3_half<BN, MT, 4>(acc, As, Bt, abase, aoff, t0, lane);
      else if (nth == 3) s3_half<BN, MT, 3>(acc, As, Bt, abase, aoff, t0, lane);
      else if (nth == 2) s3_half<BN, MT, 2>(acc, As, Bt, abase, aoff, t0, lane);
      else if (nth == 1) s3_half<BN, MT, 1>(acc, As, Bt, abase, aoff, t0, lane);
    }
  };
  while (have) {
    __syncthreads();                       // X: everyone finished the MFMAs of the previous chunk
    TR();
    if (SL > 1) { st_sc = cur_sc; st_sh = cur_sh; st_cm = cur_cm; }
    storeA(As);
    wcur = nw;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of B(half 0) has landed in LDS
    __syncthreads();                       // Y: input tile + half 0 visible
    TR();
    ++cn; c0 += KC * SL;
    have = settle();
    if (have) head();
    else nrs = __builtin_amdgcn_make_buffer_rsrc((void*)d.src[0].x, 0, 0, 0x00020000);
    if (nt1) dma_half(wcur, Bh1, nt0, nt1);
    mfma_half(Bs, 0, nt0, true);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // B(half 1) (and the next input tile) landed
    __syncthreads();                       // Z: everyone finished reading half 0
    TR();
    if (have) dma_half(nw, Bs, 0, nt0);
    if (nt1) mfma_half(Bh1, nt0, nt1, false);
    TR();
  }
}

// PIPE 11 -- 1x1 convolutions on the split-bf16 path, activations straight from global memory.
// A 1x1 layer has no halo and no reuse of an input pixel across taps: staging its input tile through LDS buys nothing and
// costs three barriers per 16-channel stage around 6 MT NT MFMAs.  Here every weight fragment of the output-channel tile
// ([K/16][NT][3 planes] x 1 KiB, e.g. 72 KiB for 192 -> 64) is DMA'd into LDS ONCE, and then each wave runs free of
// barriers: lane (pixel li, half lh) loads channels 16 k + 8 lh .. + 7 of its pixel (two 16-byte buffer loads: exactly
// the A-operand layout of v_mfma_f32_32x32x16_bf16), applies the operand transform from an LDS table
// [K] x {scale, shift, relu floor, channel multiplier}, splits into three bf16 planes in registers and multiplies.
// PF k-steps of loads are in flight per wave; the split of step k + 1 is issued next to the MFMAs of step k.
// Host conditions: conv_direct_lds().
// MTAP (PIPE 13): the same loop over VIRTUAL k-steps v = tap * (K / 16) + k of a multi-tap convolution (2x2 / 3x3, any
// dilation, stride 1 or 2; <= 9 taps): the weight fragments are already packed tap-major ([tap][K/16][Cout/32][plane]), so
// the fragment index is v itself; a lane's pixel moves by (dy, dx) of the tap when the channel counter wraps; taps that fall
// outside the image address the buffer out of range (hardware zero) and -- for operands seen through a BatchNorm / ReLU /
// multiplier view, whose transform would turn that 0 into `shift` -- are zeroed again behind the transform (zero padding of
// the TRANSFORMED map).  No input tile in LDS, no barrier per stage; every tap re-reads its pixels through L1 / L2.
// Selected by the caller (pmf_conv_desc_t.cfg bit 24: the plan autotuner tries it next to the LDS-staged loop).
// MODE 2 (PIPE 14, the stem class: ONE operand of 8 padded channels, many taps -- the 7x7 RGB stem): a 16-deep MFMA step holds
// the 8 channels of TWO taps; lane (pixel, half) loads the 32 bytes of its pixel shifted by tap 2 v + half, which is
// exactly its A fragment.  Weights: pmf_pack_job_t format 2 (K index = tap * 8 + channel).
template <int BN, int MT, int MODE = 0>
__device__ __forceinline__ void conv_kloop_direct(const pmf_conv_desc_t& d, const ConvGeom& g, f32x16 (&acc)[MT][BN / 32],
                                                  char* __restrict__ Bs, const int (&segrow)[MT], const int (&segcol)[MT],
                                                  int tid, int li, int lh, int n, int n0, int oy0, int ox0) {
  constexpr int NT = BN / 32;
  constexpr int PF = 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  constexpr bool MTAP = MODE != 0, HALF = MODE == 2;
  const int Ktot = g.Ktot, KS = Ktot >> 4, nks = HALF ? (d.ntaps + 1) >> 1 : (MTAP ? KS * d.ntaps : KS), CT = d.ldw >> 5;
  const int is = d.in_stride, sH = d.src[0].H, sW = d.src[0].W;
  // weights: every fragment of this output-channel tile resident in LDS (kchunk 0), or streamed in chunks of kchunk
  // 16-channel steps through two buffers: chunk c + 1 is DMA'd while chunk c is multiplied, one wait + barrier per chunk
  // (layers whose fragments would leave room for only one workgroup per CU)
  const int kch = g.kchunk;
  const int nres = kch ? kch : nks;                    // steps per buffer
  const int bufbytes = nres * NT * 3 * 1024;
  auto dma_chunk = [&](int c, char* __restrict__ dst) {
    const int k0 = c * nres;
    const int nf = min(nks - k0, nres) * NT * 3;
    const char* wsrc = (const char*)d.w_s3 + (size_t)(n0 >> 5) * 3 * 1024 + lane * 16;
    for (int f = wave; f < nf; f += 4) {
      const int k16 = f / (NT * 3), up = f - k16 * (NT * 3);
      __builtin_amdgcn_global_load_lds((const float*)(wsrc + ((size_t)(k0 + k16) * CT * 3 + up) * 1024), (lds_ptr_t)(dst + f * 1024), 16, 0, 0);
    }
  };
  dma_chunk(0, Bs);
  const int nfrag = (kch ? 2 : 1) * nres * NT * 3;     // (fragment slots ahead of the operand table)
  bool plain = true;
  for (int i = 0; i < d.nsrc; ++i)
    plain = plain && !d.src[i].scale && !d.src[i].cmul && !(d.src[i].flags & PMF_SRC_RELU);
  float* __restrict__ tab = (float*)(Bs + nfrag * 1024);   // [4][Ktot]
  if (!plain) {
    for (int k = tid; k < Ktot; k += 256) {
      int si = 0, c = k;
      while (c >= d.src[si].C) { c -= d.src[si].C; ++si; }
      const float* ssc = d.src[si].scale;
      const float* scm = d.src[si].cmul;
      tab[k] = ssc ? ssc[c] : 1.f;
      tab[Ktot + k] = ssc ? d.src[si].shift[c] : 0.f;
      tab[2 * Ktot + k] = (d.src[si].flags & PMF_SRC_RELU) ? 0.f : -__builtin_inff();
      tab[3 * Ktot + k] = scm ? scm[(size_t)n * d.src[si].cmul_ld + c] : 1.f;
    }
  }
  // ---- load stream: (tap, source, channel) of the next k-step to fetch
  int pix[MT];
  unsigned okcur = 0u;                 // bit m: the current tap of segment m lies inside the image
  int ltap = 0;
  auto set_tap = [&](int t) {
    int ty, tx;
    bool tap_ok = true;
    if (HALF) {                      // step t: taps 2 t (lower half wave) and 2 t + 1 (upper half)
      const int t0 = 2 * t, t1 = min(2 * t + 1, d.ntaps - 1);
      const int y0 = (int)d.tdy[t0], x0 = (int)d.tdx[t0], y1 = (int)d.tdy[t1], x1 = (int)d.tdx[t1];
      ty = lh ? y1 : y0; tx = lh ? x1 : x0;
      tap_ok = 2 * t + lh < d.ntaps;
    } else {
      ty = (int)d.tdy[t]; tx = (int)d.tdx[t];
    }
    okcur = 0u;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int oy = oy0 + segrow[m], ox = ox0 + segcol[m] * 32 + li;
      const int iy = oy * is + ty, ix = ox * is + tx;
      const bool ok = tap_ok && oy < d.OH && ox < d.OW && iy >= 0 && iy < sH && ix >= 0 && ix < sW;
      pix[m] = ok ? (n * sH + iy) * sW + ix : -1;
      okcur |= ok ? (1u << m) : 0u;
    }
  };
  set_tap(0);
  int lsi = 0, lc0 = 0, lC = 0;
  unsigned lbase[MT];
  __amdgpu_buffer_rsrc_t lrs;
  auto lhead = [&]() {
    if (lsi < d.nsrc) {
      const float* sx = d.src[lsi].x;
      const int sld = d.src[lsi].ldc, sC = d.src[lsi].C;
      PMF_SGPR_BATCH("s"(sx), "s"(sld), "s"(sC));
      lrs = __builtin_amdgcn_make_buffer_rsrc((void*)sx, 0, d.N * sH * sW * sld * 4, 0x00020000);
      lC = sC;
#pragma unroll
      for (int m = 0; m < MT; ++m) lbase[m] = pix[m] >= 0 ? (unsigned)(pix[m] * sld * 4 + (HALF ? 0 : lh * 32)) : 0x80000000u;
    } else {          // past the last k-step: the range check returns zeros without touching memory
      lrs = __builtin_amdgcn_make_buffer_rsrc((void*)d.src[0].x, 0, 0, 0x00020000);
      lC = 1 << 30;
    }
  };
  f32x4 raw[PF][MT][2];
  unsigned okslot[PF] = {0u, 0u, 0u, 0u};
  auto issue = [&](auto slot_c) {
    constexpr int j = decltype(slot_c)::value;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      raw[j][m][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(lrs, lbase[m] + lc0 * 4, 0, 0));
      raw[j][m][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(lrs, lbase[m] + lc0 * 4 + 16, 0, 0));
    }
    if (MTAP) okslot[j] = okcur;
    if (HALF) {                      // the 8 channels are one load pair: every step moves to the next two taps
      ++ltap;
      if (ltap < nks) { set_tap(ltap); } else { lsi = d.nsrc; }
      lhead();
      return;
    }
    lc0 += 16;
    if (lc0 >= lC) {
      ++lsi; lc0 = 0;
      if (MTAP && lsi >= d.nsrc && ltap + 1 < d.ntaps) { ++ltap; lsi = 0; set_tap(ltap); }   // next tap: same channels
      lhead();
    }
  };
  lhead();
  issue(std::integral_constant<int, 0>{});
  issue(std::integral_constant<int, 1>{});
  issue(std::integral_constant<int, 2>{});
  issue(std::integral_constant<int, 3>{});
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PF * MT * 2) : "memory");   // the weight DMA (older than the 4 prefetches) landed
  __syncthreads();
  const char* bp = Bs + lane * 16;
  // transform + split of the 8 channels this lane holds of k-step kk
  auto prep = [&](auto slot_c, int kk, bf16x8 (&a)[MT][3]) {
    constexpr int j = decltype(slot_c)::value;
    f32x4 sc[2], sh[2], lo[2], cm[2];
    if (!plain) {
      const int kc = HALF ? 0 : (MTAP ? kk - (kk / KS) * KS : kk);       // channel step inside the tap
      const float* t0 = tab + (HALF ? 0 : kc * 16 + lh * 8);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        sc[h] = *(const f32x4*)(t0 + h * 4); sh[h] = *(const f32x4*)(t0 + Ktot + h * 4);
        lo[h] = *(const f32x4*)(t0 + 2 * Ktot + h * 4); cm[h] = *(const f32x4*)(t0 + 3 * Ktot + h * 4);
      }
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      u32x2 p0[2], p1[2], p2[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        f32x4 t = raw[j][m][h];
        if (!plain) {
          t = t * sc[h] + sh[h];
          t.x = s3_vmax(t.x, lo[h].x); t.y = s3_vmax(t.y, lo[h].y); t.z = s3_vmax(t.z, lo[h].z); t.w = s3_vmax(t.w, lo[h].w);
          t = t * cm[h];
          if (MTAP) {           // zero padding of the transformed map
            const bool ok = (okslot[j] >> m) & 1u;
            t.x = ok ? t.x : 0.f; t.y = ok ? t.y : 0.f; t.z = ok ? t.z : 0.f; t.w = ok ? t.w : 0.f;
          }
        }
        unsigned a0, a1, a2, b0, b1, b2;
        s3_split2(t.x, t.y, a0, a1, a2);
        s3_split2(t.z, t.w, b0, b1, b2);
        p0[h] = u32x2{a0, b0}; p1[h] = u32x2{a1, b1}; p2[h] = u32x2{a2, b2};
      }
      typedef __attribute__((ext_vector_type(4))) unsigned u32x4_;
      a[m][0] = __builtin_bit_cast(bf16x8, u32x4_{p0[0].x, p0[0].y, p0[1].x, p0[1].y});
      a[m][1] = __builtin_bit_cast(bf16x8, u32x4_{p1[0].x, p1[0].y, p1[1].x, p1[1].y});
      a[m][2] = __builtin_bit_cast(bf16x8, u32x4_{p2[0].x, p2[0].y, p2[1].x, p2[1].y});
    }
  };
  auto mma = [&](int kk, const bf16x8 (&a)[MT][3]) {
    bf16x8 b[NT][3];
#pragma unroll
    for (int u = 0; u < NT; ++u)
#pragma unroll
      for (int p = 0; p < 3; ++p) b[u][p] = *(const bf16x8*)(bp + ((kk * NT + u) * 3 + p) * 1024);
    constexpr int PA[6] = {0, 1, 2, 0, 1, 0}, PB[6] = {2, 1, 0, 1, 0, 0};
#pragma unroll
    for (int pr = 0; pr < 6; ++pr)
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int u = 0; u < NT; ++u)
          acc[m][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m][PA[pr]], b[u][PB[pr]], acc[m][u], 0, 0, 0);
  };
  bf16x8 a0[MT][3], a1[MT][3];
  prep(std::integral_constant<int, 0>{}, 0, a0);
  // step kk (slot kk % 4): refill its slot for step kk + 4, split step kk + 1, multiply step kk
  auto quad = [&](int kk, auto guard_c) {
    constexpr bool G = decltype(guard_c)::value;
    issue(std::integral_constant<int, 0>{});
    prep(std::integral_constant<int, 1>{}, kk + 1, a1);
    if (!G || kk < nks) mma(kk, a0);
    issue(std::integral_constant<int, 1>{});
    prep(std::integral_constant<int, 2>{}, kk + 2, a0);
    if (!G || kk + 1 < nks) mma(kk + 1, a1);
    issue(std::integral_constant<int, 2>{});
    prep(std::integral_constant<int, 3>{}, kk + 3, a1);
    if (!G || kk + 2 < nks) mma(kk + 2, a0);
    issue(std::integral_constant<int, 3>{});
    prep(std::integral_constant<int, 0>{}, kk + 4, a0);
    if (!G || kk + 3 < nks) mma(kk + 3, a1);
  };
  int kk = 0;
  for (int c = 0; c * nres < nks; ++c) {
    const int kend = min(nks, (c + 1) * nres);
    if (kch) {
      // buffer (c + 1) & 1 was last read in chunk c - 1, and every wave has passed the barrier behind that chunk
      if (kend < nks) dma_chunk(c + 1, Bs + ((c + 1) & 1) * bufbytes);
      bp = Bs + (c & 1) * bufbytes + lane * 16 - (size_t)c * bufbytes;     // mma() indexes by the absolute step
    }
    for (; kk + PF <= kend; kk += PF) quad(kk, std::false_type{});
    if (kk < kend) { quad(kk, std::true_type{}); kk = kend; }
    if (kch && kend < nks) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's share of chunk c + 1 has landed ...
      __syncthreads();                                       // ... everyone's; and everyone is done with chunk c
    }
  }
}

// PIPE: 0 generic K loop, 1 pipelined, 4 pipelined with 64-channel stages (1x1 convs).
// Measured and rejected on this loop (kept out of the code): a second input tile in LDS (two barriers per chunk instead
// of three: 49.2 vs 47.8 us on 64->64 3x3 at 32x1024, 23.60 vs 23.23 ms per training step); a start delay for the
// workgroup in the odd wave slots (de-phasing the co-resident pair: monotonically slower, 47.6 -> 50.2 us at 16k cycles);
// a 512-thread "paired" form with two pixel tiles per workgroup whose MFMA / staging phases are complementary by
// construction (one group multiplies while the other stages; shared, double-buffered weight slabs: 53.3 vs 47.3 us,
// 24.13 vs 23.18 ms per step).  Two waves per SIMD that interleave freely fill each other's gaps better than any
// enforced schedule here; what did help is placing the next step's LDS reads inside the MFMA gaps (pmf_sgb_seq).
template <int BN, int MT, int PIPE>
__global__ __launch_bounds__(256) void conv_fwd_k(const pmf_conv_desc_t d, const ConvGeom g) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  {  // everything the prologue reads from the two argument structs, as ONE scalar-cache batch (see PMF_SGPR_BATCH)
    PMF_SGPR_BATCH("s"(d.N), "s"(d.OH), "s"(d.OW), "s"(d.nsrc), "s"(d.ntaps), "s"(d.in_stride), "s"(d.w), "s"(d.ldw),
                   "s"(d.src[0].C), "s"(d.src[0].H), "s"(d.src[0].W), "s"(g.segs_x_log2), "s"(g.th), "s"(g.tw),
                   "s"(g.tiles_x), "s"(g.in_rows), "s"(g.in_cols), "s"(g.dy_min), "s"(g.dx_min), "s"(g.Ktot),
                   "s"(g.kc_alloc), "s"(g.a_floats), "s"(g.ksplit));
  }
  float* __restrict__ As = smem;
  float* __restrict__ Bs = smem + g.a_floats * ((PIPE > 1 && PIPE < 5) ? PIPE : 1);
  constexpr int NT = BN / 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  // XCD-aware tile order: the dispatcher deals consecutive workgroup ids round-robin to the 8 XCDs (each with its own
  // L2).  Re-number so that one XCD gets a CONTIGUOUS range of (tile, sample) for a fixed (output-channel tile, K
  // split): neighbouring tiles share their halo and all of them share one weight slab in that XCD's L2, instead of
  // every L2 holding every slab (matters for the low-resolution layers, whose weights are 2-20 MB).
  unsigned lin = blockIdx.x + gridDim.x * (blockIdx.z + gridDim.z * blockIdx.y);
  {
    const unsigned total = gridDim.x * gridDim.y * gridDim.z;
    if ((total & 7u) == 0u) lin = (lin & 7u) * (total >> 3) + (lin >> 3);
  }
  int tile, bz, by;
  if constexpr (PIPE == 11 || PIPE == 13 || PIPE == 14) {
    // no input tile in LDS to share: the output-channel tiles of one pixel tile run back to back on one XCD, so the
    // activations come from HBM once and from that XCD's L2 for the other tiles
    by = lin % gridDim.y;
    const unsigned lin_r = lin / gridDim.y;
    tile = lin_r % gridDim.x; bz = lin_r / gridDim.x;
  } else {
    tile = lin % gridDim.x;
    const unsigned lin_r = lin / gridDim.x;
    bz = lin_r % gridDim.z; by = lin_r / gridDim.z;
  }
  const int tx = tile % g.tiles_x, ty = tile / g.tiles_x;
  const int n = bz, n0 = (by / g.ksplit) * BN, ks = by % g.ksplit;
  const int oy0 = ty * g.th, ox0 = tx * g.tw;
  const int is = d.in_stride;
  const int in_cols = g.in_cols;
  const int kca = g.kc_alloc;
  int tri_ = 0;
  TR_START();
  TR();

  f32x16 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][t][r] = 0.f;

  int segrow[MT], segcol[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    int s = wave * MT + m;
    segrow[m] = s >> g.segs_x_log2;
    segcol[m] = s & ((1 << g.segs_x_log2) - 1);
  }

  if constexpr (PIPE == 12) {         // stride-2 3x3 (one slab per stage, 9 taps at compile time, 128-pixel tiles only)
    if constexpr (MT == 1)
      conv_kloop_s3<BN, 1, 1, 9, 2>(d, g, acc, (char*)smem, (char*)(smem + g.a_floats), segrow, segcol, tid, li, lh, n, n0, ks, oy0, ox0, tri_);
  } else if constexpr (PIPE == 11) {  // 1x1, split-bf16, activations straight from global memory
    conv_kloop_direct<BN, MT>(d, g, acc, (char*)smem, segrow, segcol, tid, li, lh, n, n0, oy0, ox0);
  } else if constexpr (PIPE == 13) {  // the same for 2 .. 9 taps (virtual k-steps)
    conv_kloop_direct<BN, MT, 1>(d, g, acc, (char*)smem, segrow, segcol, tid, li, lh, n, n0, oy0, ox0);
  } else if constexpr (PIPE == 14) {  // stem class: 8 padded channels, two taps per MFMA step
    conv_kloop_direct<BN, MT, 2>(d, g, acc, (char*)smem, segrow, segcol, tid, li, lh, n, n0, oy0, ox0);
  } else if constexpr (PIPE == 8) {   // one slab per stage, 9 taps at compile time
    if (g.one)
      conv_kloop_s3<BN, MT, 1, 9, 1, true>(d, g, acc, (char*)smem, (char*)(smem + g.a_floats), segrow, segcol, tid, li, lh, n, n0, ks, oy0, ox0, tri_);
    else
      conv_kloop_s3<BN, MT, 1, 9>(d, g, acc, (char*)smem, (char*)(smem + g.a_floats), segrow, segcol, tid, li, lh, n, n0, ks, oy0, ox0, tri_);
  } else if constexpr (PIPE == 10) {  // two slabs per stage, 4 taps at compile time (the 2x2 dilated layers)
    if (g.one)
      conv_kloop_s3<BN, MT, 2, 4, 1, true>(d, g, acc, (char*)smem, (char*)(smem + g.a_floats), segrow, segcol, tid, li, lh, n, n0, ks, oy0, ox0, tri_);
    else
      conv_kloop_s3<BN, MT, 2, 4>(d, g, acc, (char*)smem, (char*)(smem + g.a_floats), segrow, segcol, tid, li, lh, n, n0, ks, oy0, ox0, tri_);
  } else if constexpr (PIPE >= 5) {          // 5, 6, 7: 1, 2, 4 slabs per stage, tap count from the descriptor
    if (g.one)
      conv_kloop_s3<BN, MT, (1 << (PIPE - 5)), 0, 1, true>(d, g, acc, (char*)smem, (char*)(smem + g.a_floats), segrow, segcol, tid, li, lh, n, n0, ks, oy0, ox0, tri_);
    else
      conv_kloop_s3<BN, MT, (1 << (PIPE - 5))>(d, g, acc, (char*)smem, (char*)(smem + g.a_floats), segrow, segcol, tid, li, lh, n, n0, ks, oy0, ox0, tri_);
  } else if constexpr (PIPE != 0) {
    conv_kloop_pipe<BN, MT, (PIPE > 1 ? PIPE : 1)>(d, g, acc, As, Bs, segrow, segcol, tid, li, lh, n, n0, ks, oy0, ox0, tri_);
  } else {
  const int ngroups = d.gather ? d.ntaps : 1;
  int k_base = 0, chunk_no = 0;
  // LDS offsets of the taps of one weight sub-stage, relative to the tile origin (gather mode: always 0).
  // Read from the kernel arguments ONCE when all taps fit one sub-stage (every conv but the 7x7 stem).
  int aoff[TAPG];
  const bool aoff_static = !d.gather && d.ntaps <= TAPG;
#pragma unroll
  for (int t = 0; t < TAPG; ++t)
    aoff[t] = (aoff_static && t < d.ntaps) ? (((int)d.tdy[t] - g.dy_min) * in_cols + ((int)d.tdx[t] - g.dx_min)) * APITCH : 0;
  for (int si = 0; si < d.nsrc; ++si) {
    const float* __restrict__ sx = d.src[si].x;
    const float* __restrict__ sscale = d.src[si].scale;
    const float* __restrict__ sshift = d.src[si].shift;
    const float* __restrict__ scm = d.src[si].cmul ? d.src[si].cmul + (size_t)n * d.src[si].cmul_ld : nullptr;
    const int sC = d.src[si].C, sld = d.src[si].ldc, sflags = d.src[si].flags;
    const bool bc = (sflags & PMF_SRC_BCAST) != 0;
    const int sH = bc ? d.OH * is : d.src[si].H, sW = bc ? d.OW * is : d.src[si].W;
    for (int c0 = 0; c0 < sC; c0 += KC) {
      if ((chunk_no++ % g.ksplit) != ks) continue;   // split-K: chunks are dealt round-robin
      const int kc = min(KC, sC - c0);
      const int nql = kc == 16 ? 2 : 1;   // log2(float4 per pixel)
      const int kcl = kc == 16 ? 4 : 3;   // log2(kc)
      for (int grp = 0; grp < ngroups; ++grp) {
        const int gt0 = d.gather ? grp : 0;
        const int gnt = d.gather ? 1 : d.ntaps;
        const int gy0 = d.gather ? (int)d.tdy[grp] : g.dy_min;
        const int gx0 = d.gather ? (int)d.tdx[grp] : g.dx_min;
        __syncthreads();
        {  // ---- stage the input tile (with halo): issue a batch of independent global loads, then transform +
           // write to LDS (a load -> wait -> store loop would expose one HBM round trip per 16 bytes)
          constexpr int AB = 4;
          const int total = (g.in_rows * in_cols) << nql;
          const int q = tid & ((1 << nql) - 1);            // 256 % (float4 per pixel) == 0: q is loop-invariant
          const int cch = c0 + q * 4;
          f32x4 sc4 = {1.f, 1.f, 1.f, 1.f}, sh4 = {0.f, 0.f, 0.f, 0.f}, cm4 = {1.f, 1.f, 1.f, 1.f};
          if (sscale) { sc4 = *(const f32x4*)(sscale + cch); sh4 = *(const f32x4*)(sshift + cch); }
          if (scm) cm4 = *(const f32x4*)(scm + cch);
          for (int base = 0; base < total; base += 256 * AB) {
            f32x4 v[AB];
            bool ok[AB];
#pragma unroll
            for (int j = 0; j < AB; ++j) {
              const int f = base + tid + 256 * j;
              const int pix = f >> nql;
              const int r = pix / in_cols, c = pix - r * in_cols;
              const int iy = oy0 * is + gy0 + r, ix = ox0 * is + gx0 + c;
              ok[j] = f < total && iy >= 0 && iy < sH && ix >= 0 && ix < sW;
              if (ok[j]) {
                const size_t off = bc ? (size_t)n * sld + cch : ((size_t)(n * sH + iy) * sW + ix) * sld + cch;
                v[j] = *(const f32x4*)(sx + off);
              }
            }
#pragma unroll
            for (int j = 0; j < AB; ++j) {
              const int f = base + tid + 256 * j;
              if (f < total) {
                f32x4 t = {0.f, 0.f, 0.f, 0.f};
                if (ok[j]) {
                  t = v[j];
                  if (sscale) t = t * sc4 + sh4;
                  if (sflags & PMF_SRC_RELU) {
                    t.x = fmaxf(t.x, 0.f); t.y = fmaxf(t.y, 0.f); t.z = fmaxf(t.z, 0.f); t.w = fmaxf(t.w, 0.f);
                  }
                  t = t * cm4;
                }
                *(f32x4*)(As + (f >> nql) * APITCH + q * 4) = t;
              }
            }
          }
        }
        for (int sub = 0; sub < gnt; sub += g.tap_group) {
          const int snt = min(g.tap_group, gnt - sub);
          if (sub) __syncthreads();
          {  // ---- stage the weight slab [snt][kc][BN] (batched loads, as above)
            constexpr int rowq = BN / 4;
            constexpr int BB = 5;
            const int totalB = snt * kc * rowq;
            for (int base = 0; base < totalB; base += 256 * BB) {
              f32x4 v[BB];
#pragma unroll
              for (int j = 0; j < BB; ++j) {
                const int f = base + tid + 256 * j;
                if (f < totalB) {
                  const int row = f / rowq, qq = f - row * rowq;
                  const int tl = row >> kcl, kk = row & (kc - 1);
                  v[j] = *(const f32x4*)(d.w + ((size_t)(gt0 + sub + tl) * g.Ktot + k_base + c0 + kk) * d.ldw + n0 + qq * 4);
                }
              }
#pragma unroll
              for (int j = 0; j < BB; ++j) {
                const int f = base + tid + 256 * j;
                if (f < totalB) {
                  const int row = f / rowq, qq = f - row * rowq;
                  const int tl = row >> kcl, kk = row & (kc - 1);
                  *(f32x4*)(Bs + (tl * kca + kk) * BN + qq * 4) = v[j];
                }
              }
            }
          }
          if (!aoff_static && !d.gather) {
#pragma unroll
            for (int t = 0; t < TAPG; ++t) {
              const int tt = gt0 + sub + (t < snt ? t : 0);
              aoff[t] = (((int)d.tdy[tt] - gy0) * in_cols + ((int)d.tdx[tt] - gx0)) * APITCH;
            }
          }
          __syncthreads();
          int abase[MT];
#pragma unroll
          for (int m = 0; m < MT; ++m)
            abase[m] = ((segrow[m] * is) * in_cols + (segcol[m] * 32 + li) * is) * APITCH + lh * 4;
          if (kc == 16 && snt == 9) conv_steps<BN, MT, 9>(acc, As, Bs, abase, aoff, kca, li, lh);
          else if (kc == 16 && snt == 4) conv_steps<BN, MT, 4>(acc, As, Bs, abase, aoff, kca, li, lh);
          else if (kc == 16 && snt == 1) conv_steps<BN, MT, 1>(acc, As, Bs, abase, aoff, kca, li, lh);
          else {   // ragged chunks (8 channels) / tap groups: plain loop
#pragma unroll
            for (int tl = 0; tl < TAPG; ++tl) {
              if (tl < snt) {
                const float* bp = Bs + (tl * kca + lh * 4) * BN + li;
                for (int kg = 0; kg < kc; kg += 8) {
                  f32x4 a[MT];
                  float b[NT][4];
#pragma unroll
                  for (int m = 0; m < MT; ++m) a[m] = *(const f32x4*)(As + abase[m] + aoff[tl] + kg);
#pragma unroll
                  for (int u = 0; u < NT; ++u)
#pragma unroll
                    for (int q4 = 0; q4 < 4; ++q4) b[u][q4] = bp[(kg + q4) * BN + u * 32];
#pragma unroll
                  for (int q4 = 0; q4 < 4; ++q4)
#pragma unroll
                    for (int m = 0; m < MT; ++m)
#pragma unroll
                      for (int u = 0; u < NT; ++u)
                        acc[m][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m][q4], b[u][q4], acc[m][u], 0, 0, 0);
                }
              }
            }
          }
        }
      }
    }
    k_base += sC;
  }
  }  // !PIPE

  // ---- epilogue (conv_epi.h)
#ifdef PMF_CONV_TRACE
  conv_epilogue<BN, MT>(d, g, acc, segrow, segcol, n, n0, ks, oy0, ox0, tile, smem, tri_, tr_w0_);
#else
  conv_epilogue<BN, MT>(d, g, acc, segrow, segcol, n, n0, ks, oy0, ox0, tile, smem, tri_);
#endif
}

// Deterministic split-K tail: out = ep( act( sum_ks ws[ks] + bias ) ), optional BatchNorm statistics.
__global__ __launch_bounds__(256) void conv_finish_k(const pmf_conv_desc_t d, int ksplit, const float* __restrict__ ws, int ws_ld, int Q) {
  __shared__ double sh[2][256][4];
  const int Qm = Q < 256 ? Q : 256, Qg = min(Q - (int)blockIdx.y * 256, 256), rows = 256 / Qm;
  const int row = threadIdx.x / Qm, cql = threadIdx.x - row * Qm;
  const bool active = cql < Qg;
  const int c = ((int)blockIdx.y * 256 + cql) * 4;
  const int64_t npix = (int64_t)d.N * d.OH * d.OW, hw = (int64_t)d.OH * d.OW;
  double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
  if (active) {
    f32x4 bias = {0.f, 0.f, 0.f, 0.f};
    if (d.bias) {
#pragma unroll
      for (int k = 0; k < 4; ++k) if (c + k < d.Cout) bias[k] = d.bias[c + k];
    }
    // PP pixels x 8 slabs of independent loads in flight (a load -> add loop exposes one L2 round trip per slab and
    // per pixel: 8 round trips on a 16-way split with 4 pixels per thread).  Every pixel is still summed in slab order
    // and the statistics still accumulate in pixel order: the result does not depend on the batching.
    constexpr int PP = 4;
    const int64_t pstride = (int64_t)gridDim.x * rows;
    for (int64_t p0 = (int64_t)blockIdx.x * rows + row; p0 < npix; p0 += pstride * PP) {
      f32x4 v[PP];
#pragma unroll
      for (int i = 0; i < PP; ++i) v[i] = bias;
      for (int s0 = 0; s0 < ksplit; s0 += 8) {
        f32x4 t[PP][8];
#pragma unroll
        for (int i = 0; i < PP; ++i)
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (s0 + j < ksplit && p0 + i * pstride < npix)
              t[i][j] = *(const f32x4*)(ws + ((int64_t)(s0 + j) * npix + p0 + i * pstride) * ws_ld + c);
#pragma unroll
        for (int i = 0; i < PP; ++i)
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (s0 + j < ksplit && p0 + i * pstride < npix) v[i] += t[i][j];
      }
#pragma unroll
      for (int i = 0; i < PP; ++i) {
        const int64_t p = p0 + i * pstride;
        if (p >= npix) break;
        const int n = (int)(p / hw);
        const int rem = (int)(p - (int64_t)n * hw), oy = rem / d.OW, ox = rem - oy * d.OW;
        // strided / offset outputs (stride-2 input-gradient parity classes, pixel-shuffle style scatter)
        const int64_t opix = (int64_t)(n * d.out_H + oy * d.out_sy + d.out_oy) * d.out_W + ox * d.out_sx + d.out_ox;
        float* op = d.out + opix * d.out_ldc + c;
        const bool vec = c + 3 < d.Cout && !d.accumulate && ((uintptr_t)op & 15) == 0;   // one 16-byte store
        f32x4 xo;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (c + k >= d.Cout) continue;
          float x = pmf_act(v[i][k], d.act);
          if (d.ep_cmul) x *= d.ep_cmul[(size_t)n * d.ep_cmul_ld + c + k];
          if (d.ep_pmask) x *= d.ep_pmask[opix];
          float xraw = 0.f;
          if (d.ep_relu_x) {
            float xr = xraw = d.ep_relu_x[opix * d.ep_relu_ldc + c + k];
            if (d.ep_relu_scale) xr = xr * d.ep_relu_scale[c + k] + d.ep_relu_shift[c + k];
            if (!(xr > 0.f) && !(d.ep_flags & PMF_EP_STAT_X_ONLY)) x = 0.f;
          }
          x += d.accumulate ? op[k] : 0.f;     // (+ 0: a -0 leaves as +0, as from the epilogue of conv_epi.h)
          if (vec) xo[k] = x; else op[k] = x;
          s1[k] += (double)x;
          s2[k] += (double)x * (double)(d.ep_stat_mean ? xraw - d.ep_stat_mean[c + k] : x);
        }
        if (vec) *(f32x4*)op = xo;
      }
    }
  }
  if (d.stats) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { sh[0][row * Qm + cql][k] = s1[k]; sh[1][row * Qm + cql][k] = s2[k]; }
    __syncthreads();
    if (row == 0 && active) {
      for (int r = 1; r < rows; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) { s1[k] += sh[0][r * Qm + cql][k]; s2[k] += sh[1][r * Qm + cql][k]; }
      double* srow = d.stats + (size_t)blockIdx.x * 2 * d.Cout;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (c + k < d.Cout) { srow[c + k] = s1[k]; srow[d.Cout + c + k] = s2[k]; }
    }
  }
}

static int floor_log2(int v) { int l = 0; while ((2 << l) <= v) ++l; return l; }

// Chooses tile shape / staging mode; returns LDS bytes (or <0).
int pmf_conv_geometry(int OH, int OW, int ntaps, const int8_t* tdy, const int8_t* tdx, int in_stride, int gather_req,
                      int BN, int MT, int kc_alloc, ConvGeom* g, int* gather_out) {
  const int nseg = 4 * MT;
  // narrowest tile whose row count does not exceed (pow2-rounded) OH
  int sx = 1;
  while (sx < nseg && (nseg / sx) > OH) sx <<= 1;
  while (sx > 1 && (sx / 2) * 32 >= OW && (nseg / (sx / 2)) <= OH) sx >>= 1;
  g->segs_x_log2 = floor_log2(sx);
  g->th = nseg / sx;
  g->tw = 32 * sx;
  g->tiles_x = cdiv(OW, g->tw);
  g->tiles_y = cdiv(OH, g->th);
  int dy_min = 127, dy_max = -127, dx_min = 127, dx_max = -127;
  for (int t = 0; t < ntaps; ++t) {
    dy_min = tdy[t] < dy_min ? tdy[t] : dy_min; dy_max = tdy[t] > dy_max ? tdy[t] : dy_max;
    dx_min = tdx[t] < dx_min ? tdx[t] : dx_min; dx_max = tdx[t] > dx_max ? tdx[t] : dx_max;
  }
  g->dy_min = dy_min; g->dx_min = dx_min;
  g->kc_alloc = kc_alloc;
  int gather = gather_req;
  for (;;) {
    int rows = (g->th - 1) * in_stride + 1, cols = (g->tw - 1) * in_stride + 1;
    if (!gather) { rows += dy_max - dy_min; cols += dx_max - dx_min; }
    g->in_rows = rows; g->in_cols = cols;
    g->a_floats = round_up(rows * cols * APITCH, 4);
    g->tap_group = gather ? 1 : (ntaps < TAPG ? ntaps : TAPG);
    int lds = (g->a_floats + g->tap_group * kc_alloc * BN) * 4;
    if (lds < 2 * 4 * 64 * 2 * 8) lds = 2 * 4 * 64 * 2 * 8;  // room for the float64 stats reduction
    if (lds <= 150 * 1024 || gather) { *gather_out = gather; return lds; }
    gather = 1;
  }
}

static int finish_rows(const pmf_conv_desc_t* d, bool stats) {
  const int Q = round_up(d->Cout, 4) / 4, Qg = Q < 256 ? Q : 256, rows = 256 / Qg;
  // four pixels per thread row when the launch writes statistics rows (one per workgroup, read back by the BatchNorm
  // finalize), one otherwise
  int64_t gx = cdiv64((int64_t)d->N * d->OH * d->OW, (int64_t)rows * (stats ? 4 : 1));
  return (int)(gx > 1024 ? 1024 : (gx < 1 ? 1 : gx));
}

// the ticket array of the in-kernel combine holds one counter per output tile: PMF_SPLITK_TICKETS entries
#define PMF_SPLITK_TICKETS 16384

// deterministic split-K tail of a launch whose workgroups wrote g.ksplit partial slabs
static int pmf_conv_finish_launch(const pmf_conv_desc_t* d, const ConvGeom& g, hipStream_t s) {
  const int Q = g.ws_ld / 4, Qg = Q < 256 ? Q : 256, rows = 256 / Qg;
  const int gx = finish_rows(d, d->stats != nullptr);
  hipLaunchKernelGGL(conv_finish_k, dim3((unsigned)gx, (unsigned)cdiv(Q, 256), 1), dim3(rows * Qg), 0, s, *d, g.ksplit,
                     (const float*)g.ws, g.ws_ld, Q);
  PMF_LAUNCH_CHECK();
  return 0;
}

// multi-destination launches (pmf_conv_desc_t.ndst): every channel range starts on an output-channel tile
static int multi_tile(const pmf_conv_desc_t* d) {        // 64 / 32: the widest tile all ranges allow; 0: none
  int t = 64, sum = 0;
  for (int i = 0; i < d->ndst; ++i) {
    if (d->dst[i].C <= 0 || d->dst[i].C % 32) return 0;
    if (d->dst[i].C % 64) t = 32;
    sum += d->dst[i].C;
  }
  return sum == d->Cout ? t : 0;
}
extern "C" int pmf_conv_multi_ok(const pmf_conv_desc_t* d) {
  return d && d->ndst > 0 && d->ndst <= PMF_MAX_SRC && !d->bias && multi_tile(d) != 0;
}

// PMF_CONV_FORCE="BN,MT,KS" (tools/bench_conv.py sweeps; 0 = keep the heuristic), parsed once per call
struct ConvForce { int bn, mt, ks; };
static ConvForce conv_force() {
  ConvForce f = {0, 0, 0};
  if (const char* e = getenv("PMF_CONV_FORCE")) sscanf(e, "%d,%d,%d", &f.bn, &f.mt, &f.ks);
  return f;
}

// tile before the per-family corrections of conv_pick: caller-tuned (cfg), else by the size of the grid
static void conv_tile(const pmf_conv_desc_t* d, const ConvForce& f, int* BN, int* MT) {
  if (d->cfg) {                       // caller-tuned tile configuration
    const int bn = d->cfg & 0xff, mt = (d->cfg >> 8) & 0xff;
    *BN = (bn == 64 && d->Cout > 32) ? 64 : 32;
    *MT = mt == 2 ? 2 : 1;
    return;
  }
  *BN = d->Cout > 32 ? 64 : 32;
  // enough workgroups to fill 256 CUs: fall back to 128-pixel tiles on small maps
  const long px = (long)d->N * cdiv(d->OH, 8) * cdiv(d->OW, 32) * cdiv(d->Cout, *BN);
  *MT = px >= 512 ? 2 : 1;
  // 200..511 workgroups with 64-wide tiles = one workgroup per CU, nothing to overlap its staging with: 32-wide tiles
  // double the grid (measured +5 % on 128 -> 128 at 16x512); below 200 the K loop is split instead
  const long b64 = (long)d->N * cdiv(d->OH, 4) * cdiv(d->OW, 32) * cdiv(d->Cout, 64);
  if (*MT == 1 && *BN == 64 && b64 >= 200 && b64 < 512) *BN = 32;
  if (f.bn == 32 || (f.bn == 64 && d->Cout > 32)) *BN = f.bn;
  if (f.mt == 1 || f.mt == 2) *MT = f.mt;
}

// split-K factor: only when the M x N grid cannot fill the 256 CUs (low-resolution, many-channel layers)
static int choose_ksplit(const pmf_conv_desc_t* d, int blocks_mn, int nchunks, int forced) {
  int k;
  if (forced >= 1 && d->splitk_ws) {                  // PMF_CONV_FORCE: sweeps only
    k = forced;
  } else if (d->cfg && ((d->cfg >> 16) & 0xff)) {     // caller-tuned number of K splits
    if (!d->splitk_ws || blocks_mn > 1024) return 1;
    k = (d->cfg >> 16) & 0xff;
  } else {
    if (!d->splitk_ws || blocks_mn >= 200 || nchunks < 4) return 1;
    k = 512 / (blocks_mn > 0 ? blocks_mn : 1);
    // (a floor on the MFMA work per split was tried: the serial K loop of 1x1 layers is slower)
    if (k > nchunks / 2) k = nchunks / 2;
  }
  if (k > nchunks) k = nchunks;
  if (k > 32) k = 32;
  const int64_t slab = (int64_t)d->N * d->OH * d->OW * round_up(d->Cout, 4) * 4;      // the workspace holds k partial slabs
  while (k > 1 && slab * k > d->splitk_ws_bytes) --k;
  return k < 2 ? 1 : k;
}

// operands of the pipelined / direct / split loops: multiples of 16 channels with the same H x W, no broadcast, 32-bit offsets
static bool conv_srcs_uniform(const pmf_conv_desc_t* d) {
  for (int i = 0; i < d->nsrc; ++i) {
    if (d->src[i].C % 16 || (d->src[i].flags & PMF_SRC_BCAST)) return false;
    if (d->src[i].H != d->src[0].H || d->src[i].W != d->src[0].W) return false;
    if ((int64_t)d->N * d->src[i].H * d->src[i].W * d->src[i].ldc * 4 >= (1ll << 31)) return false;
  }
  return true;
}
static int conv_kc_alloc(const pmf_conv_desc_t* d) {     // rows per tap of the LDS weight tile: the widest operand, <= KC
  int cmax = 0;
  for (int i = 0; i < d->nsrc; ++i) cmax = d->src[i].C > cmax ? d->src[i].C : cmax;
  return cmax < KC ? cmax : KC;
}
static int conv_stages(const pmf_conv_desc_t* d, int kc) {     // K stages of kc channels (every operand a multiple of kc)
  int n = 0;
  for (int i = 0; i < d->nsrc; ++i) n += d->src[i].C / kc;
  return n;
}

// K-loop variant: 0 generic, 1 software-pipelined (halo tile, 1/3/4/9 taps, stride 1, operands multiples of 16
// channels with the same H x W, no broadcast), 4 pipelined with 64-channel stages (1x1, operands multiples of 64)
static int conv_pipe_mode(const pmf_conv_desc_t* d, const ConvGeom& g, int gather, int MT) {
  if (gather || d->in_stride != 1) return 0;
  if (d->ntaps != 1 && d->ntaps != 2 && d->ntaps != 3 && d->ntaps != 4 && d->ntaps != 9) return 0;
  if (!conv_srcs_uniform(d)) return 0;
  bool c64 = true;
  for (int i = 0; i < d->nsrc; ++i) c64 = c64 && d->src[i].C % 64 == 0;
  if (g.in_rows * g.in_cols * 4 > 256 * (MT == 2 ? 7 : 5)) return 0;
  if (d->ntaps == 1 && MT == 1 && c64 && g.in_rows * g.in_cols == 128) return 4;
  return 1;
}

// PIPE 11 (conv_kloop_direct): LDS bytes of the launch, or 0 when the layer does not qualify -- one tap, split-bf16
// weights, operands multiples of 16 channels with the same H x W, all weight fragments of one output-channel tile
// resident in LDS.
static bool conv_stem_class(const pmf_conv_desc_t* d) {
  // Default since round 6 (PMF_STEM_DIRECT=0 switches it off).  Per launch the variant is pinned against float64 like every
  // other (tests) and it is faster (7x7 stem 172-185 -> 121-134 us).  Rounds 4-5 kept it opt-in because the full-size gradient
  // parity of the camera decoder's low-resolution layers went from 1e-5 to 1e-3 against float64 with it; round 6's
  // mask-injected backward check (bench.py --parity-masked: the float64 / fp32 oracle passes replay the HIP path's activation
  // decisions) shows that residual is ReLU-kink flips, not arithmetic: with the decisions shared every parameter gradient sits
  // within 7e-5 of float64 with the variant on (tests/test_gpu_fullsize.py::test_masked_backward_parity).
  static const bool on = [] { const char* e = getenv("PMF_STEM_DIRECT"); return !(e && e[0] == '0'); }();
  return on && d->nsrc == 1 && d->src[0].C == 8 && d->ntaps >= 2 && d->ntaps <= PMF_MAX_TAPS &&
         !(d->src[0].flags & PMF_SRC_BCAST);
}
static int conv_direct_lds(const pmf_conv_desc_t* d, int BN, int* kchunk = nullptr) {
  constexpr int stream_kib = 96;
  if (kchunk) *kchunk = 0;
  // more than one tap: only on request (cfg bit 24, set by the plan autotuner when the variant measured faster), <= 9 taps
  const bool mtap = d->ntaps > 1;
  const bool stem = conv_stem_class(d);       // 8 padded channels, many taps: two taps per MFMA step (PIPE 14)
  if (mtap && !stem && (!((d->cfg >> 24) & 1) || d->ntaps > TAPG)) return 0;
  if (!d->w_s3 || (d->gather && !stem) || (d->ldw & 31)) return 0;
  if (stem) {
    if ((int64_t)d->N * d->src[0].H * d->src[0].W * d->src[0].ldc * 4 >= (1ll << 31)) return 0;
    const int lds_ = ((d->ntaps + 1) / 2) * (BN / 32) * 3 * 1024 + 16 * 8 + 256;
    return lds_ > 160 * 1024 ? 0 : (lds_ < 2 * 4 * 64 * 2 * 8 ? 2 * 4 * 64 * 2 * 8 : lds_);
  }
  if (!conv_srcs_uniform(d)) return 0;
  int Ktot = 0;
  for (int i = 0; i < d->nsrc; ++i) Ktot += d->src[i].C;
  const int NT = BN / 32, tab = 16 * Ktot + 256, steps = (Ktot / 16) * d->ntaps;
  int lds = steps * NT * 3 * 1024 + tab;
  if (lds < 2 * 4 * 64 * 2 * 8) lds = 2 * 4 * 64 * 2 * 8;
  if (lds > 160 * 1024 && !mtap) return 0;           // (multi-tap: streamed below or refused)
  // layers whose resident fragments exceed 96 KiB (768 input channels) stream them in chunks sized so that TWO workgroups
  // fit a CU and the weight DMA runs under the MFMAs instead of in front of them: 768 -> 256 at 16x512 70 -> 59 us
  // (threshold 96 KiB; from 64 KiB the streaming form measured neutral to 4 % slower)
  if (stream_kib > 0 && lds > stream_kib * 1024) {
    const int kch = ((76 * 1024 - tab) / (2 * NT * 3 * 1024)) & ~3;
    if (kch >= 8 && kch < steps) {
      if (kchunk) *kchunk = kch;
      return 2 * kch * NT * 3 * 1024 + tab;
    }
  }
  return lds > 160 * 1024 ? 0 : lds;
}

// split-bf16 path: 16-channel slabs per stage (1, 2 or 4) -- see conv_kloop_s3
static int conv_s3_slabs(const pmf_conv_desc_t* d, const ConvGeom& g) {
  for (int c = 4; c >= 2; c >>= 1) {
    if (d->ntaps * c > TAPG || g.in_rows * g.in_cols * 4 * c > 256 * 8) continue;
    bool ok = true;
    for (int i = 0; i < d->nsrc; ++i) ok = ok && d->src[i].C % (KC * c) == 0;
    if (ok) return c;
  }
  return 1;
}
// LDS bytes of the LDS-staged split loops (PIPE 5-10, 12): sl input slabs, the weight fragments of ntaps x sl stages for BN
// output channels, the per-thread scratch of the staging stores
static int conv_s3_lds(const ConvGeom& g, int ntaps, int sl, int BN) {
  return sl * round_up(g.in_rows * g.in_cols * (S3_APB / 4), 4) * 4 + ntaps * sl * (BN / 32) * 3 * 1024 + 2048;
}
// ... as the eligibility rules judge it before the tile is known: on the 64-wide tile, 16 bytes per slab in hand
static bool conv_s3_lds_fits(const ConvGeom& g, int ntaps, int sl) { return conv_s3_lds(g, ntaps, sl, 64) + 16 * sl <= 160 * 1024; }

// stride-2 3x3 layers on the split loop (PIPE 12): all nine taps live, halo tile of the 4 x 32-pixel output tile
// (9 x 65 input pixels) within ten staging slots per thread and the LDS budget of the 64-wide tile
static bool conv_s3_stride2(const pmf_conv_desc_t* d) {
  if (d->in_stride != 2 || d->ntaps != 9 || d->gather || !conv_srcs_uniform(d)) return false;
  ConvGeom g;
  int gather;
  // the 64 x 128-pixel tile, whatever the launch chose: the class is promised to the plan before cfg is known, PIPE 12 runs
  // 128-pixel tiles only and the 64-wide tile needs the most LDS
  pmf_conv_geometry(d->OH, d->OW, d->ntaps, d->tdy, d->tdx, 2, 0, 64, 1, conv_kc_alloc(d), &g, &gather);
  if (gather || g.in_rows * g.in_cols * 4 > 256 * 10) return false;
  return conv_s3_lds_fits(g, 9, 1);
}

// the LDS-staged split loop with MT x 128-pixel tiles: pipelined class + LDS budget (judged on the 64-wide tile)
static bool conv_s3_fits(const pmf_conv_desc_t* d, int MT) {
  if (d->in_stride == 2) return MT == 1 && conv_s3_stride2(d);
  ConvGeom g;
  int gather;
  // the 64-wide tile of MT x 128 pixels the caller asks about (pmf_conv_s3_eligible: 128 pixels, before cfg is known;
  // conv_pick: 256 pixels, to fall back to 128 where they do not qualify), not the chosen one
  pmf_conv_geometry(d->OH, d->OW, d->ntaps, d->tdy, d->tdx, d->in_stride, d->gather, 64, MT, conv_kc_alloc(d), &g, &gather);
  if (conv_pipe_mode(d, g, gather, MT) == 0) return false;
  return conv_s3_lds_fits(g, d->ntaps, conv_s3_slabs(d, g));
}

extern "C" int pmf_conv_s3_eligible(const pmf_conv_desc_t* d) {
  if (conv_stem_class(d) || d->ntaps == 1) {
    // stem class (3: weights in pack format 2) and 1x1 (2: only the direct variant), judged on the narrow tile; the caller sets
    // w_s3 afterwards
    pmf_conv_desc_t t = *d;
    t.w_s3 = (const void*)1;
    if (!t.ldw) t.ldw = 64;
    return conv_direct_lds(&t, 32) ? (conv_stem_class(d) ? 3 : 2) : 0;
  }
  return conv_s3_fits(d, 1) ? 1 : 0;      // (a 256-pixel tile that does not qualify falls back to 128 pixels: conv_pick)
}

extern "C" int pmf_conv_fwd_stat_rows_max(const pmf_conv_desc_t* d) {
  ConvGeom g;
  int gather;
  // the 32 x 128-pixel tile: 128-pixel tiles give the most rows of every tile cfg may select; split-K gives <= 1024
  pmf_conv_geometry(d->OH, d->OW, d->ntaps, d->tdy, d->tdx, d->in_stride, d->gather, 32, 1, conv_kc_alloc(d), &g, &gather);
  const int rows = g.tiles_x * g.tiles_y * d->N;
  return rows > 1024 ? rows : 1024;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The kernel selection.  conv_pick() answers once, for a descriptor, which kernel runs, on which tile, with how many K stages
// and K splits, combined where, on which grid, with how much LDS and how many partial-statistics rows; the launch,
// pmf_conv_fwd_stat_rows, pmf_conv_fwd_kstages and pmf_conv_fwd_variant all read the same ConvPick.  (The plan sizes the float64
// partial-row buffer from the row count and the BatchNorm finalize reads exactly that many rows: a count computed for another
// kernel than the one launched is an out-of-bounds write, or uninitialised rows in the batch statistics.)
enum { CONV_WS = PMF_CONV_WS_FAMILY };                        // family: the PIPE of conv_fwd_k, or the wave-scheduled kernel
enum { COMBINE_NONE = 0, COMBINE_TICKETS = 1, COMBINE_FINISH = 2 };     // K splits: in-kernel tickets / conv_finish_k
struct ConvPick {
  int rc;               // 0, or what pmf_conv_fwd returns instead of launching
  int family, BN, MT;
  ConvGeom g;           // as the chosen family needs it
  int gather;           // effective gather mode (the halo tile of a gather == 0 request may not fit LDS)
  int nchunks;          // K stages (wave-scheduled: of the conv_fwd_k selection it replaces, which the tuner sizes K splits from)
  int combine, stat_rows, lds;
  dim3 grid;
  WsPick ws;            // wave-scheduled: NCO, A-slab variant, WsGeom
};

// the wave-scheduled N-split kernel (conv_ws.hip): on request -- cfg bit 25 (PMF_CFG_WS, set by the plan autotuner where it
// measured faster) or PMF_CONV_WS=1 (every eligible launch with at least 128 workgroups: A/B) -- and eligible
static bool conv_ws_wanted(const pmf_conv_desc_t* d, WsPick* w) {
  static const int force = getenv("PMF_CONV_WS") ? atoi(getenv("PMF_CONV_WS")) : -1;     // 0: never, 1: wherever eligible
  constexpr int min_wgs = 128;
  const bool asked = (d->cfg >> 25) & 1;
  w->nco = w->rows = 0;
  if (force == 0 || (!asked && force != 1)) return false;
  conv_ws_pick(d, w);
  return w->nco && (asked || w->rows * (d->Cout / (32 * w->nco)) >= min_wgs);
}

static void conv_pick(const pmf_conv_desc_t* d, ConvPick* p) {
  const ConvForce force = conv_force();
  ConvGeom& g = p->g;
  p->rc = 0;
  auto refuse = [p](int rc) { if (!p->rc) p->rc = rc; };     // (the first refusal is the return code; the rest is still filled in)
  int BN, MT;
  conv_tile(d, force, &BN, &MT);
  if (d->ndst > 0 && BN == 64 && multi_tile(d) == 32) BN = 32;    // a 32-channel destination: no tile may straddle two
  // 1x1 / stem class / multi-tap on request (cfg bit 24) on split-bf16 weights: the direct variant -- no input tile in LDS, no K
  // split.  It was promised for the 32-wide tile (pmf_conv_s3_eligible); a 64-wide tile whose weight fragments do not fit LDS
  // falls back to it
  g.kchunk = 0;
  int direct = conv_direct_lds(d, BN, &g.kchunk);
  if (!direct && BN == 64 && (direct = conv_direct_lds(d, 32, &g.kchunk)) != 0) BN = 32;
  // LDS-staged split loop: the stride-2 form has 128-pixel tiles only, and the 256-pixel tile may not qualify where the
  // 128-pixel one does (dilated 3x3 on a 4-row map)
  if (d->w_s3 && d->ntaps > 1 && MT == 2 &&
      (d->in_stride == 2 || (!conv_stem_class(d) && !((d->cfg >> 24) & 1) && !conv_s3_fits(d, 2)))) MT = 1;
  p->BN = BN; p->MT = MT;
  int lds = pmf_conv_geometry(d->OH, d->OW, d->ntaps, d->tdy, d->tdx, d->in_stride, d->gather, BN, MT, conv_kc_alloc(d), &g,
                              &p->gather);
  if (lds > 160 * 1024) refuse(PMF_E_UNSUPPORTED);
  // 32-bit byte offsets in the epilogue (buffer stores): every tensor it touches must stay below 2 GiB
  if ((int64_t)d->N * d->out_H * d->out_W * d->out_ldc * 4 >= (1ll << 31)) refuse(PMF_E_UNSUPPORTED);
  if (d->ep_relu_x && (int64_t)d->N * d->out_H * d->out_W * d->ep_relu_ldc * 4 >= (1ll << 31)) refuse(PMF_E_UNSUPPORTED);
  if (d->ep_stat_mean && (!d->stats || !d->ep_relu_x)) refuse(PMF_E_ARG);
  if ((d->ep_flags & PMF_EP_STAT_X_ONLY) && !d->ep_stat_mean) refuse(PMF_E_ARG);
  g.Ktot = 0;
  int nchunks = 0;
  for (int i = 0; i < d->nsrc; ++i) { g.Ktot += d->src[i].C; nchunks += cdiv(d->src[i].C, KC); }
  int mode = conv_pipe_mode(d, g, p->gather, MT);
  if (direct) {
    mode = conv_stem_class(d) ? 14 : (d->ntaps > 1 ? 13 : 11);
    lds = direct;
    nchunks = 1;
  } else if (d->w_s3 && d->in_stride == 2) {     // stride-2 3x3
    if (MT != 1 || !conv_s3_stride2(d) || (d->ldw & 31)) refuse(PMF_E_UNSUPPORTED);
    mode = 12;
    nchunks = conv_stages(d, KC);
    g.a_floats = round_up(g.in_rows * g.in_cols * (S3_APB / 4), 4);
    lds = conv_s3_lds(g, 9, 1, BN);
    if (lds > 160 * 1024) refuse(PMF_E_UNSUPPORTED);
  } else if (d->w_s3 && mode == 0) {             // split-bf16 weights: the pipelined class only (pmf_conv_s3_eligible)
    refuse(PMF_E_UNSUPPORTED);
  } else if (d->w_s3) {
    if (d->ldw & 31) refuse(PMF_E_UNSUPPORTED);
    const int sl = conv_s3_slabs(d, g);
    mode = sl == 4 ? 7 : (sl == 2 ? 6 : 5);
    if (sl == 1 && d->ntaps == 9) mode = 8;
    if (sl == 2 && d->ntaps == 4) mode = 10;
    g.a_floats = sl * round_up(g.in_rows * g.in_cols * (S3_APB / 4), 4);
    lds = conv_s3_lds(g, d->ntaps, sl, BN);
    nchunks = conv_stages(d, KC * sl);
    if (lds < 2 * 4 * 64 * 2 * 8) lds = 2 * 4 * 64 * 2 * 8;
    if (lds > 160 * 1024) refuse(PMF_E_UNSUPPORTED);
  } else {
    if (!d->w) refuse(PMF_E_ARG);
    if (mode == 4) {                             // 64-channel stages
      nchunks = conv_stages(d, KC * 4);
      lds = (g.a_floats * 4 + 4 * KC * BN) * 4;
    }
  }
  if (mode == 1) g.kc_alloc = KC;   // the pipelined loop lays the weight slab out as [tap][16][BN]
  if (d->ndst > 0 && !pmf_conv_multi_ok(d)) refuse(PMF_E_ARG);
  const int co_tiles = cdiv(d->Cout, BN), tiles = g.tiles_x * g.tiles_y * d->N;
  g.ksplit = d->ndst > 0 ? 1 : choose_ksplit(d, tiles * co_tiles, nchunks, force.ks);
  g.ws = d->splitk_ws;
  g.ws_ld = round_up(d->Cout, 4);
  // in-kernel combine by the last-arriving workgroup of an output tile (conv_epi.h) when the caller gave a ticket array
  p->combine = g.ksplit == 1 ? COMBINE_NONE
             : (d->splitk_tickets != nullptr && tiles * co_tiles <= PMF_SPLITK_TICKETS ? COMBINE_TICKETS : COMBINE_FINISH);
  g.tickets = p->combine == COMBINE_TICKETS ? d->splitk_tickets : nullptr;
  g.one = (d->nsrc == 1 && g.ksplit == 1) ? 1 : 0;
  p->family = mode;
  p->nchunks = nchunks;
  p->lds = lds;
  p->grid = dim3(g.tiles_x * g.tiles_y, co_tiles * g.ksplit, d->N);
  // one row per workgroup of the kernel that writes the statistics: conv_finish_k's, else one per tile and sample
  p->stat_rows = p->combine == COMBINE_FINISH ? finish_rows(d, true) : tiles;
  if (conv_ws_wanted(d, &p->ws)) {               // replaces the whole selection above but its K-stage count; refuses nothing
    const WsPick& w = p->ws;
    p->rc = 0;
    p->family = CONV_WS; p->BN = 32 * w.nco; p->MT = 1;
    g = w.cg;
    p->gather = 0;
    p->combine = COMBINE_NONE; p->stat_rows = w.rows; p->lds = w.lds;
    p->grid = dim3(w.g.tiles_x * w.g.tiles_y, d->Cout / (32 * w.nco), d->N);
  }
}

// number of partial-statistics rows pmf_conv_fwd writes for this descriptor (stats must hold rows*2*Cout doubles)
extern "C" int pmf_conv_fwd_stat_rows(const pmf_conv_desc_t* d) { ConvPick p; conv_pick(d, &p); return p.stat_rows; }
extern "C" int pmf_conv_fwd_kstages(const pmf_conv_desc_t* d) { ConvPick p; conv_pick(d, &p); return p.nchunks; }

// the launch of one instantiation; the LDS opt-in once per device, the first time a launch asks for more than 64 KiB
template <int BN, int MT, int PIPE>
static int conv_run(const pmf_conv_desc_t* d, const ConvPick& p, hipStream_t s) {
  static unsigned long long opted_in = 0ull;
  if (p.lds > 64 * 1024 && pmf_first_on_device(&opted_in))
    (void)hipFuncSetAttribute((const void*)conv_fwd_k<BN, MT, PIPE>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  pmf_conv_desc_t dd = *d;
  dd.gather = p.gather;
  hipLaunchKernelGGL((conv_fwd_k<BN, MT, PIPE>), p.grid, dim3(256), p.lds, s, dd, p.g);
  PMF_LAUNCH_CHECK();
  return p.combine == COMBINE_FINISH ? pmf_conv_finish_launch(&dd, p.g, s) : 0;
}

static int conv_args(const pmf_conv_desc_t* d) {
  if (!d || d->nsrc < 1 || d->nsrc > PMF_MAX_SRC || d->ntaps < 1 || d->ntaps > PMF_MAX_TAPS) return PMF_E_ARG;
  if (d->ldw % 4 || d->in_stride < 1 || d->in_stride > 2) return PMF_E_ARG;
  for (int i = 0; i < d->nsrc; ++i)
    if (d->src[i].C % 8 || d->src[i].ldc % 4) return PMF_E_ARG;
  return 0;
}

// what only a launch needs: a shape with something to compute, an operand and a destination to address
static int conv_launch_args(const pmf_conv_desc_t* d) {
  if (d->N < 1 || d->OH < 1 || d->OW < 1 || d->Cout < 1) return PMF_E_ARG;
  for (int i = 0; i < d->nsrc; ++i)
    if (!d->src[i].x) return PMF_E_ARG;
  if (d->ndst <= 0 && !d->out) return PMF_E_ARG;
  for (int k = 0; k < d->ndst && k < PMF_MAX_SRC; ++k)
    if (!d->dst[k].out) return PMF_E_ARG;
  return 0;
}

extern "C" int pmf_conv_fwd(const pmf_conv_desc_t* d, pmf_stream_t st) {
  hipStream_t s = (hipStream_t)st;
  if (const int rc = conv_args(d)) return rc;
  if (const int rc = conv_launch_args(d)) return rc;
  ConvPick p;
  conv_pick(d, &p);
  if (p.rc) return p.rc;
  if (p.family == CONV_WS) return conv_ws_run(d, p.ws, s);
  // (BN, MT, PIPE) -> its instantiation; 64-channel stages (4) and the stride-2 split loop (12) exist for 128-pixel tiles only
#define CONV_CASE(bn, mt, pipe) case bn * 1000 + mt * 100 + pipe: return conv_run<bn, mt, pipe>(d, p, s);
#define CONV_TILE(bn, mt)                                                                                                 \
  CONV_CASE(bn, mt, 0) CONV_CASE(bn, mt, 1) CONV_CASE(bn, mt, 5) CONV_CASE(bn, mt, 6) CONV_CASE(bn, mt, 7) CONV_CASE(bn, mt, 8) \
  CONV_CASE(bn, mt, 10) CONV_CASE(bn, mt, 11) CONV_CASE(bn, mt, 13) CONV_CASE(bn, mt, 14)
  switch (p.BN * 1000 + p.MT * 100 + p.family) {
    CONV_TILE(32, 1) CONV_TILE(32, 2) CONV_TILE(64, 1) CONV_TILE(64, 2)
    CONV_CASE(32, 1, 4) CONV_CASE(32, 1, 12) CONV_CASE(64, 1, 4) CONV_CASE(64, 1, 12)
  }
#undef CONV_TILE
#undef CONV_CASE
  return PMF_E_UNSUPPORTED;
}

// which kernel pmf_conv_fwd runs for a descriptor, and how (include/pmf_amd.h); nothing is launched
extern "C" int pmf_conv_fwd_variant(const pmf_conv_desc_t* d, int32_t info[12]) {
  for (int i = 0; i < 12; ++i) info[i] = 0;
  if (const int rc = conv_args(d)) return rc;
  ConvPick p;
  conv_pick(d, &p);
  const bool ws = p.family == CONV_WS;
  const int32_t v[12] = {p.BN, p.MT, p.g.ksplit, p.combine, p.stat_rows, p.nchunks, p.lds, (int32_t)p.grid.x, (int32_t)p.grid.y,
                         (int32_t)p.grid.z, ws ? p.ws.nco : 0, ws ? p.ws.asl : 0};
  for (int i = 0; i < 12; ++i) info[i] = v[i];
  return p.rc ? p.rc : p.family;
}
