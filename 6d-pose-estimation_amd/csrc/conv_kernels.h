// Device code of the implicit-GEMM convolution: the register-staged and LDS-DMA
// kernels, the patch kernel (conv_patch.h) and the fused backward kernels.
// Included by conv_igemm.hip only.
#pragma once
#include "conv_geom.h"
#include "lds_dma.h"
#include "wgrad_body.h"

namespace {

constexpr int kThreads = 256;

// TM x TN accumulator tiles per wave; PART = floats of one (tile, split) partial
template <int TM, int TN, int NW>
__device__ __forceinline__ bool splitk_merge(f32x4 (&acc)[TM][TN], char* smem, int tile, int split, int nsplit,
                                             int* cnt, float* part) {
  constexpr int PART = NW * TM * TN * 64 * 4;
  constexpr int SC1 = 16;   // buffer cache-policy bits: sc1
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* base = part + (int64_t)tile * nsplit * PART;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(base, 0, nsplit * PART * 4, 0x00020000);
  const int voff = (wave * TM * TN * 64 + lane) * 16;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[i][j]), rs,
                                             voff + (i * TN + j) * 1024, split * PART * 4, SC1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave, before the barrier
  __syncthreads();
  int* flag = reinterpret_cast<int*>(smem);
  if (tid == 0) flag[0] = __hip_atomic_fetch_add(&cnt[tile], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const bool last = flag[0] == nsplit - 1;
  __syncthreads();   // flag read by every wave before the epilogue reuses the LDS
  if (!last) return false;
  if (tid == 0) __hip_atomic_store(&cnt[tile], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  f32x4 mine[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) mine[i][j] = acc[i][j];
  for (int s = 0; s < nsplit; ++s) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const f32x4 v = s == split ? mine[i][j]
                                   : __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                                   rs, voff + (i * TN + j) * 1024, s * PART * 4, SC1));
        acc[i][j] = s == 0 ? v : acc[i][j] + v;
      }
  }
  return true;
}

// LDS bytes the BN-reduce epilogue needs beyond the staged tile: per wave, per chunk
// column, (sum dz, sum dz xhat, sum dz xhat2) x 16-byte chunk = 12 bytes per column,
// + four per-channel constants
constexpr int bnr_lds(int nw, int bn) { return 12 * nw * bn + 16 * bn; }

// kDgradS2 launched in place (dres == dx) when a single parity class has taps
// (1x1 stride 2): the other classes' pixels are already final, so the grid covers
// that class alone instead of launching three workgroups per tile that only exit.
void s2_single_class(Geom& g, const void* res, const void* out) {
  g.s2one = 0;
  if (res != out) return;
  int n = 0, last = 0;
  for (int cls = 0; cls < 4; ++cls) {
    const int kh0 = ((cls >> 1) + g.pad) & 1, kw0 = ((cls & 1) + g.pad) & 1;
    if (((g.KH - kh0 + 1) >> 1) * ((g.KW - kw0 + 1) >> 1) > 0) { ++n; last = cls; }
  }
  if (n == 1) g.s2one = last + 1;
}
__host__ __device__ inline int s2_classes(const Geom& g) { return g.s2one ? 1 : 4; }


// ds_read_b128 fragment reads: lanes (row = l & 15, chunk = l >> 4) of a 16-row
// block; this XOR makes every 16-lane LDS group hit 16 distinct 16-byte slots.
__device__ __forceinline__ int swz(int row) { return (4 - ((row >> 2) & 3)) & 3; }

// Output row of GEMM row m: m itself, or for a kDgradS2 parity class cls = (py, px)
// the dX pixel (n, 2*yy + py, 2*xx + px) of class-local row m = (n, yy, xx).
__device__ __forceinline__ int64_t out_row(const Geom& g, int cls, int m) {
  if (cls < 0) return m;
  const int hw = g.RH * g.RW;
  const int n = m / hw, rem = m - n * hw;
  const int yy = rem / g.RW, xx = rem - yy * g.RW;
  return ((int64_t)n * 2 * g.RH + 2 * yy + (cls >> 1)) * (2 * g.RW) + 2 * xx + (cls & 1);
}

// Shared epilogue: + bias, BatchNorm partial statistics, LDS-staged 16-B stores
// (+ residual).  Must be entered after a barrier that ends all LDS reads.
// ACT: the eval BN-act store (Geom::act) compiled in (1) or out (0): the launchers
// instantiate both, so the training kernels carry no trace of it
// NW waves per workgroup: WM = NW / 2 along M times 2 along N, each wave owning a
// (BM / WM) x (BN / 2) block of 16x16 MFMA tiles (TM x TN of them)
// n consecutive floats (n = 4 or 8, 16-B aligned) as 16-B loads
template <int N>
__device__ __forceinline__ void load_f32s(const float* __restrict__ p, float (&f)[N]) {
  static_assert(N % 4 == 0, "16-byte loads");
#pragma unroll
  for (int i = 0; i < N / 4; ++i) {
    const float4 v = *reinterpret_cast<const float4*>(p + 4 * i);
    f[4 * i] = v.x; f[4 * i + 1] = v.y; f[4 * i + 2] = v.z; f[4 * i + 3] = v.w;
  }
}

template <int NW> struct WaveGrid { static constexpr int WM = NW / 2, WN = 2, NT = 64 * NW; };

// BatchNorm-backward partial sums of one tile (Geom::bnr_*): a thread's chunks share
// one chunk column (E channels); lanes of a column fold by xor shuffles, waves through
// LDS (`red`, past the staged tile), in a fixed order -- deterministic.  dz = dX as
// stored (T) times the BN's ReLU: the stored bits (bnr_mask) or T(y * rs + rb) > 0
// recomputed, exactly as pose6d_bn_bwd's reduce decides it.  The per-channel
// constants sit in LDS (`cst` [4][BN]: mean, invstd, then rs, rb or mean2, invstd2),
// read per 4-channel group where used: held in registers they cost the data-gradient
// kernels two waves of occupancy.
template <typename T, int BN, int NW, int IT>
__device__ __forceinline__ void bnr_partials(const Geom& g, const uint4 (&ov)[IT], const bool (&okv)[IT],
                                             const int64_t (&oidx)[IT], const uint4 (&yv)[IT],
                                             const unsigned (&mb)[IT], float* red, const float* cst, int prow,
                                             int n0) {
  constexpr int E = 16 / (int)sizeof(T), CPR = BN * (int)sizeof(T) / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cl = (tid % CPR) * E;   // the chunk column's first channel within the tile
  const bool dual = g.bnr_y2 != nullptr, mk3 = g.bnr_mask != nullptr;
  float sd[E], sq[E], sq2[E];
#pragma unroll
  for (int e = 0; e < E; ++e) sd[e] = sq[e] = sq2[e] = 0.f;
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    if (!okv[it]) continue;
    T a[E], yy[E], y2[E];
    __builtin_memcpy(a, &ov[it], 16);
    __builtin_memcpy(yy, &yv[it], 16);
    // the dual branch's y: loaded here, not prefetched (registers; still before the stores)
    const uint4 y2v = dual ? *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(g.bnr_y2) + oidx[it])
                           : uint4{0, 0, 0, 0};
    __builtin_memcpy(y2, &y2v, 16);
#pragma unroll
    for (int e4 = 0; e4 < E; e4 += 4) {
      const float4 mu = *reinterpret_cast<const float4*>(cst + cl + e4);
      const float4 iv = *reinterpret_cast<const float4*>(cst + BN + cl + e4);
      const float4 ca = *reinterpret_cast<const float4*>(cst + 2 * BN + cl + e4);
      const float4 cb = *reinterpret_cast<const float4*>(cst + 3 * BN + cl + e4);
      const float m4[4] = {mu.x, mu.y, mu.z, mu.w}, i4[4] = {iv.x, iv.y, iv.z, iv.w};
      const float a4[4] = {ca.x, ca.y, ca.z, ca.w}, b4[4] = {cb.x, cb.y, cb.z, cb.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = e4 + k;
        const float y = p6::to_f(yy[e]);
        const bool on = mk3 ? ((mb[it] >> e) & 1u) != 0u : p6::to_f(p6::from_f<T>(fmaf(y, a4[k], b4[k]))) > 0.f;
        const float d = on ? p6::to_f(a[e]) : 0.f;
        sd[e] += d;
        sq[e] = fmaf(d, (y - m4[k]) * i4[k], sq[e]);
        if (dual) sq2[e] = fmaf(d, (p6::to_f(y2[e]) - a4[k]) * b4[k], sq2[e]);
      }
    }
    asm volatile("" ::: "memory");   // keep the constant reads per trip (not hoisted into registers)
  }
#pragma unroll
  for (int o = CPR; o < 64; o <<= 1)
#pragma unroll
    for (int e = 0; e < E; ++e) {
      sd[e] += __shfl_xor(sd[e], o, 64);
      sq[e] += __shfl_xor(sq[e], o, 64);
      if (dual) sq2[e] += __shfl_xor(sq2[e], o, 64);
    }
  if (lane < CPR) {
    float* r = red + (wave * CPR + lane) * 3 * E;
#pragma unroll
    for (int e = 0; e < E; ++e) { r[e] = sd[e]; r[E + e] = sq[e]; r[2 * E + e] = sq2[e]; }
  }
  __syncthreads();
  if (tid < BN) {
    const int cc = tid / E, e = tid - cc * E, c = n0 + tid;
    float S = 0.f, Q = 0.f, Q2 = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const float* r = red + (w * CPR + cc) * 3 * E;
      S += r[e];
      Q += r[E + e];
      Q2 += r[2 * E + e];
    }
    if (c < g.Ncols) {
      const int64_t rows = g.bnr_rows;
      g.bnr_part[(int64_t)c * rows + prow] = S;
      g.bnr_part[((int64_t)g.Ncols + c) * rows + prow] = Q;
      if (dual) {
        g.bnr_part2[(int64_t)c * rows + prow] = S;
        g.bnr_part2[((int64_t)g.Ncols + c) * rows + prow] = Q2;
      }
    }
  }
}

// What the epilogue's store loop reads from global memory besides the tile: the
// residual chunks and their mask bytes, and for the BN-reduce epilogue the BN's input
// y chunks, its ReLU bits and per-channel constants (epi_prefetch).  Kept apart from
// conv_epilogue so that a workgroup with one or two K-steps can issue these loads
// right behind its operand DMA (one memory round trip instead of two per workgroup:
// the 1x1 data gradients with K = Cout = 64 / 128 are a DMA wait, 8 MFMAs and this
// epilogue).
template <typename T, int BM, int BN, int NW, bool BNR>
struct EpiPre {
  static constexpr int CPR = BN * (int)sizeof(T) / 16;                 // 16-B chunks per tile row
  static constexpr int IT = (BM * CPR + 64 * NW - 1) / (64 * NW);      // store-loop trips per thread
  static constexpr int BI = BNR ? IT : 1;
  bool okv[IT];
  int64_t oidx[IT];    // element offset of the trip's chunk in `out` (0 when out of range)
  uint4 rv[IT];
  unsigned mbv[IT];
  uint4 byv[BI];       // BN reduce: the BN's input y chunks
  unsigned bmv[BI];    // and its ReLU bits
  float bcst[4];       // this thread's channel's BN-reduce constants (tid < BN)
};

template <typename T, int BM, int BN, int ACT, int NW, bool BNR>
__device__ __forceinline__ void epi_prefetch(EpiPre<T, BM, BN, NW, BNR>& p, const Geom& g,
                                             const T* __restrict__ res, int m0, int n0, int cls) {
  using P = EpiPre<T, BM, BN, NW, BNR>;
  constexpr int NT = WaveGrid<NW>::NT, CPR = P::CPR, IT = P::IT;
  constexpr int E = 16 / (int)sizeof(T);
  constexpr bool act = ACT == 1;
  const int tid = threadIdx.x;
  const bool bnr = BNR && g.bnr_part != nullptr;
  for (int k = 0; k < 4; ++k) p.bcst[k] = 0.f;
  if constexpr (BNR) {
    if (bnr && tid < BN) {
      const int c = n0 + tid < g.Ncols ? n0 + tid : 0;
      p.bcst[0] = g.bnr_mean[c];
      p.bcst[1] = g.bnr_inv[c];
      if (g.bnr_y2) {
        p.bcst[2] = g.bnr_mean2[c];
        p.bcst[3] = g.bnr_inv2[c];
      } else if (!g.bnr_mask) {
        p.bcst[2] = g.bnr_rs[c];
        p.bcst[3] = g.bnr_rb[c];
      }
    }
  }
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int idx = tid + it * NT;
    const int lr = idx / CPR, cc = idx - lr * CPR;
    const int m = m0 + lr, c = n0 + cc * E;
    p.okv[it] = idx < BM * CPR && m < g.M && c < g.Ncols;
    p.oidx[it] = p.okv[it] ? out_row(g, cls, m) * g.Ncols + c : 0;
    p.rv[it] = uint4{0, 0, 0, 0};
    p.mbv[it] = 0xFFu;
    if (res) {
      p.rv[it] = *reinterpret_cast<const uint4*>(res + p.oidx[it]);
      if (!act && g.res_mask) p.mbv[it] = g.res_mask[p.oidx[it] / E];
    }
    if constexpr (BNR) {
      p.byv[it] = uint4{0, 0, 0, 0};
      p.bmv[it] = 0u;
      if (bnr) {
        p.byv[it] = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(g.bnr_y) + p.oidx[it]);
        if (g.bnr_mask) p.bmv[it] = g.bnr_mask[p.oidx[it] / E];
      }
    }
  }
}

// BNR: the BN-reduce epilogue (Geom::bnr_*) compiled in -- the data-gradient instances.
// `pre`: the store loop's global operands, already fetched (epi_prefetch) when
// `pre_done`, else fetched here first.
template <typename T, int BM, int BN, int ACT = 0, int NW = 4, bool DUAL = false, bool BNR = false>
__device__ __forceinline__ void conv_epilogue(f32x4 (&acc)[BM / (16 * (NW / 2))][BN / 32], char* smem, const Geom& g,
                                              const float* __restrict__ bias, const T* __restrict__ res,
                                              T* __restrict__ out, float* __restrict__ stats, int m0, int n0,
                                              int cls, const f32x4 (*acc2)[BN / 32],
                                              EpiPre<T, BM, BN, NW, BNR>& pre, bool pre_done) {
  constexpr int WM = WaveGrid<NW>::WM, NT = WaveGrid<NW>::NT;
  constexpr int TM = BM / (16 * WM), TN = BN / 32;
  static_assert(TM % 2 == 0, "BatchNorm partials cover 32-row blocks of one wave");
  constexpr int CROW = BN * (int)sizeof(T) + 16;  // epilogue tile row stride (bytes)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int CPR = BN * (int)sizeof(T) / 16;  // 16-B chunks per tile row
  constexpr int E = 16 / (int)sizeof(T);
  constexpr int IT = (BM * CPR + NT - 1) / NT;    // store-loop trips per thread
  static_assert(NT % CPR == 0, "store loop: fixed chunk column per thread");
  constexpr bool act = ACT == 1;
  // Everything the store loop reads from global memory (the residual chunks and their
  // mask bytes here, the eval BN-act constants once the tile is staged) is fetched
  // before the first store, and the stores are issued after the last use: a load
  // issued after a store can only be waited for with vmcnt(0), which waits for the
  // store's acknowledgement too -- a full memory round trip per trip of the store loop
  // (measured: the eval 1x1 convs took 1.2-2.2x their plain-store time that way).
  if (!pre_done) epi_prefetch<T, BM, BN, ACT, NW, BNR>(pre, g, res, m0, n0, cls);
  const bool (&okv)[IT] = pre.okv;
  const int64_t (&oidx)[IT] = pre.oidx;
  const uint4 (&rv)[IT] = pre.rv;
  const unsigned (&mbv)[IT] = pre.mbv;
  const auto& byv = pre.byv;
  const auto& bmv = pre.bmv;
  const float (&bcst)[4] = pre.bcst;
  const bool bnr = BNR && g.bnr_part != nullptr;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fc = lane >> 4;
  const int row_base = m0 + wm * (BM / WM);
  const int col_base = n0 + wn * (BN / 2);
  if (bias) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int c = col_base + j * 16 + fr;
      const float bv = c < g.Ncols ? bias[c] : 0.f;
#pragma unroll
      for (int i = 0; i < TM; ++i) acc[i][j] += bv;
    }
  }
  if (stats) {
    // partials over blocks of 32 rows (two 16-row MFMA tiles), stats row r = m / 32,
    // stored channel-major: stats[c][r] (sum), stats[C + c][r] (M2):
    // (sum, M2 about the block-local mean) -- Chan-mergeable, free of the
    // E[x^2]-E[x]^2 cancellation; row counts follow from M (pose6d_bn_finalize).
#pragma unroll
    for (int h = 0; h < TM / 2; ++h) {
      const int rb = row_base + h * 32;
      const int nval = min(max(g.M - rb, 0), 32);
      const float inv_n = nval > 0 ? 1.0f / (float)nval : 0.f;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        float s = 0.f;
#pragma unroll
        for (int i = 2 * h; i < 2 * h + 2; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = row_base + i * 16 + fc * 4 + r;
            s += m < g.M ? acc[i][j][r] : 0.f;
          }
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        const float mu = s * inv_n;
        float q = 0.f;
#pragma unroll
        for (int i = 2 * h; i < 2 * h + 2; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = row_base + i * 16 + fc * 4 + r;
            const float d = acc[i][j][r] - mu;
            q = m < g.M ? fmaf(d, d, q) : q;
          }
        q += __shfl_xor(q, 16, 64);
        q += __shfl_xor(q, 32, 64);
        const int c = col_base + j * 16 + fr;
        if (lane < 16 && c < g.Ncols && nval > 0) {
          // channel-major [2][C][rows]: the finalize reads each channel's rows coalesced
          const int64_t rows = (g.M + 31) >> 5;
          stats[(int64_t)c * rows + (rb >> 5)] = s;
          stats[((int64_t)g.Ncols + c) * rows + (rb >> 5)] = q;
        }
      }
    }
  }
  // stage the tile through LDS (staging buffers are dead after the final barrier)
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lr = wm * (BM / WM) + i * 16 + fc * 4 + r;
        const int lc = wn * (BN / 2) + j * 16 + fr;
        *reinterpret_cast<T*>(smem + lr * CROW + lc * (int)sizeof(T)) = p6::from_f<T>(acc[i][j][r]);
        // kGemmDual: the downsample branch's tile, rounded to T as its own launch stored it
        if constexpr (DUAL)
          *reinterpret_cast<T*>(smem + (BM + lr) * CROW + lc * (int)sizeof(T)) = p6::from_f<T>(acc2[i][j][r]);
      }
  float* bnr_cst = reinterpret_cast<float*>(smem + BM * CROW + 12 * NW * BN);
  if constexpr (BNR) {
    if (bnr && tid < BN) {
#pragma unroll
      for (int k = 0; k < 4; ++k) bnr_cst[k * BN + tid] = bcst[k];
    }
  }
  float asc[E], ash[E], arsc[E], arsh[E];
  // (issued after the accumulators are staged: their registers are free again)
  if (act) {
    // a thread's 16-B chunk column (tid % CPR) is the same on every trip: one set of
    // channel constants; Ncols % 8 == 0, so a chunk is wholly in range or out
    const int c = n0 + (tid % CPR) * E;
    const int cs = c < g.Ncols ? c : 0;
    load_f32s<E>(g.act_scale + cs, asc);
    load_f32s<E>(g.act_shift + cs, ash);
    if (g.act_rscale) {
      load_f32s<E>(g.act_rscale + cs, arsc);
      load_f32s<E>(g.act_rshift + cs, arsh);
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e) arsc[e] = arsh[e] = 0.f;
    }
  }
  // raw barrier: LDS writes done (lgkmcnt), the prefetched global loads stay in flight
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  uint4 ov[IT];
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int idx = tid + it * NT;
    const int lr = idx < BM * CPR ? idx / CPR : 0, cc = idx - (idx / CPR) * CPR;
    uint4 v = *reinterpret_cast<const uint4*>(smem + lr * CROW + cc * 16);
    if (act) {
      // pose6d_bn_act_fwd's arithmetic on the stored (T-rounded) conv output
      T a[E], b[E];
      __builtin_memcpy(a, &v, 16);
      if constexpr (DUAL) {
        const uint4 dv = *reinterpret_cast<const uint4*>(smem + (BM + lr) * CROW + cc * 16);
        __builtin_memcpy(b, &dv, 16);
      } else {
        __builtin_memcpy(b, &rv[it], 16);
      }
#pragma unroll
      for (int e = 0; e < E; ++e) {
        float x = fmaf(p6::to_f(a[e]), asc[e], ash[e]);
        if (DUAL || res) x += g.act_rscale ? fmaf(p6::to_f(b[e]), arsc[e], arsh[e]) : p6::to_f(b[e]);
        if (g.act_relu) x = fmaxf(x, 0.f);
        a[e] = p6::from_f<T>(x);
      }
      __builtin_memcpy(&v, a, 16);
    } else if (res) {
      const unsigned mb = mbv[it];
      T a[E], b[E];
      __builtin_memcpy(a, &v, 16);
      __builtin_memcpy(b, &rv[it], 16);
#pragma unroll
      for (int e = 0; e < E; ++e)
        a[e] = p6::from_f<T>(p6::to_f(a[e]) + ((mb >> e) & 1u ? p6::to_f(b[e]) : 0.f));
      __builtin_memcpy(&v, a, 16);
    }
    ov[it] = v;
  }
  if constexpr (BNR) {
    if (bnr) {
      const int prow = ((cls >= 0 && !g.s2one) ? cls : 0) * g.gm + m0 / BM;
      bnr_partials<T, BN, NW, IT>(g, ov, okv, oidx, byv, bmv, reinterpret_cast<float*>(smem + BM * CROW), bnr_cst,
                                  prow, n0);
    }
  }
#pragma unroll
  for (int it = 0; it < IT; ++it)
    if (okv[it]) *reinterpret_cast<uint4*>(out + oidx[it]) = ov[it];
}

template <typename T, int BM, int BN, int MODE, bool ACT>
__global__ __launch_bounds__(kThreads) void conv_igemm_kernel(const T* __restrict__ src, const T* __restrict__ wts,
                                                              const float* __restrict__ bias, const T* __restrict__ res,
                                                              T* __restrict__ out, float* __restrict__ stats, Geom g) {
  constexpr int VEC = KT<T>::VEC;
  constexpr int BK = KT<T>::BK;
  constexpr int TM = BM / 32;            // 16x16 tiles per wave along M (waves 2 x 2)
  constexpr int TN = BN / 32;
  constexpr int A_PER = BM / 64;         // 16-B chunks per thread per A stage
  constexpr int B_PER = BN / 64;
  constexpr int STAGE = (BM + BN) * 64;  // bytes per LDS buffer
  extern __shared__ __attribute__((aligned(16))) char smem[];

  // XCD-aware remap: consecutive logical tiles (same M rows) share an XCD's L2.
  const int nwg = g.gm * g.gn;
  int bid = blockIdx.x;
  {
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  const int tm = bid / g.gn, tn = bid - tm * g.gn;
  const int m0 = tm * BM, n0 = tn * BN;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int ck = tid & 3;  // this thread's 16-B chunk within a 64-B row segment

  // ---- per-thread A rows (fixed over K) ----
  int a_pix[A_PER], a_y[A_PER], a_x[A_PER];
  bool a_ok[A_PER];
#pragma unroll
  for (int i = 0; i < A_PER; ++i) {
    const int m = m0 + (tid >> 2) + 64 * i;
    a_ok[i] = m < g.M;
    const int mm = a_ok[i] ? m : 0;
    if (MODE == kGemm) {
      a_pix[i] = mm; a_y[i] = 0; a_x[i] = 0;
    } else {
      const int hw = g.RH * g.RW;
      const int n = mm / hw, rem = mm - n * hw;
      const int y = rem / g.RW, x = rem - y * g.RW;
      a_pix[i] = n * g.SH * g.SW;
      if (MODE == kDgrad) { a_y[i] = y + g.pad; a_x[i] = x + g.pad; }
      else { a_y[i] = y * g.stride - g.pad; a_x[i] = x * g.stride - g.pad; }
    }
  }
  // ---- per-thread B rows ----
  const T* b_ptr[B_PER];
  bool b_ok[B_PER];
#pragma unroll
  for (int i = 0; i < B_PER; ++i) {
    const int n = n0 + (tid >> 2) + 64 * i;
    b_ok[i] = n < g.Ncols;
    b_ptr[i] = wts + (int64_t)(b_ok[i] ? n : 0) * g.Kpad + ck * VEC;
  }

  const int nk = g.Kpad / BK;
  uint4 ra[A_PER], rb[B_PER];

  auto load_tile = [&](int kt) {
    const int k0 = kt * BK;
#pragma unroll
    for (int i = 0; i < B_PER; ++i)
      rb[i] = b_ok[i] ? *reinterpret_cast<const uint4*>(b_ptr[i] + k0) : make_uint4(0, 0, 0, 0);
    if (MODE == kGemm) {
#pragma unroll
      for (int i = 0; i < A_PER; ++i)
        ra[i] = a_ok[i] ? *reinterpret_cast<const uint4*>(src + (int64_t)a_pix[i] * g.K + k0 + ck * VEC)
                        : make_uint4(0, 0, 0, 0);
    } else if (MODE == kFwd || MODE == kDgrad) {
      const int tap = k0 >> g.log2SC, c0 = k0 & (g.SC - 1);
      const int kh = tap / g.KW, kw = tap - kh * g.KW;
#pragma unroll
      for (int i = 0; i < A_PER; ++i) {
        int sy, sx;
        bool ok = a_ok[i] && k0 < g.K;
        if (MODE == kFwd) {
          sy = a_y[i] + kh; sx = a_x[i] + kw;
        } else {
          const int ty = a_y[i] - kh, tx = a_x[i] - kw;
          ok = ok && ty >= 0 && tx >= 0;
          if (g.stride == 2) { ok = ok && !(ty & 1) && !(tx & 1); sy = ty >> 1; sx = tx >> 1; }
          else { sy = ty; sx = tx; }
        }
        ok = ok && (unsigned)sy < (unsigned)g.SH && (unsigned)sx < (unsigned)g.SW;
        ra[i] = ok ? *reinterpret_cast<const uint4*>(src + ((int64_t)(a_pix[i] + sy * g.SW + sx) << g.log2SC) + c0 +
                                                     ck * VEC)
                   : make_uint4(0, 0, 0, 0);
      }
    } else {  // kFwdNarrow: SC == 4 channels per tap (stem, Cin padded 3 -> 4)
      constexpr int UNITS = VEC / 4;       // taps per 16-B chunk (bf16: 2, fp32: 1)
#pragma unroll
      for (int i = 0; i < A_PER; ++i) {
        uint32_t w[4];
#pragma unroll
        for (int u = 0; u < UNITS; ++u) {
          const int k = k0 + ck * VEC + u * 4;
          const int tap = k >> 2;
          const int kh = tap / g.KW, kw = tap - kh * g.KW;
          const int sy = a_y[i] + kh, sx = a_x[i] + kw;
          const bool ok = a_ok[i] && k < g.K && (unsigned)sy < (unsigned)g.SH && (unsigned)sx < (unsigned)g.SW;
          const T* p = src + ((int64_t)(a_pix[i] + sy * g.SW + sx) << 2);
          if (UNITS == 2) {
            uint2 v = ok ? *reinterpret_cast<const uint2*>(p) : make_uint2(0, 0);
            w[2 * u] = v.x; w[2 * u + 1] = v.y;
          } else {
            uint4 v = ok ? *reinterpret_cast<const uint4*>(p) : make_uint4(0, 0, 0, 0);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
          }
        }
        ra[i] = make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
  };

  auto store_tile = [&](int buf) {
    char* As = smem + buf * STAGE;
    char* Bs = As + BM * 64;
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      const int row = (tid >> 2) + 64 * i;
      *reinterpret_cast<uint4*>(As + row * 64 + ((ck ^ swz(row)) << 4)) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      const int row = (tid >> 2) + 64 * i;
      *reinterpret_cast<uint4*>(Bs + row * 64 + ((ck ^ swz(row)) << 4)) = rb[i];
    }
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fc = lane >> 4;
  auto compute = [&](int buf) {
    const char* As = smem + buf * STAGE;
    const char* Bs = As + BM * 64;
    uint4 af[TM], bfr[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int row = wm * (BM / 2) + i * 16 + fr;
      af[i] = *reinterpret_cast<const uint4*>(As + row * 64 + ((fc ^ swz(row)) << 4));
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int row = wn * (BN / 2) + j * 16 + fr;
      bfr[j] = *reinterpret_cast<const uint4*>(Bs + row * 64 + ((fc ^ swz(row)) << 4));
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        if constexpr (sizeof(T) == 2) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[i]),
                                                              __builtin_bit_cast(bf16x8, bfr[j]), acc[i][j], 0, 0, 0);
        } else {
          const f32x4 a4 = __builtin_bit_cast(f32x4, af[i]);
          const f32x4 b4 = __builtin_bit_cast(f32x4, bfr[j]);
#pragma unroll
          for (int s = 0; s < 4; ++s) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[s], b4[s], acc[i][j], 0, 0, 0);
        }
      }
  };

  load_tile(0);
  store_tile(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) load_tile(kt + 1);
    compute(cur);
    if (kt + 1 < nk) store_tile(cur ^ 1);
    __syncthreads();
  }

  EpiPre<T, BM, BN, 4, false> pre;
  conv_epilogue<T, BM, BN, ACT ? 1 : 0>(acc, smem, g, bias, res, out, stats, m0, n0, -1, nullptr, pre, false);
}

// ============================================================================
// Fast path (bf16, K a multiple of 64 within one tap): BK = 64, an S-stage LDS
// ring filled by LDS-DMA (global_load_lds_dwordx4, 1 KiB = 8 rows x 128 B per
// wave instruction), S-1 stages in flight while one is computed; one raw
// s_barrier per K-step behind a counted vmcnt (never __syncthreads in the loop:
// its fence would drain the in-flight DMA).  Padding taps / rows past M read a
// zero page instead of being masked.  The XOR swizzle (row >> 1) & 7 is applied
// on the DMA SOURCE address (the LDS destination of LDS-DMA is lane-linear) and
// on the ds_read_b128 fragment reads: conflict-free for both 16-lane k-halves.
// S is picked per layer: deep rings for small, long-K grids (latency bound: one
// workgroup per CU, each K-step short), shallow ones for big grids (occupancy).
// ============================================================================
// Fragment reads of one k-half as ONE asm block: NR ds_read_b128 then
// lgkmcnt(0).  Written as plain C++ loads, hipcc cannot tell the ring slot being
// read from the slots the in-flight LDS-DMA is filling and emits vmcnt(0) before
// the first ds_read of every K-step, draining the whole prefetch ring (the .s
// showed it: deeper rings bought nothing).  The counted vmcnt + barrier in the
// K-loop is what orders these reads after the DMA that filled the slot.
template <int NR>
__device__ __forceinline__ void lds_read_frags(u32x4 (&f)[NR], const unsigned (&addr)[NR]) {
  static_assert(NR == 4 || NR == 6 || NR == 8, "fragment batch of 4, 6 or 8 reads");
  if constexpr (NR == 4) {
    asm volatile(
        "ds_read_b128 %0, %4\n\tds_read_b128 %1, %5\n\tds_read_b128 %2, %6\n\tds_read_b128 %3, %7\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(f[0]), "=&v"(f[1]), "=&v"(f[2]), "=&v"(f[3])
        : "v"(addr[0]), "v"(addr[1]), "v"(addr[2]), "v"(addr[3]));
  } else if constexpr (NR == 6) {
    asm volatile(
        "ds_read_b128 %0, %6\n\tds_read_b128 %1, %7\n\tds_read_b128 %2, %8\n\tds_read_b128 %3, %9\n\t"
        "ds_read_b128 %4, %10\n\tds_read_b128 %5, %11\n\ts_waitcnt lgkmcnt(0)"
        : "=&v"(f[0]), "=&v"(f[1]), "=&v"(f[2]), "=&v"(f[3]), "=&v"(f[4]), "=&v"(f[5])
        : "v"(addr[0]), "v"(addr[1]), "v"(addr[2]), "v"(addr[3]), "v"(addr[4]), "v"(addr[5]));
  } else {
    asm volatile(
        "ds_read_b128 %0, %8\n\tds_read_b128 %1, %9\n\tds_read_b128 %2, %10\n\tds_read_b128 %3, %11\n\t"
        "ds_read_b128 %4, %12\n\tds_read_b128 %5, %13\n\tds_read_b128 %6, %14\n\tds_read_b128 %7, %15\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(f[0]), "=&v"(f[1]), "=&v"(f[2]), "=&v"(f[3]), "=&v"(f[4]), "=&v"(f[5]), "=&v"(f[6]), "=&v"(f[7])
        : "v"(addr[0]), "v"(addr[1]), "v"(addr[2]), "v"(addr[3]), "v"(addr[4]), "v"(addr[5]), "v"(addr[6]),
          "v"(addr[7]));
  }
}

// Both k-halves of a 64x64 tile's fragments (2 x 4 ds_read_b128) issued as ONE asm
// batch without a wait; lds_wait_first / lds_wait_all then release them in two
// steps (counted lgkmcnt), so the second half's reads are in flight while the
// first half's MFMAs run.  The waits name the fragments as in-out operands: the
// compiler cannot hoist an MFMA that consumes them above the wait.
__device__ __forceinline__ void lds_issue_frags8(u32x4 (&f)[2][4], const unsigned (&a)[2][4]) {
  asm volatile(
      "ds_read_b128 %0, %8\n\tds_read_b128 %1, %9\n\tds_read_b128 %2, %10\n\tds_read_b128 %3, %11\n\t"
      "ds_read_b128 %4, %12\n\tds_read_b128 %5, %13\n\tds_read_b128 %6, %14\n\tds_read_b128 %7, %15"
      : "=&v"(f[0][0]), "=&v"(f[0][1]), "=&v"(f[0][2]), "=&v"(f[0][3]), "=&v"(f[1][0]), "=&v"(f[1][1]),
        "=&v"(f[1][2]), "=&v"(f[1][3])
      : "v"(a[0][0]), "v"(a[0][1]), "v"(a[0][2]), "v"(a[0][3]), "v"(a[1][0]), "v"(a[1][1]), "v"(a[1][2]),
        "v"(a[1][3]));
}
__device__ __forceinline__ void lds_wait_first(u32x4 (&f)[4]) {
  asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]));
}
__device__ __forceinline__ void lds_wait_all(u32x4 (&f)[4]) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]));
}

// one 16-byte fragment pair -> the 16x16 accumulator: bf16 = one 16x16x32 MFMA,
// fp32 = four exact 16x16x4 MFMAs (component s of every lane's chunk)
template <typename T>
__device__ __forceinline__ void mma_frag(f32x4& acc, const u32x4& a, const u32x4& b) {
  if constexpr (sizeof(T) == 2) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0,
                                                  0, 0);
  } else {
    const f32x4 a4 = __builtin_bit_cast(f32x4, a), b4 = __builtin_bit_cast(f32x4, b);
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[s], b4[s], acc, 0, 0, 0);
  }
}

// one workgroup's work; `bid_in` = its index in this conv's sub-grid (the whole grid,
// or the leading part of a fused backward launch), `smem` = the kernel's dynamic LDS
// PRE: a workgroup with at most two K-steps fetches its epilogue's global operands
// (epi_prefetch) right after issuing its operand DMA (profiles/r03t_epi_prefetch_ab.txt)
template <typename T, int BM, int BN, int MODE, int S, bool ACT = false, int NW = 4, bool BNR = false,
          bool PRE = false>
__device__ __forceinline__ void conv_lds_body(char* smem, int bid_in, const T* __restrict__ src,
                                              const T* __restrict__ wts, const float* __restrict__ bias,
                                              const T* __restrict__ res, T* __restrict__ out,
                                              float* __restrict__ stats, const Geom& g) {
  constexpr int CH = LK<T>::CH, KS = LK<T>::KS;
  static_assert(KS == 64 || KS == 32, "bf16 or fp32");
  constexpr int LOG_KS = KS == 64 ? 6 : 5;
  constexpr int WM = WaveGrid<NW>::WM;
  constexpr int TM = BM / (16 * WM), TN = BN / 32;
  constexpr int RW = 8 * NW;                        // rows one DMA instruction of every wave covers
  constexpr int A_INS = BM / RW, B_INS = BN / RW;   // DMA instructions per thread per stage
  static_assert(A_INS * RW == BM && B_INS * RW == BN, "tile rows must be a multiple of 8 x waves");
  constexpr int LOADS = A_INS + B_INS;
  constexpr int SA = BM * 128, STAGE = (BM + BN) * 128;
  static_assert(S >= 2, "ring needs two stages");

  constexpr bool SK = MODE == kGemm || MODE == kFwd || MODE == kDgrad;   // split-K capable modes
  const int nsplit = SK && g.splits > 1 ? g.splits : 1;
  const int per = g.gm * g.gn;
  const int nwg = (MODE == kDgradS2 ? s2_classes(g) * per : per) * nsplit;
  int bid = bid_in;
  {
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  // split-K: the splits of one tile are consecutive logical ids (one XCD, mostly)
  int split = 0;
  if (nsplit > 1) {
    split = bid % nsplit;
    bid /= nsplit;
  }
  const int tile_id = bid;
  // parity class (kDgradS2): the four classes of one tile are consecutive logical
  // ids, so every XCD gets an even share of the heavy and the empty classes and the
  // four blocks that gather the same dY rows run on the same L2
  constexpr bool DUAL = MODE == kGemmDual;
  int cls = -1, py = 0, px = 0, kh0 = 0, kw0 = 0, ntx = 1, nk = g.Kpad >> LOG_KS;
  const int nk1 = nk;   // kGemmDual: K-steps of the first (block) GEMM
  if (DUAL) nk += g.Kpad2 >> LOG_KS;
  if (MODE == kDgradS2) {
    if (g.s2one) {
      cls = g.s2one - 1;
    } else {
      // the four classes of tile t are logical ids 4t .. 4t+3 (one XCD, one L2), in an
      // order that rotates with t: the dispatcher deals an XCD's workgroups out to its
      // shader engines in turn, so a fixed order would give each engine one class (the
      // 4-tap class's engine doing 4/9 of the work; a 1x1's tap class on one engine;
      // profiles/r05rot_s2_class_order_ab.txt)
      cls = 3 - ((bid + (bid >> 2)) & 3);
      bid >>= 2;
    }
    py = cls >> 1; px = cls & 1;
    kh0 = (py + g.pad) & 1; kw0 = (px + g.pad) & 1;   // first tap of this parity, then every 2nd
    const int nty = (g.KH - kh0 + 1) >> 1;
    ntx = (g.KW - kw0 + 1) >> 1;
    nk = (nty * ntx) << (g.log2SC - LOG_KS);
    // a class no tap reaches (1x1 stride 2: three of four) contributes zeros: with
    // the residual accumulated in place (res == out) its pixels are already final
    if (nk == 0 && res == out) return;
  }
  // consecutive logical tiles share an XCD (remap above): M-major keeps a few A row
  // blocks + all of B in that XCD's L2
  const int tm = bid / g.gn, tn = bid - tm * g.gn;
  const int m0 = tm * BM, n0 = tn * BN;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int r8 = lane >> 3, pch = lane & 7;
  const char* zp = reinterpret_cast<const char*>(g_zero_page);

  // rows this lane DMAs: row = i*RW + wave*8 + r8; it fetches logical chunk pch ^ swz8(row)
  int a_pix[A_INS], a_y[A_INS], a_x[A_INS], a_ck[A_INS];
  int a_pix2[DUAL ? A_INS : 1];   // kGemmDual: the row's pixel in the downsample operand
  bool a_ok[A_INS];
#pragma unroll
  for (int i = 0; i < A_INS; ++i) {
    const int row = i * RW + wave * 8 + r8;
    const int m = m0 + row;
    a_ok[i] = m < g.M;
    a_ck[i] = (pch ^ swz8(row)) * CH;
    const int mm = a_ok[i] ? m : 0;
    if (MODE == kGemm || DUAL) {
      a_pix[i] = mm; a_y[i] = 0; a_x[i] = 0;
      if constexpr (DUAL) {
        const int hw = g.RH * g.RW;
        const int n = mm / hw, rem = mm - n * hw;
        const int y = rem / g.RW, x = rem - y * g.RW;
        a_pix2[i] = (n * g.SH2 + y * g.stride2) * g.SW2 + x * g.stride2;
      }
    } else {
      const int hw = g.RH * g.RW;
      const int n = mm / hw, rem = mm - n * hw;
      const int y = rem / g.RW, x = rem - y * g.RW;
      a_pix[i] = n * g.SH * g.SW;
      if (MODE == kDgrad) { a_y[i] = y + g.pad; a_x[i] = x + g.pad; }
      else if (MODE == kDgradS2) { a_y[i] = y; a_x[i] = x; }
      else if (MODE == kFwdRowTap) { a_y[i] = y * g.stride - g.pad; a_x[i] = x * g.stride - g.pad - (kRowTaps - g.KW); }
      else { a_y[i] = y * g.stride - g.pad; a_x[i] = x * g.stride - g.pad; }
    }
  }
  // B rows: n >= Ncols read the zero page (offset masked to 0)
  const T* b_base[B_INS];
  unsigned b_mask[B_INS];
#pragma unroll
  for (int j = 0; j < B_INS; ++j) {
    const int row = j * RW + wave * 8 + r8;
    const int n = n0 + row;
    const bool ok = n < g.Ncols;
    b_base[j] = ok ? wts + (int64_t)n * g.Kpad + (pch ^ swz8(row)) * CH : reinterpret_cast<const T*>(zp);
    b_mask[j] = ok ? ~0u : 0u;
  }
  // kGemmDual: the downsample weights' rows, switched to after the first GEMM's K-steps
  const T* b_base2[DUAL ? B_INS : 1];
  if constexpr (DUAL) {
#pragma unroll
    for (int j = 0; j < B_INS; ++j) {
      const int row = j * RW + wave * 8 + r8;
      const int n = n0 + row;
      b_base2[j] = n < g.Ncols ? reinterpret_cast<const T*>(g.wts2) + (int64_t)n * g.Kpad2 + (pch ^ swz8(row)) * CH
                               : reinterpret_cast<const T*>(zp);
    }
  }
  int phase = 0;   // kGemmDual: 0 = block GEMM, 1 = downsample GEMM

  // The K loop walks filter taps in order; inside a tap the 64-deep slices are
  // contiguous channels.  Row source pointers (and their validity: padding, rows
  // past M, stride-2 holes) change only at a tap boundary, so they are rebuilt
  // there (uniform branch) and each K-step only adds the channel offset c0 --
  // the per-step address arithmetic that made these kernels issue-bound at one
  // workgroup per CU.  issue() is called with consecutive kt.
  int tap_len = (MODE == kGemm || DUAL) ? g.Kpad : (MODE == kFwdRowTap ? KS : g.SC);   // row-tap: one K-step
  int c0 = 0, kh = kh0, kw = kw0, tw = 0, tap_koff = MODE == kDgradS2 ? (kh0 * g.KW + kw0) * g.SC : 0;
  const T* a_base[A_INS];
  unsigned a_mask[A_INS];
  auto set_tap = [&]() {
#pragma unroll
    for (int i = 0; i < A_INS; ++i) {
      bool ok = a_ok[i];
      int64_t off = 0;
      if (MODE == kGemm || DUAL) {
        off = (int64_t)a_pix[i] * g.K;
        if constexpr (DUAL) {
          if (phase) {
            off = (int64_t)a_pix2[i] * g.Kpad2;
            a_base[i] = ok ? reinterpret_cast<const T*>(g.src2) + off + a_ck[i] : reinterpret_cast<const T*>(zp);
            a_mask[i] = ok ? ~0u : 0u;
            continue;
          }
        }
      } else if (MODE == kFwdRowTap) {
        // K-step kh: this lane's 16-B chunk (logical chunk a_ck / CH) is kernel row kr,
        // taps 4 x2 .. (8 elements = 2 pixels bf16, 4 = 1 pixel fp32) of that row
        const int ke = kh * KS + a_ck[i];
        const int kr = ke >> 5, sy = a_y[i] + kr, sx = a_x[i] + ((ke & 31) >> 2);
        ok = ok && kr < g.KH && (unsigned)sy < (unsigned)g.SH && (unsigned)sx < (unsigned)g.SW;
        a_base[i] = ok ? src + ((int64_t)(a_pix[i] + sy * g.SW + sx) << 2) : reinterpret_cast<const T*>(zp);
        a_mask[i] = ok ? ~0u : 0u;
        continue;
      } else {
        int sy, sx;
        if (MODE == kFwd) {
          sy = a_y[i] + kh; sx = a_x[i] + kw;
        } else if (MODE == kDgradS2) {
          // dX(2yy+py) <- dY((2yy + py + pad - kh) / 2); the numerator is even by construction
          sy = a_y[i] + ((py + g.pad - kh) >> 1);
          sx = a_x[i] + ((px + g.pad - kw) >> 1);
        } else {
          const int ty = a_y[i] - kh, tx = a_x[i] - kw;
          ok = ok && ty >= 0 && tx >= 0;
          if (g.stride == 2) { ok = ok && !(ty & 1) && !(tx & 1); sy = ty >> 1; sx = tx >> 1; }
          else { sy = ty; sx = tx; }
        }
        ok = ok && (unsigned)sy < (unsigned)g.SH && (unsigned)sx < (unsigned)g.SW;
        off = (int64_t)(a_pix[i] + sy * g.SW + sx) << g.log2SC;
      }
      a_base[i] = ok ? src + off + a_ck[i] : reinterpret_cast<const T*>(zp);
      a_mask[i] = ok ? ~0u : 0u;
    }
  };

  // one stage's DMA as (source, LDS destination) pairs, then the tap walk advanced;
  // issue() fires them back to back
  const T* dsrc[LOADS];
  char* ddst[LOADS];
  auto prep = [&](int buf) {
    char* As = smem + buf * STAGE;
    char* Bs = As + SA;
    if (c0 == 0) set_tap();
    const unsigned boff = (unsigned)(tap_koff + c0);
#pragma unroll
    for (int j = 0; j < B_INS; ++j) {
      const T* bb = b_base[j];
      if constexpr (DUAL) bb = phase ? b_base2[j] : b_base[j];
      dsrc[j] = bb + (boff & b_mask[j]);
      ddst[j] = Bs + (j * RW + wave * 8) * 128;
    }
#pragma unroll
    for (int i = 0; i < A_INS; ++i) {
      dsrc[B_INS + i] = a_base[i] + ((unsigned)c0 & a_mask[i]);
      ddst[B_INS + i] = As + (i * RW + wave * 8) * 128;
    }
    c0 += KS;
    if (c0 == tap_len) {
      c0 = 0;
      if constexpr (DUAL) {
        phase = 1;
        tap_len = g.Kpad2;
        return;
      }
      if (MODE == kDgradS2) {
        kw += 2;
        if (++tw == ntx) { tw = 0; kw = kw0; kh += 2; }
        tap_koff = (kh * g.KW + kw) * g.SC;
      } else if (MODE == kFwdRowTap) {   // kh counts K-steps
        ++kh;
        tap_koff += KS;
      } else {
        if (++kw == g.KW) { kw = 0; ++kh; }
        tap_koff += g.SC;
      }
    }
  };
  auto issue = [&](int kt, int buf) {
    (void)kt;
    prep(buf);
#pragma unroll
    for (int q = 0; q < LOADS; ++q) glds16(dsrc[q], ddst[q]);
  };

  // split-K: this workgroup's K-steps [kb, ke) of the tile; the tap walk starts at kb
  if (SK && nsplit > 1) {
    const int kb = (int)((int64_t)split * nk / nsplit), ke = (int)((int64_t)(split + 1) * nk / nsplit);
    nk = ke - kb;
    if (MODE == kGemm) {
      c0 = kb << LOG_KS;
    } else {
      const int spt = g.SC >> LOG_KS;   // K-steps per filter tap
      const int tap = kb / spt;
      c0 = (kb - tap * spt) << LOG_KS;
      kh = tap / g.KW;
      kw = tap - kh * g.KW;
      tap_koff = tap * g.SC;
    }
    if (c0 != 0) set_tap();   // issue() rebuilds the row pointers only at a tap start
  }

  f32x4 acc[TM][TN];
  f32x4 acc2[DUAL ? TM : 1][DUAL ? TN : 1];   // kGemmDual: the block GEMM's sums, parked
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // per-lane fragment byte offsets inside a ring slot (row-dependent swizzle), per k-half
  const int fr = lane & 15, fc = lane >> 4;
  unsigned frag_off[2][TM + TN];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int row = wm * (BM / WM) + i * 16 + fr;
      frag_off[kk][i] = row * 128 + (((fc + 4 * kk) ^ swz8(row)) << 4);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int row = wn * (BN / 2) + j * 16 + fr;
      frag_off[kk][TM + j] = SA + row * 128 + (((fc + 4 * kk) ^ swz8(row)) << 4);
    }
  }
  const unsigned ring_base = lds_addr(smem);
  // mid(): issued between the fragment reads and their wait, so the next stage's
  // LDS-DMA issue (tens of cycles per instruction) overlaps the LDS read latency
  auto compute = [&](int buf, auto&& mid, auto& acc) {
    const unsigned slot = ring_base + buf * STAGE;
    if constexpr (TM + TN == 4) {
      unsigned addr[2][4];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int r = 0; r < 4; ++r) addr[kk][r] = slot + frag_off[kk][r];
      u32x4 f[2][4];
      lds_issue_frags8(f, addr);
      mid();
      lds_wait_first(f[0]);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        if (kk == 1) lds_wait_all(f[1]);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) mma_frag<T>(acc[i][j], f[kk][i], f[kk][TM + j]);
      }
      return;
    }
    mid();
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      unsigned addr[TM + TN];
#pragma unroll
      for (int r = 0; r < TM + TN; ++r) addr[r] = slot + frag_off[kk][r];
      u32x4 f[TM + TN];
      lds_read_frags<TM + TN>(f, addr);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) mma_frag<T>(acc[i][j], f[i], f[TM + j]);
    }
  };

  // prologue: stages 0 .. S-2 in flight; step kt refills the buffer step kt-1 read
  for (int s = 0; s < S - 1 && s < nk; ++s) issue(s, s);
  // early epilogue fetch (PRE): younger than the prologue DMA, so the loop's counted
  // waits (which count DMA only) over-wait it on the first step -- correct, and with
  // one or two K-steps the two sets of loads are in flight together
  EpiPre<T, BM, BN, NW, BNR> pre;
  const bool early = PRE && !DUAL && nk <= 2;
  if (early) epi_prefetch<T, BM, BN, ACT ? 1 : 0, NW, BNR>(pre, g, res, m0, n0, cls);
  int cur = 0, wbuf = S - 1;
  for (int kt = 0; kt < nk; ++kt) {
    const int left = nk - 1 - kt;
    wait_ahead<LOADS, S - 2>(left < S - 2 ? left : S - 2);   // stage kt landed, for every wave
    auto mid = [&]() {
      if (kt + S - 1 < nk) issue(kt + S - 1, wbuf);
    };
    if constexpr (DUAL) {
      // the block GEMM is complete: park its sums, accumulate the downsample afresh
      // (one accumulator set in the loop keeps the register budget of the plain kernel)
      if (kt == nk1) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            acc2[i][j] = acc[i][j];
            acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
      }
    }
    compute(cur, mid, acc);
    cur = cur == S - 1 ? 0 : cur + 1;
    wbuf = wbuf == S - 1 ? 0 : wbuf + 1;
  }
  asm volatile("s_barrier" ::: "memory");   // every wave done reading the ring before the epilogue reuses it
  if constexpr (SK) {
    if (nsplit > 1 && !splitk_merge<TM, TN, NW>(acc, smem, tile_id, split, nsplit, g.sk_cnt, g.sk_part)) return;
  }
  if constexpr (DUAL)   // acc2 = the block GEMM, acc = the downsample branch
    conv_epilogue<T, BM, BN, 1, NW, true>(acc2, smem, g, bias, nullptr, out, nullptr, m0, n0, -1, acc, pre, false);
  else
    conv_epilogue<T, BM, BN, ACT ? 1 : 0, NW, false, BNR>(acc, smem, g, bias, res, out, stats, m0, n0, cls, nullptr,
                                                          pre, early);
}

// BNR: data gradient with the BatchNorm-reduce epilogue (its own instance: the
// forward 1x1 kernels, kGemm too, keep their register budget)
template <typename T, int BM, int BN, int MODE, int S, bool ACT, int NW, bool BNR = false>
__global__ __launch_bounds__(64 * NW) void conv_lds_kernel(const T* __restrict__ src, const T* __restrict__ wts,
                                                           const float* __restrict__ bias, const T* __restrict__ res,
                                                           T* __restrict__ out, float* __restrict__ stats, Geom g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  conv_lds_body<T, BM, BN, MODE, S, ACT, NW, BNR>(smem, blockIdx.x, src, wts, bias, res, out, stats, g);
}

#include "conv_patch.h"

// Fused backward of one conv.  Both passes read the same dY, and the weight-
// gradient workgroups fill the CUs the (often small) data-gradient grid leaves idle
// -- one launch instead of two.  Workgroup order = the order the dispatcher starts
// them, longest work first (`wfirst`, chosen per conv by launch_bwd): with wfirst,
// [0, nw) the weight gradient, [nw_pad, nw_pad + nd) the data gradient, else the data
// gradient [0, nd) and the weight gradient [nd_pad, nd_pad + nw); the carried slab
// reduce last.  (nw_pad / nd_pad round up to 8 so each part's XCD remap stays intact;
// the padding workgroups exit at once.)  The weight-gradient workgroups of a 1x1
// conv run ~10 K-steps; dispatched behind thousands of one- to four-step data-
// gradient workgroups they were the launch's tail.
// T = float: the same launch for the reference-precision (fp32) step -- the fp32
// LDS-DMA data gradient and the fp32 LDS-DMA weight gradient (wgrad_body.h).
// pixels per fp32 64x64 weight-gradient stage in the fused launch: 32 (with fused_ds's
// 3-slot data-gradient ring) fits three workgroups per CU (profiles/r05f32r_bwd_ring_ab.txt)
constexpr int kBwdF32MS = 32;
// WBT (fp32 only): the weight-gradient tile, 64 or 128 (the wider KxK convs' plans: 128x128
// on 32-pixel stages, conv_wgrad_lds_body_f32)
template <int DMODE, int DS, int WS, typename T = bf16, int WBT = 64>
__global__ __launch_bounds__(kThreads) void conv_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ wt,
                                                            const T* __restrict__ dres, T* __restrict__ dx,
                                                            Geom gd, int nd, int nd_pad, int wfirst,
                                                            const T* __restrict__ x, float* __restrict__ ws,
                                                            p6::WGeom gw, ReduceJob rj) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int b = blockIdx.x;
  const int nw = gw.gm * gw.gn * gw.splits;
  const int nw_pad = (nw + 7) & ~7;
  const int d0 = wfirst ? nw_pad : 0;                  // first data-gradient workgroup
  const int w0 = wfirst ? 0 : nd_pad;                  // first weight-gradient workgroup
  const int r0 = wfirst ? nw_pad + nd : nd_pad + nw;   // first reduce workgroup (last: they fill the tail)
  if (b >= d0 && b < d0 + nd) {
    conv_lds_body<T, 64, 64, DMODE, DS, false, 4, true, true>(smem, b - d0, dy, wt, nullptr, dres, dx, nullptr, gd);
  } else if (b >= w0 && b < w0 + nw) {
    // kGemm data gradient <=> pointwise conv: the weight gradient takes the pointwise body
    if constexpr (sizeof(T) == 2)
      conv_wgrad_lds_body<64, 64, WS, DMODE == kGemm>(smem, b - w0, x, dy, ws, gw);
    else if constexpr (WBT == 128)
      conv_wgrad_lds_body_f32<32, WS, DMODE == kGemm, 128>(smem, b - w0, x, dy, ws, gw);
    else
      conv_wgrad_lds_body_f32<kBwdF32MS, WS, DMODE == kGemm>(smem, b - w0, x, dy, ws, gw);
  } else if (b >= r0) {
    // the previous conv's weight-gradient slabs (another workspace), reduced here
    // instead of in a launch of their own
    run_reduce_job(smem, b - r0, rj);
  }
}

// The 8-wave form of the fused backward for the bf16 weight gradients on 128x128 tiles
// (wgrad_body.h, NW = 8: twice the MACs per staged byte of the 64x64 tile; the KxK
// convs' plans, conv_wgrad.hip): the data gradient runs on 128x64 tiles of 8 waves in
// the same launch, the carried slab reduce on the first four waves of its workgroups
// (the other four only meet its one barrier).
template <int DMODE, int DS, int WS>
__global__ __launch_bounds__(2 * kThreads) void conv_bwd8_kernel(const bf16* __restrict__ dy,
                                                                  const bf16* __restrict__ wt,
                                                                  const bf16* __restrict__ dres, bf16* __restrict__ dx,
                                                                  Geom gd, int nd, int nd_pad, int wfirst,
                                                                  const bf16* __restrict__ x, float* __restrict__ ws,
                                                                  p6::WGeom gw, ReduceJob rj) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int b = blockIdx.x;
  const int nw = gw.gm * gw.gn * gw.splits;
  const int nw_pad = (nw + 7) & ~7;
  const int d0 = wfirst ? nw_pad : 0;
  const int w0 = wfirst ? 0 : nd_pad;
  const int r0 = wfirst ? nw_pad + nd : nd_pad + nw;
  if (b >= d0 && b < d0 + nd) {
    conv_lds_body<bf16, 128, 64, DMODE, DS, false, 8, true, true>(smem, b - d0, dy, wt, nullptr, dres, dx, nullptr,
                                                                  gd);
  } else if (b >= w0 && b < w0 + nw) {
    conv_wgrad_lds_body<128, 128, WS, DMODE == kGemm, false, 8>(smem, b - w0, x, dy, ws, gw);
  } else if (b >= r0) {
    if (threadIdx.x < kThreads) run_reduce_job(smem, b - r0, rj);
    else __syncthreads();   // the reduce body's one workgroup barrier
  }
}

}  // namespace
