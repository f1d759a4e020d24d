// Launch planning of the implicit-GEMM convolution, host only: the GEMM geometry of a
// ConvShape, the plan (kernel, tile, ring, split-K) of a forward / data gradient and of
// a whole backward.  Included by conv_igemm.hip after conv_kernels.h (the patch plan of
// conv_patch.h).
#pragma once
#include "conv_geom.h"
#include "wgrad_body.h"

namespace {

// K-steps of the longest work item (kDgradS2: the class with the most taps);
// ks = elements per K-step (64 bf16, 32 fp32)
int fast_nk(int mode, const Geom& g, int ks = 64) {
  if (mode == kGemmDual) return (g.Kpad + g.Kpad2) / ks;
  if (mode != kDgradS2) return g.Kpad / ks;
  int best = 0;
  for (int cls = 0; cls < 4; ++cls) {
    const int kh0 = ((cls >> 1) + g.pad) & 1, kw0 = ((cls & 1) + g.pad) & 1;
    const int t = ((g.KH - kh0 + 1) >> 1) * ((g.KW - kw0 + 1) >> 1);
    best = t > best ? t : best;
  }
  return best * g.SC / ks;
}

// tile choice: the biggest tile that still gives >= 2 waves of workgroups per CU-pass
int pick_tile(int M, int N) {
  auto blocks = [&](int bm, int bn) { return (int64_t)p6::ceil_div(M, bm) * p6::ceil_div(N, bn); };
  if (N <= 64) return blocks(128, 64) >= 512 ? 1 : 3;
  if (blocks(128, 128) >= 512) return 0;
  if (blocks(128, 64) >= 512) return 1;
  if (blocks(64, 128) >= 512) return 2;
  return 3;
}

// implementation choice: the LDS-DMA fast path whenever each 128-byte K slice (64
// bf16 / 32 fp32 channels) lies inside one filter tap; the register-staged kernel
// otherwise (the Cin-4 stem, the 3- and 32-channel z-CNN layers).  A pose6d_tuning_t
// (the *_tuned entry points: tests and tools/conv_bench.py only) can force the
// register-staged kernel, a tile, a ring depth or the masked stride-2 gather; the
// product entry points never take one, so each conv has one plan (one summation order).
bool fast_ok(int dtype, int mode, const Geom& g) {
  if (mode == kFwdNarrow) return false;
  if (mode == kFwdRowTap) return true;   // its only path (fwd_geom checked the geometry)
  if (mode == kGemmDual) {
    const int ks2 = dtype == POSE6D_DT_BF16 ? 64 : 32;
    return g.K % ks2 == 0 && g.Kpad == g.K && g.Kpad2 % ks2 == 0;
  }
  const int ks = dtype == POSE6D_DT_BF16 ? 64 : 32;   // elements per 128-byte K-step
  if (g.K % ks != 0 || g.Kpad != g.K) return false;
  return mode == kGemm || g.SC % ks == 0;
}

// Tile per GEMM shape.  The 64x64 / 4-wave tile keeps the most workgroups resident
// and wins while K is short or the grid would get thin; a 128x128 tile on 8 waves
// (tile 4) halves the LDS-DMA bytes per MFMA (each 32 KiB stage feeds four times
// the MACs of a 16 KiB one), which wins inside the training step once K >= 256 and
// the grid keeps >= 384 workgroups (layer2.0 ds / conv1, layer3.0 ds / conv1,
// layer3 conv3: 1-3 us each).  128x64 on 8 waves (tile 5) won standalone sweeps
// (tools/conv_bench.py) but lost in the step, so bf16 never picks it.  fp32
// (MFMA-bound: 4x the MFMAs per byte) takes 128x128 on long K at about one
// workgroup per CU (profiles/r02_conv_tiles.txt).
// the bf16 128x128 tile's minimum K: 128 puts layer2's 128 -> 512 convs on it
// (profiles/r04_tile4_k128_ab.txt)
constexpr int kTile4MinK = 128;
int pick_tile_fast(int dtype, int64_t M, int N, int K) {
  const int64_t wg4 = p6::ceil_div(M, 128) * (int64_t)p6::ceil_div(N, 128);
  if (dtype == POSE6D_DT_F32) return (K >= 512 && N >= 128 && wg4 >= 192 && wg4 < 384) ? 4 : 3;
  return (N >= 128 && K >= kTile4MinK && wg4 >= 384) ? 4 : 3;
}

using p6::tuned;

// a tile code's extent: 0 = 128x128, 1 = 128x64, 3 = 64x64 (4 waves); 4 = 128x128,
// 5 = 128x64 (8 waves)
struct TileDims {
  bool rows128, cols128;
  int bm() const { return rows128 ? 128 : 64; }
  int bn() const { return cols128 ? 128 : 64; }
};
TileDims tile_dims(int tile) { return {tile <= 1 || tile == 4 || tile == 5, tile == 0 || tile == 4}; }

struct Plan {
  bool fast;
  int mode, tile, stages;
  Geom g;
};

// stride-2 data gradient as four parity classes: needs every dX pixel's class to
// have the same extent (H, W even; Ho = H / 2, Wo = W / 2)
bool s2_ok(const Geom& g) {
  return g.stride == 2 && (g.RH & 1) == 0 && (g.RW & 1) == 0 && g.SH == g.RH / 2 && g.SW == g.RW / 2;
}

// Default split-K count of a FORWARD conv (data gradients keep one split, so the fused
// backward launch and the separate data-gradient launch stay bit-identical): a function
// of the geometry only (never of a tuned tile or
// ring depth, so every tile / ring variant of a plan keeps one summation order).
// Split-K pays where a long K loop runs on a grid of at most one 64x64 workgroup per
// CU: layer4's 3x3 convs (72 K-steps, 200 tiles at batch 32: 23.2 -> 18.6 us forward,
// 23.5 -> 18.6 us data gradient, graph-replayed) and its 2048->512 1x1 (32 K-steps:
// 12.7 -> 11.9 us); fp32 the same shapes (32-channel K-steps): 90.1 -> 84.8, 43.7 -> 40.9
// and 95.2 -> 83.7 us (profiles/r04_f32_conv_sweep.txt).  Everywhere else the merge (write-through partial stores, the
// arrival atomic, the partial reads: ~3-5 us on the last arriver's critical path)
// costs more than the shorter K loop saves (profiles/r04_splitk_sweep.txt).
// grids of at most this many 64x64 tiles with >= 16 K-steps split K four ways
// (profiles/r06_b1_splitk.txt)
constexpr int kSplitkSmallTiles = 64;
int default_splits(int dtype, int mode, const Geom& g, bool fused) {
  if (fused || !(mode == kGemm || mode == kFwd || mode == kDgrad)) return 1;
  const int ks = dtype == POSE6D_DT_BF16 ? 64 : 32;
  const int nk = fast_nk(mode, g, ks);
  const int64_t tiles64 = (int64_t)p6::ceil_div(g.M, 64) * p6::ceil_div(g.Ncols, 64);
  // small grids (batch 1-2: at most a quarter of the CUs busy) with >= 16 K-steps: four
  // shorter K walks per tile (B = 1 eval forwards 7.7 -> 7.1 us on 14x14 1024->256, 14.4 ->
  // 10.6 us on layer4's 3x3; profiles/r06_b1_splitk.txt); no batch-32 conv has <= 64 tiles
  if (nk >= 16 && tiles64 <= kSplitkSmallTiles) return 4;
  if (nk >= 32 && tiles64 <= 256) return 2;
  return 1;
}

// fused = the data-gradient half of conv_bwd_kernel (its workgroups are 64x64 / 4 waves)
Plan choose(int dtype, int mode, const Geom& g, bool fused = false, const pose6d_tuning_t* tn = nullptr,
            bool fwd = false) {
  Plan p{};
  p.fast = fast_ok(dtype, mode, g) && tuned(tn, &pose6d_tuning_t::conv_base, 0) == 0;
  p.mode = mode;
  p.g = g;
  if (!p.fast) {
    p.tile = tuned(tn, &pose6d_tuning_t::conv_tile, pick_tile(g.M, g.Ncols));
    if (p.tile > 3) p.tile = 3;
    return p;
  }
  if (mode == kDgrad && s2_ok(g) && tuned(tn, &pose6d_tuning_t::conv_s2, 1)) {
    p.mode = kDgradS2;
    p.g.M = g.M / 4;
    p.g.RH = g.RH / 2;
    p.g.RW = g.RW / 2;
  }
  int dflt_tile = pick_tile_fast(dtype, p.g.M, g.Ncols, g.K);
  // long-K 1x1 forwards on the small grids (layer3 / layer4 at batch 32, M <= 6272): 8-wave
  // tiles on a 4-slot ring -- 128x128 where that still gives >= 96 workgroups, else
  // 128x64.  In-graph eval times (profiles/r05b_eval_variants.txt): 1024->256 16.0 ->
  // 11.0 us, 1024->512 18.9 -> 15.9, 1024->2048/s2 17.5 -> 15.2, 2048->512 12.9 -> 12.3
  const bool long1x1 = fwd && dtype == POSE6D_DT_BF16 && g.KH == 1 && g.KW == 1 && g.K >= 1024 && p.g.M <= 6272;
  if (long1x1) {
    const int64_t wg4 = (int64_t)p6::ceil_div(p.g.M, 128) * p6::ceil_div(g.Ncols, 128);
    dflt_tile = (g.Ncols >= 512 && wg4 >= 96) ? 4 : 5;
  }
  // fp32 KxK stride-2 data gradients (four parity classes of 1-4 taps): 64x64 tiles on a
  // 4-slot ring -- graph-timed 56x56 128->128 114.6 -> 94.1, 28x28 256->256 97.1 -> 92.0,
  // 14x14 512->512 165.0 -> 111.7 us (profiles/r05s2st_f32_s2_dgrad_plan.txt)
  const bool f32s2 = dtype == POSE6D_DT_F32 && p.mode == kDgradS2 && !fused && (g.KH > 1 || g.KW > 1);
  if (f32s2) dflt_tile = 3;
  p.tile = (fused || mode == kGemmDual) ? 3 : tuned(tn, &pose6d_tuning_t::conv_tile, dflt_tile);
  if (p.tile == 2 || p.tile < 0 || p.tile > 5) p.tile = 3;   // no 64x128 instance on the fast path
  // two slots (32 KiB at 64x64) keep several workgroups per CU resident, which hides
  // the DMA latency better than a deeper ring; only long-K grids that leave CUs
  // idle (one wave of workgroups) take a 4-deep ring
  const TileDims td = tile_dims(p.tile);
  const int64_t tiles = (int64_t)p6::ceil_div(p.g.M, td.bm()) * p6::ceil_div(g.Ncols, td.bn());
  const int64_t grid = tiles * (p.mode == kDgradS2 ? 4 : 1);
  const int nk = fast_nk(p.mode, p.g, dtype == POSE6D_DT_BF16 ? 64 : 32);
  int dflt = (nk > 24 && grid <= 512) ? 4 : 2;
  // fp32 forward (MFMA-bound: 4 exact 16x16x4 MFMAs per 16-byte chunk): 3 slots for
  // 1x1 filters, 2 for the rest (tools/conv_bench.py --graph --dtype f32 sweep, round 2)
  if (dtype == POSE6D_DT_F32 && (p.mode == kGemm || p.mode == kFwd)) dflt = (g.KH == 1 && g.KW == 1) ? 3 : 2;
  if (long1x1 || f32s2) dflt = 4;
  p.stages = tuned(tn, &pose6d_tuning_t::conv_stages, dflt);
  if (p.stages < 2) p.stages = 2;
  if (p.stages > 6) p.stages = 6;
  if (p.stages == 5) p.stages = 4;
  if (td.cols128 && td.rows128 && p.stages > 4) p.stages = 4;   // 6 x 32 KiB exceeds the 160 KiB LDS
  if (fused && p.stages == 3) p.stages = 4;   // the fused backward instantiates 2- and 4-slot data gradients
  // forwards split by default; data gradients only under an explicit tuning (tests, tools):
  // the backward entry points take no split-K workspace, and the fused and separate data
  // gradients stay one plan (one summation order)
  p.g.splits = tuned(tn, &pose6d_tuning_t::conv_splitk, fwd ? default_splits(dtype, p.mode, p.g, fused) : 1);
  if (fused || !(p.mode == kGemm || p.mode == kFwd || p.mode == kDgrad) || p.g.splits < 1) p.g.splits = 1;
  if (tiles > kSkMaxTiles) p.g.splits = 1;
  if (p.g.splits > nk) p.g.splits = nk > 0 ? nk : 1;
  // split-K plans keep their long-K ring depth (the sweep's fastest: 4 slots) unless tuned
  if (p.g.splits > 1 && tuned(tn, &pose6d_tuning_t::conv_stages, -1) < 0 && p.stages < 4 &&
      !(td.cols128 && td.rows128))
    p.stages = 4;
  return p;
}

// 2 ring slots: deeper rings measured slower (graph-timed, profiles/r05d_patch_sweep.txt:
// 56x56 64->64 17.8 / 23.5 / 25.1 us at 2 / 3 / 6 slots)
constexpr int kPatchStages = 2;
// the patch plan applies to bf16 3x3 / stride 1 / pad 1 forwards with 64-channel
// slices and no BatchNorm statistics, unless a tuning forces an implicit-GEMM plan
// (tile / ring / kernel / split-K) or turns it off (conv_patch = 0)
bool patch_eligible(int dtype, int mode, const Geom& g, const float* stats, const pose6d_tuning_t* tn,
                    PatchPlan* pp) {
  if (dtype != POSE6D_DT_BF16 || mode != kFwd || stats != nullptr) return false;
  if (g.KH != 3 || g.KW != 3 || g.stride != 1 || g.pad != 1 || g.SH != g.RH || g.SW != g.RW) return false;
  if (g.SC % 64 != 0 || g.Ncols % kPatchBN != 0 || g.Kpad != g.K || g.act_rscale != nullptr) return false;
  if (tn) {
    if (tn->conv_patch == 0) return false;
    if (tn->conv_patch < 0 && (tn->conv_tile >= 0 || tn->conv_stages >= 0 || tn->conv_base >= 0 ||
                               tn->conv_splitk >= 0))
      return false;
    if (tn->conv_patch == 1 && (tn->conv_tile >= 0 || tn->conv_base >= 0 || tn->conv_splitk >= 0))
      return false;
  }
  // the 56x56 stage only: in the eval graph the layer1 3x3 convs gain 1.7-2.5 us each,
  // the 28x28 ones lose 0.5-0.7 us (profiles/r05e_eval_layers.txt), and on 14x14 / 7x7
  // (few tiles per image, long K) the implicit GEMM is faster (profiles/r05d_patch_sweep.txt:
  // 17.7 vs 18.3 us, 19.1 vs 48.2 us)
  if (g.RH * g.RW < 3136 && !(tn && tn->conv_patch == 1)) return false;
  *pp = patch_plan(g.M / (g.RH * g.RW), g.RH, g.RW, g.SC, g.Ncols, kPatchStages);
  return pp->ok;
}

// bytes of split-K workspace a plan needs (0: it does not split K)
int64_t splitk_need(const Plan& p) {
  if (!p.fast || p.g.splits <= 1) return 0;
  const int bm = tile_dims(p.tile).bm(), bn = tile_dims(p.tile).bn();
  const int64_t tiles = (int64_t)p6::ceil_div(p.g.M, bm) * p6::ceil_div(p.g.Ncols, bn);
  return kSkCntBytes + tiles * p.g.splits * bm * bn * 4;
}

// Packed filter layout of a forward conv (the wp operand): taps per kernel row (KW, or
// kRowTaps for the row-tap stems) and the padded K, a multiple of the K-step of every
// kernel that reads it.  pose6d_conv_pack_geom exports it.
int pack_geom(int dtype, int Cin, int KH, int KW, int stride, int pad, int* kwp) {
  const bool rowtap = p6::rowtap_geom(Cin, KH, KW, stride, pad);
  *kwp = rowtap ? kRowTaps : KW;
  const int ks = dtype == POSE6D_DT_BF16 ? 64 : 32;   // LDS-DMA K-step
  const int bk = rowtap ? ks : (dtype == POSE6D_DT_BF16 ? 32 : 16);
  return p6::ceil_div(KH * *kwp * Cin, bk) * bk;
}

bool is_gemm(const ConvShape& c) { return c.KH == 1 && c.KW == 1 && c.stride == 1 && c.pad == 0; }

Geom fwd_geom(int dtype, const ConvShape& c, int* mode) {
  Geom g{};
  int kwp = 0;
  g.M = c.N * c.Ho * c.Wo; g.Ncols = c.Cout;
  g.Kpad = pack_geom(dtype, c.Cin, c.KH, c.KW, c.stride, c.pad, &kwp);
  g.K = kwp == kRowTaps ? g.Kpad : c.KH * c.KW * c.Cin;
  g.SH = c.H; g.SW = c.W; g.SC = c.Cin; g.log2SC = ilog2(c.Cin); g.RH = c.Ho; g.RW = c.Wo;
  g.KH = c.KH; g.KW = c.KW; g.stride = c.stride; g.pad = c.pad;
  if (is_gemm(c)) *mode = kGemm;
  else if (kwp == kRowTaps) *mode = kFwdRowTap;
  else if (c.Cin == 4) *mode = kFwdNarrow;
  else *mode = kFwd;
  return g;
}

Geom dgrad_geom(const ConvShape& c, int* mode) {
  Geom g{};
  g.M = c.N * c.H * c.W; g.Ncols = c.Cin; g.K = c.KH * c.KW * c.Cout; g.Kpad = g.K;
  g.SH = c.Ho; g.SW = c.Wo; g.SC = c.Cout; g.log2SC = ilog2(c.Cout); g.RH = c.H; g.RW = c.W;
  g.KH = c.KH; g.KW = c.KW; g.stride = c.stride; g.pad = c.pad;
  *mode = is_gemm(c) ? kGemm : kDgrad;
  return g;
}

// BatchNorm-reduce partial rows of a data-gradient plan: one per output tile (x the four
// parity classes of kDgradS2)
// (0: a register-staged plan, which has no BN-reduce epilogue)
int bnr_plan_rows(const Plan& p) {
  if (!p.fast) return 0;
  return p6::ceil_div(p.g.M, tile_dims(p.tile).bm()) * (p.mode == kDgradS2 ? 4 : 1);
}

int check_bnr(const pose6d_bn_reduce_t* b, const Plan& p, const void* dres, const void* dx) {
  if (!b) return POSE6D_OK;
  P6_CHECK_ARG(b->y && b->mean && b->invstd && b->partial, "pose6d_bn_reduce_t: null y / mean / invstd / partial");
  P6_CHECK_ARG(b->relu_mask || (b->relu_scale && b->relu_shift),
               "pose6d_bn_reduce_t: needs relu_mask or relu_scale + relu_shift");
  P6_CHECK_ARG(!b->y2 || (b->relu_mask && b->mean2 && b->invstd2 && b->partial2),
               "pose6d_bn_reduce_t: a second BatchNorm needs relu_mask, mean2, invstd2, partial2");
  P6_CHECK_ARG(dres != dx, "pose6d_bn_reduce_t: the data gradient must be written whole (no in-place residual)");
  P6_CHECK_ARG(p.fast, "pose6d_bn_reduce_t: this data gradient runs the register-staged kernel (no BN reduce)");
  P6_CHECK_ARG(b->rows == bnr_plan_rows(p), "pose6d_bn_reduce_t: rows %d != %d (pose6d_conv2d_backward_bn_rows)",
               b->rows, bnr_plan_rows(p));
  return POSE6D_OK;
}

// data-gradient ring depth of the fused launch for a plan of `stages` slots: fp32 plans
// of 4 run 3, so that with the 32-pixel weight-gradient stages (kBwdF32MS) the launch
// fits 48 KiB of LDS and three workgroups per CU (its VGPR budget allows three) -- the
// fp32 step 12.19 -> 11.94 ms against 4 slots and 64-pixel stages (64 KiB, two per CU;
// profiles/r05f32r_bwd_ring_ab.txt)
// the bf16 fused data-gradient ring for 4-slot plans stays 4 (profiles/r05bfr_bf16_bwd_ring_ab.txt)
constexpr int kBwdBf16DS4 = 4;
int fused_ds(int dtype, int stages) {
  if (stages <= 2) return stages;
  return dtype == POSE6D_DT_F32 ? 3 : kBwdBf16DS4;
}

bool bwd_fused(int dtype, const Plan& pd, const p6::WgradPlan& pw, const pose6d_tuning_t* tn) {
  // the fused kernels carry the 64x64 weight-gradient bodies (conv_bwd_kernel) and the
  // bf16 128x128 one (conv_bwd8_kernel: its data gradient on 128x64 tiles of 8 waves)
  if (!pd.fast || pd.tile != 3 || !(pd.stages == 2 || pd.stages == 4) || !pw.fast) return false;
  if (tuned(tn, &pose6d_tuning_t::bwd_separate, 0) != 0) return false;
  if (pw.bm == 128 && dtype == POSE6D_DT_BF16) return pw.stages == 2 || pw.stages == 3;
  if (pw.bm == 128) return pw.stages == p6::kWgradStagesF32;   // fp32 KxK, 128x128
  return pw.bm == 64 && pw.stages == (dtype == POSE6D_DT_BF16 ? p6::kWgradStages : p6::kWgradStagesF32);
}

// the data-gradient plan a fused launch runs: the bf16 8-wave launch (128x128 weight-
// gradient tiles) takes 128x64 data-gradient tiles of 8 waves (tile 5), which also sets
// the BatchNorm-reduce partial rows (bnr_plan_rows); the fp32 launch keeps the plan's tile
Plan fused_dplan(int dtype, const Plan& pd, const p6::WgradPlan& pw) {
  Plan q = pd;
  if (dtype == POSE6D_DT_BF16 && pw.bm == 128) q.tile = 5;
  return q;
}

// The whole backward of one conv, planned once: the launch (conv_backward_impl) and the
// size / variant queries (pose6d_bwd_variant, pose6d_conv2d_backward_bn_rows) read this.
struct BwdPlan {
  p6::WgradPlan pw;
  p6::WGeom gw;
  bool direct;   // one split of a 1x1 conv whose K is exactly Cin: the slab [Cout][Cin] IS the OIHW dW
  bool dgrad;    // Cin is a power of two >= 8: the conv has a data gradient (else only the above are set)
  Plan pd;       // the data gradient as the fused launch's rule sees it (choose(..., fused = true))
  bool fused;    // data and weight gradient run as ONE launch
  Plan run;      // the data-gradient plan that really runs: fused_dplan, or the separate launch's plan
  int bn_rows;   // BatchNorm-reduce partial rows of `run` (pose6d_bn_reduce_t::rows)
};

BwdPlan plan_backward(int dtype, const ConvShape& c, const pose6d_tuning_t* tn) {
  BwdPlan b{};
  b.gw = p6::wgrad_geom(dtype, c, &b.pw, tn);
  b.direct = b.gw.splits == 1 && c.KH == 1 && c.KW == 1 && b.gw.Kpad == c.Cin;
  b.dgrad = c.Cin % 8 == 0 && ilog2(c.Cin) >= 3;
  if (!b.dgrad) return b;
  int mode;
  const Geom gd = dgrad_geom(c, &mode);
  b.pd = choose(dtype, mode, gd, true, tn);
  b.fused = bwd_fused(dtype, b.pd, b.pw, tn);
  b.run = b.fused ? fused_dplan(dtype, b.pd, b.pw) : choose(dtype, mode, gd, false, tn);
  b.bn_rows = bnr_plan_rows(b.run);
  return b;
}

}  // namespace
