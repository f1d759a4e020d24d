// What the host and the device code of the implicit-GEMM convolution share
// (conv_kernels.h, conv_plan.h, conv_igemm.hip; ConvShape and ilog2 also conv_wgrad.hip).
#pragma once
#include "common.h"

namespace p6 {
// one convolution's shape, in the order the C entry points take it
struct ConvShape { int N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo; };

// log2 of a power of two, -1 otherwise
inline int ilog2(int v) {
  int r = 0;
  while ((1 << r) < v) ++r;
  return (1 << r) == v ? r : -1;
}

}  // namespace p6

namespace {

using p6::ConvShape, p6::ilog2;

template <typename T> struct KT;
template <> struct KT<bf16> { static constexpr int VEC = 8; static constexpr int BK = 32; };
template <> struct KT<float> { static constexpr int VEC = 4; static constexpr int BK = 16; };

// kDgradS2: stride-2 data gradient split into the four output parity classes
// (y & 1, x & 1); each class only gathers the taps that reach it, so no MAC is
// spent on the zeros a masked stride-2 gather would multiply.
// kGemmDual (eval only): a bottleneck's last 1x1 conv and its downsample branch in one
// launch -- K-steps [0, Kpad) are the block's 1x1 GEMM over src, the rest the 1x1
// (stride2) downsample over src2 with weights wts2, summed into a second accumulator
// set; the epilogue applies both BatchNorms exactly as the separate launches did.
enum Mode { kGemm = 0, kFwd = 1, kFwdNarrow = 2, kDgrad = 3, kDgradS2 = 4, kGemmDual = 5, kFwdRowTap = 6 };

// Row-tap forward (kFwdRowTap: the 4-channel stems, 7x7 / stride 2 / pad 3; layout in
// common.h): the filter packed with kRowTaps taps per kernel row and a zero tap in front
// (pose6d_conv_pack_geom), so the 8 taps x 4 channels of one kernel row of one output
// pixel are 8 consecutive input pixels -- 64 contiguous bytes (bf16) starting at an
// even pixel (2 ox - pad - 1): the LDS-DMA A tile fetches them as four aligned 16-B
// chunks (fp32: one kernel row per 128-B K-step row).  Replaces the register-staged
// 8-byte gather of kFwdNarrow for these convs.
using p6::kRowTaps;

struct Geom {
  int M, Ncols, K, Kpad;   // GEMM dims; Kpad = weight row length
  int SH, SW, SC, log2SC;  // gathered source tensor (NHWC)
  int RH, RW;              // row grid: m = (n * RH + y) * RW + x
  int KH, KW, stride, pad;
  int gm, gn;              // grid in tiles
  int s2one;               // kDgradS2: 0 = grid covers the four parity classes; c + 1 = only class c
  // forward with the BatchNorm already known (eval): the epilogue stores
  // act(T(y) * scale + shift [+ res | + res * res_scale + res_shift]) instead of y
  // (pose6d_conv2d_fwd_act); `res` is then the residual tensor
  const float *act_scale, *act_shift, *act_rscale, *act_rshift;
  int act, act_relu;
  // data gradient: the residual contribution is res * mask (one bit per element, one
  // byte per 16-byte chunk: pose6d_bn_act_fwd_mask's ReLU bits), i.e. the masked dout
  // of the block's last BN, instead of a materialised dz (null = res as is)
  const uint8_t* res_mask;
  // kGemmDual: the downsample operand [N][SH2][SW2][Kpad2], its packed weights
  // [Ncols][Kpad2], its stride (rows m = (n, oy, ox) of the RH x RW output grid)
  const void* src2;
  const void* wts2;
  int Kpad2, SH2, SW2, stride2;
  // data gradient that completes a BatchNorm's output gradient (pose6d_bn_reduce_t):
  // the epilogue also sums that BN's dz = dX * relu and dz * xhat per channel over its
  // tile into partial row bnr_rows-major [2][C][bnr_rows] (null bnr_part = off)
  const void* bnr_y;
  const float *bnr_mean, *bnr_inv, *bnr_rs, *bnr_rb;
  const uint8_t* bnr_mask;
  float* bnr_part;
  const void* bnr_y2;
  const float *bnr_mean2, *bnr_inv2;
  float* bnr_part2;
  int bnr_rows;
  // split-K (LDS-DMA path, kGemm / kFwd / kDgrad): each output tile's K-steps are
  // divided over `splits` workgroups (0 or 1 = none); see splitk_merge.  sk_cnt /
  // sk_part: the caller's split-K workspace (arrival counters, partial tiles)
  int splits;
  int* sk_cnt;
  float* sk_part;
};

// ---------------------------------------------------------------------------
// Split-K inside one launch.  The small-grid layers (layer3/4 at batch 32: a few
// hundred 64x64 tiles, 16-72 K-steps each) are bound by the operand bytes a CU
// keeps in flight, not by MFMA: bigger tiles move fewer bytes per MAC but leave CUs
// idle unless the K range of a tile is shared by several workgroups.  Each split
// writes its fp32 partial tile write-through (buffer stores with sc1), waits for
// them (vmcnt(0)), and after a workgroup barrier one lane adds 1 to the tile's
// arrival counter (agent scope); the workgroup whose add returns splits-1 is the
// last: it re-arms the counter, reads the other partials with sc1 buffer loads
// (after a barrier) and sums ALL partials in split order p0 + p1 + ... (its own from
// registers) -- one summation order per plan, whoever arrives last -- then runs the
// normal epilogue (bias, BN statistics, act, residual).  No workgroup waits for
// another, so residency does not matter.  This is the hand-off MI355X_MICROARCH.md
// measures valid with sc1 stores and loads in place of release / acquire fences.
// The partials and counters live in a CALLER-PROVIDED workspace (no library-owned
// state, so launches on different streams with different workspaces never meet):
// [kSkCntBytes of arrival counters, one int per output tile][partial tiles].  The
// counter block has a fixed size so that every plan run on one workspace finds its
// counters at the same words; the caller zeroes it once (every launch leaves it
// zero).  Size query: pose6d_conv_splitk_workspace.
constexpr int kSkMaxTiles = 8192;                       // plans with more tiles never split
constexpr int64_t kSkCntBytes = (int64_t)kSkMaxTiles * 4;   // 32 KiB

// Element geometry of the LDS-DMA path: a 16-byte chunk holds CH elements, a K-step
// (one 128-byte LDS row per GEMM row) KS = 8 CH: 64 bf16 or 32 fp32.  bf16 feeds
// v_mfma_f32_16x16x32_bf16 (one per 16x16 tile and k-half); fp32 feeds the exact
// v_mfma_f32_16x16x4_f32, four per tile and k-half -- a lane's 16-byte chunk holds
// k = 4 (fc + 4 kk) + s, s = 0..3, for A and B alike, so MFMA s sums the same k.
template <typename T> struct LK { static constexpr int CH = 16 / (int)sizeof(T), KS = 8 * CH; };

}  // namespace
