// Implicit-GEMM convolution (forward and data-gradient) on MFMA for gfx950.
//
// Replaces the cuDNN convolutions behind torchvision's ResNet50 trunk (used by
// every reference model, e.g. pose_net_rgbd_geometric.py:23-25) and the z-CNN of
// pose_net_rgb_geometric.py:36-55.
//
// GEMM view (NHWC activations, K ordered (kh, kw, c) with c fastest):
//   forward : Y[m = (n,oy,ox)][co] = sum_k A[m][k] * Wp[co][k],  A = im2col(X)
//   dgrad   : dX[m = (n,y,x)][ci]  = sum_k A[m][k] * Wt[ci][k],  A = col2im-gather(dY)
// One 256-thread workgroup = 4 waves (2 x 2) computes a BM x BN tile; K advances
// 64 bytes per step (BK = 32 bf16 / 16 fp32) through a double-buffered,
// XOR-swizzled LDS image (register staged so that padding taps load zeros).
// MFMA: v_mfma_f32_16x16x32_bf16 (bf16) or v_mfma_f32_16x16x4_f32 (fp32, exact
// fp32 products; used for the fp32 parity path).  Every lane reads its A and B
// fragments with one ds_read_b128 each; the swizzle makes those conflict-free.
// Epilogue: + bias, per-wave BatchNorm partial statistics (sum, sum of squares of
// the fp32 accumulators -> stats workspace, reduced by pose6d_bn_finalize), the
// tile goes through LDS so that global stores are whole 16-byte chunks of
// contiguous NHWC rows, optionally adding a residual tensor (dgrad: dX += dRes).
// This file: the launchers and the C entry points; conv_geom.h: what host and device
// share, conv_kernels.h: the kernels, conv_plan.h: the launch planning.
#include <type_traits>

#include "conv_kernels.h"
#include "conv_plan.h"

namespace {

// operands of one forward / data-gradient launch
struct ConvOps {
  const void *src, *w; const float* bias; const void* res; void* out; float* stats; hipStream_t s;
};
// the forward / data-gradient kernels' common signature
template <typename T> using ConvKernel = void (*)(const T*, const T*, const float*, const T*, T*, float*, Geom);

template <typename T, int BM, int BN, int MODE, int S, int NW = 4>
int launch_fast(const Geom& g0, const ConvOps& o) {
  Geom g = g0;
  g.gm = p6::ceil_div(g.M, BM);
  g.gn = p6::ceil_div(g.Ncols, BN);
  const int nk = fast_nk(MODE, g, LK<T>::KS);
  const int ring = (nk < S ? (nk > 0 ? nk : 1) : S) * (BM + BN) * 128;
  // kGemmDual stages both branches' tiles for its epilogue
  const int epi = (MODE == kGemmDual ? 2 : 1) * BM * (BN * (int)sizeof(T) + 16) + (g.bnr_part ? bnr_lds(NW, BN) : 0);
  const int lds = ring > epi ? ring : epi;
  if (MODE == kDgradS2) s2_single_class(g, o.res, o.out);
  constexpr bool SK = MODE == kGemm || MODE == kFwd || MODE == kDgrad;
  // the plan's split count (choose / splitk_need: <= nk, <= kSkMaxTiles tiles, the
  // workspace checked by run_plan)
  if (!SK || g.splits < 1 || !g.sk_cnt) g.splits = 1;
  const int grid = g.gm * g.gn * (MODE == kDgradS2 ? s2_classes(g) : 1) * (g.splits > 1 ? g.splits : 1);
  ConvKernel<T> kern = nullptr;
  if constexpr (MODE == kGemm || MODE == kFwd || MODE == kGemmDual)   // eval BN-act epilogue (pose6d_conv2d_fwd_act)
    if (g.act) kern = conv_lds_kernel<T, BM, BN, MODE, S, true, NW>;
  if constexpr (MODE == kGemm || MODE == kDgrad || MODE == kDgradS2)   // data gradient + BatchNorm reduce
    if (!kern && g.bnr_part) kern = conv_lds_kernel<T, BM, BN, MODE, S, false, NW, true>;
  if (!kern) kern = conv_lds_kernel<T, BM, BN, MODE, S, false, NW>;
  kern<<<grid, 64 * NW, lds, o.s>>>((const T*)o.src, (const T*)o.w, o.bias, (const T*)o.res, (T*)o.out, o.stats, g);
  P6_LAUNCH_CHECK();
  return POSE6D_OK;
}

// The LDS-DMA instances, as one ladder per plan field: mode -> tile -> ring depth.
// Ring depths 2, 3, 4 and -- where six stages fit the 160 KiB LDS -- 6 (else 4)
template <typename T, int MODE, int BM, int BN, int NW>
int launch_fast_ring(const Plan& p, const ConvOps& o) {
  if constexpr (MODE == kFwdRowTap) {   // (few instances: 2 / 3 / 4 slots)
    if (p.stages >= 4) return launch_fast<T, BM, BN, MODE, 4, NW>(p.g, o);
    if (p.stages == 3) return launch_fast<T, BM, BN, MODE, 3, NW>(p.g, o);
    return launch_fast<T, BM, BN, MODE, 2, NW>(p.g, o);
  } else switch (p.stages) {
    case 2: return launch_fast<T, BM, BN, MODE, 2, NW>(p.g, o);
    case 3: return launch_fast<T, BM, BN, MODE, 3, NW>(p.g, o);
    case 4: return launch_fast<T, BM, BN, MODE, 4, NW>(p.g, o);
    default:
      if constexpr ((BM + BN) * 128 * 6 <= 160 * 1024) return launch_fast<T, BM, BN, MODE, 6, NW>(p.g, o);
      else return launch_fast<T, BM, BN, MODE, 4, NW>(p.g, o);
  }
}

// tile codes: tile_dims (conv_plan.h).  The row-tap stems have the 4-wave 128x64 and 64x64
// tiles only, kGemmDual 64x64
template <typename T, int MODE>
int launch_fast_tile(const Plan& p, const ConvOps& o) {
  if constexpr (MODE == kGemmDual) return launch_fast_ring<T, MODE, 64, 64, 4>(p, o);
  else if constexpr (MODE == kFwdRowTap)
    return (p.tile == 1 || p.tile == 5) ? launch_fast_ring<T, MODE, 128, 64, 4>(p, o)
                                        : launch_fast_ring<T, MODE, 64, 64, 4>(p, o);
  else switch (p.tile) {
    case 0: return launch_fast_ring<T, MODE, 128, 128, 4>(p, o);
    case 1: return launch_fast_ring<T, MODE, 128, 64, 4>(p, o);
    case 4: return launch_fast_ring<T, MODE, 128, 128, 8>(p, o);
    case 5: return launch_fast_ring<T, MODE, 128, 64, 8>(p, o);
    default: return launch_fast_ring<T, MODE, 64, 64, 4>(p, o);
  }
}

template <typename T>
int dispatch_fast_t(const Plan& p, const ConvOps& o) {
  switch (p.mode) {
    case kGemm: return launch_fast_tile<T, kGemm>(p, o);
    case kFwd: return launch_fast_tile<T, kFwd>(p, o);
    case kFwdRowTap: return launch_fast_tile<T, kFwdRowTap>(p, o);
    case kDgradS2: return launch_fast_tile<T, kDgradS2>(p, o);
    case kGemmDual: return launch_fast_tile<T, kGemmDual>(p, o);
    default: return launch_fast_tile<T, kDgrad>(p, o);
  }
}

int dispatch_fast(int dtype, const Plan& p, const ConvOps& o) {
  return dtype == POSE6D_DT_BF16 ? dispatch_fast_t<bf16>(p, o) : dispatch_fast_t<float>(p, o);
}

template <typename T, int BM, int BN, int MODE>
int launch_t(const Geom& g0, const ConvOps& o) {
  Geom g = g0;
  g.gm = p6::ceil_div(g.M, BM);
  g.gn = p6::ceil_div(g.Ncols, BN);
  const int stage = 2 * (BM + BN) * 64;
  const int epi = BM * (BN * (int)sizeof(T) + 16);
  const int lds = stage > epi ? stage : epi;
  ConvKernel<T> kern = nullptr;
  if constexpr (MODE != kDgrad)   // eval BN-act epilogue (pose6d_conv2d_fwd_act)
    if (g.act) kern = conv_igemm_kernel<T, BM, BN, MODE, true>;
  if (!kern) kern = conv_igemm_kernel<T, BM, BN, MODE, false>;
  kern<<<g.gm * g.gn, kThreads, lds, o.s>>>((const T*)o.src, (const T*)o.w, o.bias, (const T*)o.res, (T*)o.out,
                                            o.stats, g);
  P6_LAUNCH_CHECK();
  return POSE6D_OK;
}

template <typename T, int MODE>
int launch_mode(const Plan& p, const ConvOps& o) {
  switch (p.tile) {
    case 0: return launch_t<T, 128, 128, MODE>(p.g, o);
    case 1: return launch_t<T, 128, 64, MODE>(p.g, o);
    case 2: return launch_t<T, 64, 128, MODE>(p.g, o);
    default: return launch_t<T, 64, 64, MODE>(p.g, o);
  }
}

// the register-staged kernels
template <typename T>
int dispatch(const Plan& p, const ConvOps& o) {
  switch (p.mode) {
    case kGemm: return launch_mode<T, kGemm>(p, o);
    case kFwd: return launch_mode<T, kFwd>(p, o);
    case kFwdNarrow: return launch_mode<T, kFwdNarrow>(p, o);
    default: return launch_mode<T, kDgrad>(p, o);
  }
}

// a planned implicit-GEMM launch: the split-K workspace of the plan, then its kernel (below)
int run_plan(int dtype, Plan p, const ConvOps& o, void* sk_ws, int64_t sk_bytes);

int run_conv(int dtype, int mode, const Geom& g, const ConvOps& o, const pose6d_tuning_t* tn, bool fwd, void* sk_ws,
             int64_t sk_bytes) {
  // 3x3 stride-1 bf16 forwards without BatchNorm statistics (eval; conv_patch.h: the
  // input patch staged once per 64-channel slice instead of once per filter tap) are
  // decided first -- the patch kernel never splits K, so it needs no split-K workspace
  // even where the implicit-GEMM plan of the same geometry would
  PatchPlan pp{};
  if (patch_eligible(dtype, mode, g, o.stats, tn, &pp)) {
    const int st = tn && tn->conv_patch == 1 && tn->conv_stages > 0 ? tn->conv_stages : kPatchStages;
    if (st != kPatchStages) pp = patch_plan(g.M / (g.RH * g.RW), g.RH, g.RW, g.SC, g.Ncols, st);
    P6_CHECK_ARG(pp.ok, "conv: patch plan with %d ring slots exceeds the LDS", st);
    const int N = g.M / (g.RH * g.RW);
    switch (st) {
      case 3: return launch_patch<3>(g, pp, N, o.src, o.w, o.bias, o.res, o.out, o.s);
      case 4: return launch_patch<4>(g, pp, N, o.src, o.w, o.bias, o.res, o.out, o.s);
      case 6: return launch_patch<6>(g, pp, N, o.src, o.w, o.bias, o.res, o.out, o.s);
      case 8: return launch_patch<8>(g, pp, N, o.src, o.w, o.bias, o.res, o.out, o.s);
      default: return launch_patch<kPatchStages>(g, pp, N, o.src, o.w, o.bias, o.res, o.out, o.s);
    }
  }
  return run_plan(dtype, choose(dtype, mode, g, false, tn, fwd), o, sk_ws, sk_bytes);
}

int run_plan(int dtype, Plan p, const ConvOps& o, void* sk_ws, int64_t sk_bytes) {
  const int64_t need = splitk_need(p);
  if (need > 0) {
    P6_CHECK_ARG(sk_ws != nullptr && sk_bytes >= need,
                 "conv: this plan splits K over %d workgroups per tile (pose6d_conv_variant >> 16) and needs a split-K "
                 "workspace of %lld bytes (pose6d_conv_splitk_workspace), got %lld",
                 p.g.splits, (long long)need, (long long)(sk_ws ? sk_bytes : 0));
    P6_CHECK_ARG(((uintptr_t)sk_ws & 255) == 0, "conv: the split-K workspace must be 256-byte aligned");
    p.g.sk_cnt = (int*)sk_ws;
    p.g.sk_part = (float*)((char*)sk_ws + kSkCntBytes);
  }
  if (p.fast) return dispatch_fast(dtype, p, o);
  return dtype == POSE6D_DT_BF16 ? dispatch<bf16>(p, o) : dispatch<float>(p, o);
}

// the checks pose6d_conv2d_fwd[_tuned] and pose6d_conv2d_fwd_act share (`fn` names the
// entry point in the messages), and the forward geometry
int fwd_checked_geom(const char* fn, int dtype, const ConvShape& c, Geom* g, int* mode) {
  P6_CHECK_ARG(dtype == POSE6D_DT_F32 || dtype == POSE6D_DT_BF16, "%s: bad dtype %d", fn, dtype);
  P6_CHECK_ARG(c.N > 0 && c.H > 0 && c.W > 0 && c.Cout > 0 && c.Cout % 8 == 0, "%s: bad shape (Cout %% 8)", fn);
  P6_CHECK_ARG(c.Ho == (c.H + 2 * c.pad - c.KH) / c.stride + 1 && c.Wo == (c.W + 2 * c.pad - c.KW) / c.stride + 1,
               "%s: Ho/Wo inconsistent", fn);
  const int bk = dtype == POSE6D_DT_BF16 ? 32 : 16;
  *g = fwd_geom(dtype, c, mode);
  if (*mode == kFwd)
    P6_CHECK_ARG(g->log2SC >= 0 && c.Cin % bk == 0, "%s: Cin must be 4 or a power of two >= %d (got %d)", fn, bk,
                 c.Cin);
  if (*mode == kGemm) P6_CHECK_ARG(c.Cin % bk == 0, "%s: 1x1 Cin %% %d != 0", fn, bk);
  return POSE6D_OK;
}

// the eval BN-act epilogue (pose6d_conv2d_fwd_act): act(y * scale + shift [+ res | + res * rscale + rshift])
void set_act(Geom& g, int relu, const float* scale, const float* shift, const float* rscale, const float* rshift) {
  g.act = 1; g.act_relu = relu != 0;
  g.act_scale = scale; g.act_shift = shift; g.act_rscale = rscale; g.act_rshift = rshift;
}

}  // namespace

// statistics rows: one per 32 output pixels (the last may cover fewer)
extern "C" int pose6d_conv_stats_rows(int32_t N, int32_t Ho, int32_t Wo, int32_t Cout) {
  (void)Cout;
  return p6::ceil_div((int64_t)N * Ho * Wo, 32);
}

extern "C" int pose6d_conv2d_fwd(int32_t dtype, const void* x, const void* w, const float* bias, void* y,
                                 float* stats, int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH,
                                 int32_t KW, int32_t stride, int32_t pad, int32_t Ho, int32_t Wo, void* splitk_ws,
                                 int64_t splitk_ws_bytes, void* stream) {
  return pose6d_conv2d_fwd_tuned(dtype, x, w, bias, y, stats, N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo,
                                 nullptr, splitk_ws, splitk_ws_bytes, stream);
}

extern "C" int pose6d_conv2d_fwd_tuned(int32_t dtype, const void* x, const void* w, const float* bias, void* y,
                                       float* stats, int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                                       int32_t KH, int32_t KW, int32_t stride, int32_t pad, int32_t Ho, int32_t Wo,
                                       const pose6d_tuning_t* tuning, void* splitk_ws, int64_t splitk_ws_bytes,
                                       void* stream) {
  const ConvShape cs{N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo};
  Geom g;
  int mode;
  const int rc = fwd_checked_geom("pose6d_conv2d_fwd", dtype, cs, &g, &mode);
  if (rc) return rc;
  if (mode == kFwdRowTap)
    P6_CHECK_ARG(dtype == POSE6D_DT_F32 || W % 2 == 0, "pose6d_conv2d_fwd: the bf16 row-tap stem needs an even W");
  return run_conv(dtype, mode, g, {x, w, bias, nullptr, y, stats, p6::stream_of(stream)}, tuning, true, splitk_ws,
                  splitk_ws_bytes);
}

extern "C" int pose6d_conv_pack_geom(int32_t dtype, int32_t Cin, int32_t KH, int32_t KW, int32_t stride, int32_t pad,
                                     int32_t* kw_packed, int32_t* Kpad) {
  P6_CHECK_ARG(kw_packed && Kpad && Cin > 0 && KH > 0 && KW > 0, "pose6d_conv_pack_geom: bad arguments");
  *Kpad = pack_geom(dtype, Cin, KH, KW, stride, pad, kw_packed);
  return POSE6D_OK;
}

// eval-mode conv + BatchNorm apply (+ residual, + ReLU) in one launch: the store of
// pose6d_conv2d_fwd followed by pose6d_bn_act_fwd, bit for bit, without the raw output
extern "C" int pose6d_conv2d_fwd_act(int32_t dtype, const void* x, const void* w, const float* bias, void* out,
                                     int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW,
                                     int32_t stride, int32_t pad, int32_t Ho, int32_t Wo, const float* scale,
                                     const float* shift, const void* res, const float* res_scale,
                                     const float* res_shift, int32_t relu, void* splitk_ws, int64_t splitk_ws_bytes,
                                     void* stream) {
  const ConvShape cs{N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo};
  Geom g;
  int mode;
  const int rc = fwd_checked_geom("pose6d_conv2d_fwd_act", dtype, cs, &g, &mode);
  if (rc) return rc;
  P6_CHECK_ARG(scale && shift, "pose6d_conv2d_fwd_act: null scale / shift");
  P6_CHECK_ARG(!res_scale == !res_shift && (!res_scale || res), "pose6d_conv2d_fwd_act: bad residual BN args");
  P6_CHECK_ARG(mode != kFwdRowTap && mode != kFwdNarrow,
               "pose6d_conv2d_fwd_act: 4-channel convs have no BN-act epilogue (pose6d_conv2d_fwd, then the BN)");
  set_act(g, relu, scale, shift, res_scale, res_shift);
  return run_conv(dtype, mode, g, {x, w, bias, res, out, nullptr, p6::stream_of(stream)}, nullptr, true, splitk_ws,
                  splitk_ws_bytes);
}

extern "C" int pose6d_conv2d_fwd_act_dual(int32_t dtype, const void* x, const void* w, const void* xd, const void* wd,
                                          void* out, int32_t N, int32_t Ho, int32_t Wo, int32_t Cin, int32_t Cout,
                                          int32_t Hd, int32_t Wd, int32_t Cind, int32_t stride_d, const float* scale,
                                          const float* shift, const float* scale_d, const float* shift_d,
                                          int32_t relu, void* stream) {
  // the block's last 1x1 conv and its 1x1 / stride_d downsample branch
  const ConvShape c3{N, Ho, Wo, Cin, Cout, 1, 1, 1, 0, Ho, Wo}, cd{N, Hd, Wd, Cind, Cout, 1, 1, stride_d, 0, Ho, Wo};
  P6_CHECK_ARG(dtype == POSE6D_DT_F32 || dtype == POSE6D_DT_BF16, "pose6d_conv2d_fwd_act_dual: bad dtype %d", dtype);
  P6_CHECK_ARG(N > 0 && Ho > 0 && Wo > 0 && Cout > 0 && Cout % 8 == 0, "pose6d_conv2d_fwd_act_dual: bad shape");
  P6_CHECK_ARG(stride_d >= 1 && Ho == (Hd - 1) / stride_d + 1 && Wo == (Wd - 1) / stride_d + 1,
               "pose6d_conv2d_fwd_act_dual: downsample geometry inconsistent");
  P6_CHECK_ARG(scale && shift && scale_d && shift_d, "pose6d_conv2d_fwd_act_dual: null BatchNorm scale / shift");
  const int ks = dtype == POSE6D_DT_BF16 ? 64 : 32;
  P6_CHECK_ARG(Cin % ks == 0 && Cind % ks == 0, "pose6d_conv2d_fwd_act_dual: Cin and Cind must be multiples of %d",
               ks);
  int m3, md;
  const Geom g3 = fwd_geom(dtype, c3, &m3), gd = fwd_geom(dtype, cd, &md);
  Geom g = g3;
  g.src2 = xd; g.wts2 = wd; g.Kpad2 = Cind;
  g.SH2 = Hd; g.SW2 = Wd; g.stride2 = stride_d;
  set_act(g, relu, scale, shift, scale_d, shift_d);
  const Plan p = choose(dtype, kGemmDual, g);
  P6_CHECK_ARG(p.fast, "pose6d_conv2d_fwd_act_dual: shape outside the LDS-DMA path");
  // bit identity with the separate launches needs their K loops unsplit (the dual
  // kernel has no split-K); pose6d_conv_variant reports the separate plans' splits
  P6_CHECK_ARG(choose(dtype, m3, g3, false, nullptr, true).g.splits == 1 &&
                   choose(dtype, md, gd, false, nullptr, true).g.splits == 1,
               "pose6d_conv2d_fwd_act_dual: the separate launches of this pair split K (pose6d_conv_variant >> 16); "
               "run them separately");
  return run_plan(dtype, p, {x, w, nullptr, nullptr, out, nullptr, p6::stream_of(stream)}, nullptr, 0);
}

namespace {
void set_bnr(Geom& g, const pose6d_bn_reduce_t* b) {
  if (!b) return;
  g.bnr_y = b->y; g.bnr_mean = b->mean; g.bnr_inv = b->invstd;
  g.bnr_rs = b->relu_scale; g.bnr_rb = b->relu_shift; g.bnr_mask = b->relu_mask;
  g.bnr_part = b->partial; g.bnr_rows = b->rows;
  g.bnr_y2 = b->y2; g.bnr_mean2 = b->mean2; g.bnr_inv2 = b->invstd2; g.bnr_part2 = b->partial2;
}

// planned: the plan of this data gradient where the caller has it (plan_backward's `run`)
int dgrad_impl(int dtype, const ConvShape& c, const void* dy, const void* wt, const void* dres,
               const uint8_t* dres_mask, void* dx, void* stream, const pose6d_tuning_t* tn = nullptr,
               const pose6d_bn_reduce_t* bnr = nullptr, void* sk_ws = nullptr, int64_t sk_bytes = 0,
               const Plan* planned = nullptr) {
  P6_CHECK_ARG(dtype == POSE6D_DT_F32 || dtype == POSE6D_DT_BF16, "pose6d_conv2d_dgrad: bad dtype %d", dtype);
  P6_CHECK_ARG(c.stride == 1 || c.stride == 2, "pose6d_conv2d_dgrad: stride must be 1 or 2");
  P6_CHECK_ARG(c.Cin % 8 == 0, "pose6d_conv2d_dgrad: Cin %% 8 != 0 (no data gradient for the stem)");
  P6_CHECK_ARG(!dres_mask || (dres && dres != dx), "pose6d_conv2d_dgrad: a residual mask needs a separate dres");
  const int bk = dtype == POSE6D_DT_BF16 ? 32 : 16;
  int mode;
  const Geom g = dgrad_geom(c, &mode);
  P6_CHECK_ARG(g.log2SC >= 0 && c.Cout % bk == 0, "pose6d_conv2d_dgrad: Cout must be a power of two >= %d", bk);
  Plan p = planned ? *planned : choose(dtype, mode, g, false, tn);
  p.g.res_mask = dres_mask;
  const int rc = check_bnr(bnr, p, dres, dx);
  if (rc) return rc;
  set_bnr(p.g, bnr);
  return run_plan(dtype, p, {dy, wt, nullptr, dres, dx, nullptr, p6::stream_of(stream)}, sk_ws, sk_bytes);
}
}  // namespace

extern "C" int pose6d_conv2d_dgrad(int32_t dtype, const void* dy, const void* wt, const void* dres, void* dx,
                                   int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW,
                                   int32_t stride, int32_t pad, int32_t Ho, int32_t Wo, void* stream) {
  return pose6d_conv2d_dgrad_tuned(dtype, dy, wt, dres, dx, N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo, nullptr,
                                   nullptr, 0, stream);
}

extern "C" int pose6d_conv2d_dgrad_tuned(int32_t dtype, const void* dy, const void* wt, const void* dres, void* dx,
                                         int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH,
                                         int32_t KW, int32_t stride, int32_t pad, int32_t Ho, int32_t Wo,
                                         const pose6d_tuning_t* tuning, void* splitk_ws, int64_t splitk_ws_bytes,
                                         void* stream) {
  const ConvShape cs{N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo};
  return dgrad_impl(dtype, cs, dy, wt, dres, nullptr, dx, stream, tuning, nullptr, splitk_ws, splitk_ws_bytes);
}

namespace {

// dispatch-order rule of the fused launch: an fp32 64-pixel weight-gradient stage is
// twice the MACs of a 32-channel data-gradient K-step, so it counts double (28x28
// 128->512 fp32: 79.5 -> 72.5 us with the weight gradient first, profiles/r04_bwd_plan_sweep.txt)
constexpr int kBwdWstepF32 = 2;

// operands of one fused backward launch: `slab` = the weight-gradient slabs (or dW itself),
// `rj` = the previous conv's slab reduce carried as trailing workgroups, `order` = a
// tuned dispatch order (-1: the rule)
struct BwdOps {
  const void *dy, *wt, *dres; void* dx; const void* x; float* slab; const ReduceJob& rj; hipStream_t s; int order;
};

template <int DMODE, int DS, int WS, typename T = bf16, int WBT = 64>
int launch_bwd(const Geom& gd0, const p6::WGeom& gw, const BwdOps& o) {
  Geom gd = gd0;
  gd.gm = p6::ceil_div(gd.M, 64);
  gd.gn = p6::ceil_div(gd.Ncols, 64);
  if (DMODE == kDgradS2) s2_single_class(gd, o.dres, o.dx);
  const int nd = gd.gm * gd.gn * (DMODE == kDgradS2 ? s2_classes(gd) : 1);
  const int nd_pad = (nd + 7) & ~7;
  const int nw = gw.gm * gw.gn * gw.splits;
  const int nk = fast_nk(DMODE, gd, LK<T>::KS);
  const int ring_d = (nk < DS ? (nk > 0 ? nk : 1) : DS) * 128 * 128;
  const int epi = 64 * (64 * (int)sizeof(T) + 16) + (gd.bnr_part ? bnr_lds(4, 64) : 0);
  const int ring_w = sizeof(T) == 2 ? WS * 128 * 128
                                    : (WBT == 128 ? WS * WgF32<32, 128>::STAGE : WS * WgF32<kBwdF32MS>::STAGE);
  int lds = ring_d > epi ? ring_d : epi;
  lds = lds > ring_w ? lds : ring_w;
  if (sizeof(T) == 4 && WBT == 128 && lds < acc_stage_bytes<128, 128>()) lds = acc_stage_bytes<128, 128>();
  // longest workgroups first: the weight gradient goes first when its stages per split
  // are at least the data gradient's K-steps per tile (fp32 stages weighted kBwdWstepF32)
  constexpr int WSTEP = sizeof(T) == 4 ? kBwdWstepF32 : 1;
  const int wfirst = o.order >= 0 ? o.order : (WSTEP * p6::ceil_div(gw.mps, 64) >= nk);
  const int grid = wfirst ? ((nw + 7) & ~7) + nd + o.rj.nblk : nd_pad + nw + o.rj.nblk;
  conv_bwd_kernel<DMODE, DS, WS, T, WBT><<<grid, kThreads, lds, o.s>>>(
      (const T*)o.dy, (const T*)o.wt, (const T*)o.dres, (T*)o.dx, gd, nd, nd_pad, wfirst, (const T*)o.x, o.slab, gw,
      o.rj);
  P6_LAUNCH_CHECK();
  return POSE6D_OK;
}

// the 8-wave fused launch (conv_bwd8_kernel): 128x64 data-gradient tiles, the 128x128
// weight-gradient body on a WS-slot ring; LDS = the larger of the two roles' rings and
// epilogue staging (the 128x128 fp32 tile staged for 16-byte slab stores: 72 KiB)
template <int DMODE, int DS, int WS>
int launch_bwd8(const Geom& gd0, const p6::WGeom& gw, const BwdOps& o) {
  Geom gd = gd0;
  gd.gm = p6::ceil_div(gd.M, 128);
  gd.gn = p6::ceil_div(gd.Ncols, 64);
  if (DMODE == kDgradS2) s2_single_class(gd, o.dres, o.dx);
  const int nd = gd.gm * gd.gn * (DMODE == kDgradS2 ? s2_classes(gd) : 1);
  const int nd_pad = (nd + 7) & ~7;
  const int nw = gw.gm * gw.gn * gw.splits;
  const int nk = fast_nk(DMODE, gd, 64);
  const int ring_d = (nk < DS ? (nk > 0 ? nk : 1) : DS) * (128 + 64) * 128;
  const int epi = 128 * (64 * 2 + 16) + (gd.bnr_part ? bnr_lds(8, 64) : 0);
  const int ring_w = WS * (128 + 128) * 128;
  int lds = ring_d > epi ? ring_d : epi;
  lds = lds > ring_w ? lds : ring_w;
  lds = lds > acc_stage_bytes<128, 128>() ? lds : acc_stage_bytes<128, 128>();
  const int wfirst = o.order >= 0 ? o.order : (p6::ceil_div(gw.mps, 64) >= nk);   // the rule of launch_bwd
  const int grid = wfirst ? ((nw + 7) & ~7) + nd + o.rj.nblk : nd_pad + nw + o.rj.nblk;
  conv_bwd8_kernel<DMODE, DS, WS><<<grid, 2 * kThreads, lds, o.s>>>(
      (const bf16*)o.dy, (const bf16*)o.wt, (const bf16*)o.dres, (bf16*)o.dx, gd, nd, nd_pad, wfirst,
      (const bf16*)o.x, o.slab, gw, o.rj);
  P6_LAUNCH_CHECK();
  return POSE6D_OK;
}

template <int DMODE>
int launch_bwd8_mode(int ds, int ws_stages, const Geom& gd, const p6::WGeom& gw, const BwdOps& o) {
  if (ws_stages >= 3) return ds == 2 ? launch_bwd8<DMODE, 2, 3>(gd, gw, o) : launch_bwd8<DMODE, 4, 3>(gd, gw, o);
  return ds == 2 ? launch_bwd8<DMODE, 2, 2>(gd, gw, o) : launch_bwd8<DMODE, 4, 2>(gd, gw, o);
}

// ds: the data-gradient plan's ring (fused_ds maps it to the launch's); wbt: the weight-gradient tile
template <int DMODE>
int launch_bwd_mode(int dtype, int ds, int wbt, const Geom& gd, const p6::WGeom& gw, const BwdOps& o) {
  if (dtype == POSE6D_DT_F32 && wbt == 128)
    return fused_ds(dtype, ds) == 2 ? launch_bwd<DMODE, 2, p6::kWgradStagesF32, float, 128>(gd, gw, o)
                                    : launch_bwd<DMODE, 3, p6::kWgradStagesF32, float, 128>(gd, gw, o);
  if (dtype == POSE6D_DT_F32)
    return fused_ds(dtype, ds) == 2 ? launch_bwd<DMODE, 2, p6::kWgradStagesF32, float>(gd, gw, o)
                                    : launch_bwd<DMODE, 3, p6::kWgradStagesF32, float>(gd, gw, o);
  return ds == 2 ? launch_bwd<DMODE, 2, p6::kWgradStages>(gd, gw, o)
                 : launch_bwd<DMODE, kBwdBf16DS4, p6::kWgradStages>(gd, gw, o);
}

// the data-gradient modes of the fused launches as compile-time constants:
// f(std::integral_constant<int, mode>)
template <typename F>
int with_dgrad_mode(int mode, F&& f) {
  switch (mode) {
    case kGemm: return f(std::integral_constant<int, kGemm>{});
    case kDgradS2: return f(std::integral_constant<int, kDgradS2>{});
    default: return f(std::integral_constant<int, kDgrad>{});
  }
}

// tensors of one conv's backward (dx == NULL: weight gradient only; dres_mask as in
// pose6d_conv2d_backward_chain_masked, or NULL)
struct BwdArgs {
  const void *x, *dy, *wt, *dres; const uint8_t* dres_mask; void* dx; float* dw; int accumulate;
  float* workspace; int64_t ws_bytes; int Cin_real;
};

// Data + weight gradient of one conv.  When both passes take the bf16 LDS-DMA
// kernels (64x64 tiles, data-gradient ring of 2 or 4 slots, weight-gradient ring
// of 3) they run as ONE launch of conv_bwd_kernel, followed by the slab reduce;
// otherwise as the separate pose6d_conv2d_dgrad + pose6d_conv2d_wgrad launches.
// rj: the previous conv's slab reduce to carry (nblk 0: none); deferred: chain mode.
int conv_backward_impl(int dtype, const ConvShape& c, const BwdArgs& a, int phases, void* stream,
                       const ReduceJob& rj = ReduceJob{}, int32_t* deferred = nullptr,
                       const pose6d_tuning_t* tn = nullptr, const pose6d_bn_reduce_t* bnr = nullptr) {
  P6_CHECK_ARG(dtype == POSE6D_DT_F32 || dtype == POSE6D_DT_BF16, "pose6d_conv2d_backward: bad dtype %d", dtype);
  if (deferred) *deferred = 0;
  hipStream_t s = p6::stream_of(stream);
  auto flush_prev = [&]() -> int {   // the carried reduce as a launch of its own
    if (rj.nblk == 0) return POSE6D_OK;
    return p6::wgrad_reduce_launch(rj.ws, rj.dw, rj.Cout, rj.Kpad, rj.SC, rj.Cin, rj.KH, rj.KW, rj.KWp, rj.splits,
                                   rj.accumulate, s);
  };
  auto wgrad_alone = [&]() -> int {
    return pose6d_conv2d_wgrad_tuned(dtype, a.x, a.dy, a.dw, a.accumulate, a.workspace, a.ws_bytes, c.N, c.H, c.W,
                                     c.Cin, a.Cin_real, c.Cout, c.KH, c.KW, c.stride, c.pad, c.Ho, c.Wo, tn, stream);
  };
  P6_CHECK_ARG(phases >= 1 && phases <= 3, "pose6d_conv2d_backward_ex: phases must be 1, 2 or 3");
  P6_CHECK_ARG(!bnr || (a.dx && phases == 3), "pose6d_conv2d_backward: a BatchNorm reduce needs the data gradient");
  const BwdPlan bp = plan_backward(dtype, c, tn);
  const p6::WgradPlan& pw = bp.pw;
  const p6::WGeom& gw = bp.gw;
  const int64_t slab_bytes = (int64_t)pw.splits * c.Cout * gw.Kpad * 4;
  // chain mode with a register-staged weight gradient (fp32, the bf16 stem): that launch
  // carries the previous conv's slab reduce as trailing workgroups and leaves its own
  // reduce pending, as the fused bf16 launch does -- one launch per conv fewer
  auto carry_wgrad = [&]() -> int {   // (*deferred = 1: carried)
    if (!deferred || phases != 3) return POSE6D_OK;
    // bf16 LDS-DMA plans go through the fused launch -- except a weight gradient alone
    // (no data gradient: the row-tap stems), whose LDS-DMA kernel carries the reduce too
    if (pw.fast && dtype == POSE6D_DT_BF16 && a.dx != nullptr) return POSE6D_OK;
    P6_CHECK_ARG(slab_bytes <= a.ws_bytes, "pose6d_conv2d_backward: workspace %lld bytes < %lld needed",
                 (long long)a.ws_bytes, (long long)slab_bytes);
    const int rc = p6::wgrad_launch_carry(dtype, gw, pw, a.x, a.dy, a.workspace, rj, s);
    *deferred = rc == POSE6D_OK;
    return rc;
  };
  if (a.dx == nullptr) {
    if (!(phases & 1)) return POSE6D_OK;
    int rc = carry_wgrad();
    if (rc || (deferred && *deferred)) return rc;
    rc = flush_prev();
    return rc ? rc : wgrad_alone();
  }
  P6_CHECK_ARG(c.stride == 1 || c.stride == 2, "pose6d_conv2d_backward: stride must be 1 or 2");
  P6_CHECK_ARG(bp.dgrad && a.Cin_real <= c.Cin,
               "pose6d_conv2d_backward: Cin must be a power of two >= 8 for the data gradient");
  P6_CHECK_ARG(!a.dres_mask || (a.dres && a.dres != a.dx),
               "pose6d_conv2d_backward: a residual mask needs a separate dres");
  if (!bp.fused) {
    if (!(phases & 1)) return POSE6D_OK;
    const bool carry = deferred && phases == 3 && (!pw.fast || dtype == POSE6D_DT_F32);
    int rc = carry ? POSE6D_OK : flush_prev();
    if (rc) return rc;
    rc = dgrad_impl(dtype, c, a.dy, a.wt, a.dres, a.dres_mask, a.dx, stream, tn, bnr, nullptr, 0, &bp.run);
    if (rc) return rc;
    if (carry) {
      rc = carry_wgrad();
      if (rc || *deferred) return rc;
      rc = flush_prev();
      if (rc) return rc;
    }
    return wgrad_alone();
  }
  P6_CHECK_ARG(slab_bytes <= a.ws_bytes, "pose6d_conv2d_backward: workspace %lld bytes < %lld needed",
               (long long)a.ws_bytes, (long long)slab_bytes);
  int rc = check_bnr(bnr, bp.run, a.dres, a.dx);
  if (rc) return rc;
  Geom gd = bp.pd.g;
  gd.res_mask = a.dres_mask;
  set_bnr(gd, bnr);
  // one weight-gradient split of a 1x1 conv whose K is exactly Cin (layer4's 1x1 convs):
  // the slab [Cout][Cin] IS the OIHW dW, so the launch writes dW itself and no reduce
  // follows (the reduce would only have copied it; profiles/r04_wgrad_direct_ab.txt)
  const bool direct = bp.direct && a.Cin_real == c.Cin && !a.accumulate;
  if (phases & 1) {
    const BwdOps o{a.dy, a.wt, a.dres, a.dx, a.x, direct ? a.dw : a.workspace, rj, s,
                   tuned(tn, &pose6d_tuning_t::bwd_order, -1)};
    const bool wide8 = pw.bm == 128 && dtype == POSE6D_DT_BF16;   // conv_bwd8_kernel
    rc = wide8 ? with_dgrad_mode(bp.pd.mode, [&](auto m) {
      return launch_bwd8_mode<decltype(m)::value>(bp.pd.stages, pw.stages, gd, gw, o);
    }) : with_dgrad_mode(bp.pd.mode, [&](auto m) {
      return launch_bwd_mode<decltype(m)::value>(dtype, bp.pd.stages, pw.bm, gd, gw, o);
    });
  }
  if (direct) return rc;   // (*deferred stays 0)
  if (deferred) {   // chain mode: this conv's slab reduce rides on the next launch
    *deferred = rc == POSE6D_OK;
    return rc;
  }
  if (rc || !(phases & 2)) return rc;
  return p6::wgrad_reduce_launch(a.workspace, a.dw, c.Cout, gw.Kpad, c.Cin, a.Cin_real, c.KH, c.KW, gw.kwp, gw.splits,
                                 a.accumulate, s);
}

ReduceJob make_job(const pose6d_wgrad_reduce_t& j) {
  const p6::WGeom g = p6::wgrad_geom(j.dtype, {j.N, j.H, j.W, j.Cin, j.Cout, j.KH, j.KW, j.stride, j.pad, j.Ho, j.Wo},
                                     nullptr);
  ReduceJob r{};
  r.ws = j.ws; r.dw = j.dw; r.Cout = j.Cout; r.Kpad = g.Kpad; r.SC = j.Cin; r.Cin = j.Cin_real;
  r.KH = j.KH; r.KW = j.KW; r.KWp = g.kwp; r.splits = g.splits; r.accumulate = j.accumulate;
  r.G = reduce_group(g.splits); r.nblk = reduce_blocks(j.Cout, g.Kpad, r.G);
  return r;
}

// the chain entry points' shared prologue (`fn` names the entry point): *job = the
// previous conv's slab reduce for this launch to carry (prev == NULL: none)
int chain_job(const char* fn, const pose6d_wgrad_reduce_t* prev, const float* workspace, const int32_t* deferred,
              ReduceJob* job) {
  P6_CHECK_ARG(deferred != nullptr, "%s: deferred must point to an int32", fn);
  *job = ReduceJob{};
  if (!prev) return POSE6D_OK;
  P6_CHECK_ARG(prev->ws != workspace, "pose6d_conv2d_backward_chain: prev slabs must live in another workspace");
  *job = make_job(*prev);
  return POSE6D_OK;
}
}  // namespace

extern "C" int pose6d_conv2d_backward(int32_t dtype, const void* x, const void* dy, const void* wt, const void* dres,
                                      void* dx, float* dw, int32_t accumulate, float* workspace, int64_t ws_bytes,
                                      int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cin_real, int32_t Cout,
                                      int32_t KH, int32_t KW, int32_t stride, int32_t pad, int32_t Ho, int32_t Wo,
                                      void* stream) {
  return pose6d_conv2d_backward_ex(dtype, x, dy, wt, dres, dx, dw, accumulate, workspace, ws_bytes, N, H, W, Cin,
                                   Cin_real, Cout, KH, KW, stride, pad, Ho, Wo, 3, stream);
}

extern "C" int pose6d_conv2d_backward_tuned(int32_t dtype, const void* x, const void* dy, const void* wt,
                                            const void* dres, void* dx, float* dw, int32_t accumulate,
                                            float* workspace, int64_t ws_bytes, int32_t N, int32_t H, int32_t W,
                                            int32_t Cin, int32_t Cin_real, int32_t Cout, int32_t KH, int32_t KW,
                                            int32_t stride, int32_t pad, int32_t Ho, int32_t Wo,
                                            const pose6d_tuning_t* tuning, void* stream) {
  const ConvShape cs{N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo};
  return conv_backward_impl(dtype, cs, {x, dy, wt, dres, nullptr, dx, dw, accumulate, workspace, ws_bytes, Cin_real}, 3,
                            stream, ReduceJob{}, nullptr, tuning);
}

extern "C" int pose6d_conv2d_backward_ex(int32_t dtype, const void* x, const void* dy, const void* wt,
                                         const void* dres, void* dx, float* dw, int32_t accumulate, float* workspace,
                                         int64_t ws_bytes, int32_t N, int32_t H, int32_t W, int32_t Cin,
                                         int32_t Cin_real, int32_t Cout, int32_t KH, int32_t KW, int32_t stride,
                                         int32_t pad, int32_t Ho, int32_t Wo, int32_t phases, void* stream) {
  const ConvShape cs{N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo};
  return conv_backward_impl(dtype, cs, {x, dy, wt, dres, nullptr, dx, dw, accumulate, workspace, ws_bytes, Cin_real},
                            phases, stream);
}

// launch variant of a forward / data-gradient conv, for profiling joins:
// (stages << 12) | (fast << 8) | (mode << 4) | tile, tile 0 = 128x128, 1 = 128x64,
// 2 = 64x128, 3 = 64x64 (stages 0 on the register-staged path)
extern "C" int pose6d_conv_variant(int32_t dtype, int32_t pass, int32_t N, int32_t H, int32_t W, int32_t Cin,
                                   int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad, int32_t Ho,
                                   int32_t Wo) {
  const ConvShape cs{N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo};
  int mode;
  const Geom g = pass == 0 ? fwd_geom(dtype, cs, &mode) : dgrad_geom(cs, &mode);
  const Plan p = choose(dtype, mode, g, false, nullptr, pass == 0);
  return (p.g.splits << 16) | (p.stages << 12) | ((int)p.fast << 8) | (p.mode << 4) | p.tile;
}

// workgroups of the patch plan a stats-free forward of this geometry runs (0 = the
// implicit-GEMM plans of pose6d_conv_variant)
extern "C" int pose6d_conv_patch_plan(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                                      int32_t KH, int32_t KW, int32_t stride, int32_t pad, int32_t Ho, int32_t Wo) {
  const ConvShape cs{N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo};
  int mode;
  const Geom g = fwd_geom(dtype, cs, &mode);
  PatchPlan pp{};
  return patch_eligible(dtype, mode, g, nullptr, nullptr, &pp) ? pp.tiles * (Cout / kPatchBN) : 0;
}

// split-K workspace bytes of a forward (pass 0) / data-gradient (pass 1) conv's plan:
// 0 when the plan does not split K (then the workspace arguments may be NULL / 0)
extern "C" int64_t pose6d_conv_splitk_workspace_tuned(int32_t dtype, int32_t pass, int32_t N, int32_t H, int32_t W,
                                                      int32_t Cin, int32_t Cout, int32_t KH, int32_t KW,
                                                      int32_t stride, int32_t pad, int32_t Ho, int32_t Wo,
                                                      const pose6d_tuning_t* tuning) {
  const ConvShape cs{N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo};
  int mode;
  const Geom g = pass == 0 ? fwd_geom(dtype, cs, &mode) : dgrad_geom(cs, &mode);
  return splitk_need(choose(dtype, mode, g, false, tuning, pass == 0));
}

extern "C" int64_t pose6d_conv_splitk_workspace(int32_t dtype, int32_t pass, int32_t N, int32_t H, int32_t W,
                                                int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t stride,
                                                int32_t pad, int32_t Ho, int32_t Wo) {
  return pose6d_conv_splitk_workspace_tuned(dtype, pass, N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo, nullptr);
}

// fused backward variant (profiling joins): (1 << 16) | (dgrad mode << 4) | data-gradient
// ring stages when pose6d_conv2d_backward runs ONE conv_bwd_kernel launch, else 0
extern "C" int pose6d_bwd_variant(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                                  int32_t KH, int32_t KW, int32_t stride, int32_t pad, int32_t Ho, int32_t Wo) {
  const ConvShape cs{N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo};
  const BwdPlan bp = plan_backward(dtype, cs, nullptr);
  return bp.fused ? (1 << 16) | (bp.pd.mode << 4) | fused_ds(dtype, bp.pd.stages) : 0;
}

extern "C" int pose6d_wgrad_reduce(const pose6d_wgrad_reduce_t* job, void* stream) {
  P6_CHECK_ARG(job != nullptr, "pose6d_wgrad_reduce: null job");
  const ReduceJob r = make_job(*job);
  return p6::wgrad_reduce_launch(r.ws, r.dw, r.Cout, r.Kpad, r.SC, r.Cin, r.KH, r.KW, r.KWp, r.splits, r.accumulate,
                                 p6::stream_of(stream));
}

extern "C" int pose6d_conv2d_backward_chain(int32_t dtype, const void* x, const void* dy, const void* wt,
                                            const void* dres, void* dx, float* dw, int32_t accumulate,
                                            float* workspace, int64_t ws_bytes, int32_t N, int32_t H, int32_t W,
                                            int32_t Cin, int32_t Cin_real, int32_t Cout, int32_t KH, int32_t KW,
                                            int32_t stride, int32_t pad, int32_t Ho, int32_t Wo,
                                            const pose6d_wgrad_reduce_t* prev, int32_t* deferred, void* stream) {
  const ConvShape cs{N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo};
  ReduceJob r;
  const int rc = chain_job("pose6d_conv2d_backward_chain", prev, workspace, deferred, &r);
  if (rc) return rc;
  return conv_backward_impl(dtype, cs, {x, dy, wt, dres, nullptr, dx, dw, accumulate, workspace, ws_bytes, Cin_real}, 3,
                            stream, r, deferred);
}

extern "C" int pose6d_conv2d_backward_chain_masked(int32_t dtype, const void* x, const void* dy, const void* wt,
                                                   const void* dres, const uint8_t* dres_mask, void* dx, float* dw,
                                                   int32_t accumulate, float* workspace, int64_t ws_bytes, int32_t N,
                                                   int32_t H, int32_t W, int32_t Cin, int32_t Cin_real, int32_t Cout,
                                                   int32_t KH, int32_t KW, int32_t stride, int32_t pad, int32_t Ho,
                                                   int32_t Wo, const pose6d_wgrad_reduce_t* prev, int32_t* deferred,
                                                   void* stream) {
  const ConvShape cs{N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo};
  ReduceJob r;
  const int rc = chain_job("pose6d_conv2d_backward_chain_masked", prev, workspace, deferred, &r);
  if (rc) return rc;
  P6_CHECK_ARG(dres_mask != nullptr, "pose6d_conv2d_backward_chain_masked: null mask");
  return conv_backward_impl(dtype, cs, {x, dy, wt, dres, dres_mask, dx, dw, accumulate, workspace, ws_bytes, Cin_real},
                            3, stream, r, deferred);
}

// BatchNorm-reduce partial rows of this conv's data gradient (pose6d_bn_reduce_t::rows):
// the plan pose6d_conv2d_backward_chain_bn will run, one row per output tile
extern "C" int pose6d_conv2d_backward_bn_rows(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t Cin,
                                              int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad,
                                              int32_t Ho, int32_t Wo) {
  const ConvShape cs{N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo};
  return plan_backward(dtype, cs, nullptr).bn_rows;
}

extern "C" int pose6d_conv2d_backward_chain_bn(int32_t dtype, const void* x, const void* dy, const void* wt,
                                               const void* dres, const uint8_t* dres_mask, void* dx, float* dw,
                                               int32_t accumulate, float* workspace, int64_t ws_bytes, int32_t N,
                                               int32_t H, int32_t W, int32_t Cin, int32_t Cin_real, int32_t Cout,
                                               int32_t KH, int32_t KW, int32_t stride, int32_t pad, int32_t Ho,
                                               int32_t Wo, const pose6d_wgrad_reduce_t* prev, int32_t* deferred,
                                               const pose6d_bn_reduce_t* bn, void* stream) {
  const ConvShape cs{N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo};
  ReduceJob r;
  const int rc = chain_job("pose6d_conv2d_backward_chain_bn", prev, workspace, deferred, &r);
  if (rc) return rc;
  P6_CHECK_ARG(!dres_mask || dres, "pose6d_conv2d_backward_chain_bn: a mask needs dres");
  return conv_backward_impl(dtype, cs, {x, dy, wt, dres, dres_mask, dx, dw, accumulate, workspace, ws_bytes, Cin_real},
                            3, stream, r, deferred, nullptr, bn);
}
