// Shared pieces of the BatchNorm2d training finalize (bn.hip): the channel result
// every finalize kernel forms from its fold, and the write-through accesses that hand
// scale / shift to other workgroups of the same launch (pose6d_bn_finalize_act).
//
// Partials are [2][C][rows] fp32 (row i: sum and M2 about the block mean of 32 output
// pixels; the last row may hold fewer).  One workgroup per channel folds them as shifted
// sums about K = row 0's mean (bn_stats_fold in bn.hip), and bn_fold_result forms
// mean = K + S1/N, var = (S2 - S1^2/N)/N from the sums.  Contraction is off so that every
// kernel inlining it rounds identically.
#pragma once
#include "common.h"

namespace p6 {

// write-through (sc1) accesses through a buffer resource: scale / shift and the ready
// flags of a finalize that other workgroups of the SAME launch read (bn.hip
// pose6d_bn_finalize_act): the hand-off MI355X_MICROARCH.md measures valid with sc1
// stores and sc1 loads on both sides (the storing waves wait for their stores, one
// lane then stores the flag)
constexpr int kSc1 = 16;   // buffer cache-policy bits: sc1
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_of(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7fffffff, 0x00020000);
}
__device__ __forceinline__ void st_sc1(float* p, int i, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsrc_of(p), i * 4, 0, kSc1);
}
__device__ __forceinline__ void st_sc1(int* p, int i, int v) {
  __builtin_amdgcn_raw_buffer_store_b32((unsigned)v, rsrc_of(p), i * 4, 0, kSc1);
}
__device__ __forceinline__ int ld_sc1(const int* p, int i) {
  return (int)__builtin_amdgcn_raw_buffer_load_b32(rsrc_of(p), i * 4, 0, kSc1);
}
__device__ __forceinline__ f32x4 ld_sc1_x4(const float* p, int i) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_of(p), i * 4, 0, kSc1));
}

// the channel's mean / biased var / invstd / scale / shift from its fold (fp64; the
// arithmetic of every finalize -- keep in one place so all of them round alike)
struct BnFoldOut {
  double mean, var;
  float inv, sc, sh;
};
__device__ __forceinline__ BnFoldOut bn_fold_result(int64_t M, float eps, double K, double s1, double s2, float g_c,
                                                    float b_c) {
#pragma clang fp contract(off)
  BnFoldOut o;
  const double N = (double)M;
  o.mean = K + s1 / N;
  o.var = (s2 - s1 * s1 / N) / N;
  if (o.var < 0.0) o.var = 0.0;
  o.inv = (float)(1.0 / sqrt(o.var + (double)eps));
  o.sc = g_c * o.inv;
  o.sh = b_c - (float)o.mean * o.sc;
  return o;
}

}  // namespace p6
