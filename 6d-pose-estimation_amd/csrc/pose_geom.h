// Pose-against-frame geometry shared by refine.hip, verify.hip and pose_project.hip: fp64,
// every product rounding on its own as numpy's do.  ONLY for files of the Makefile's EXACT
// list (built with -ffp-contract=off) -- include it from nothing else: under the default
// contraction these expressions fuse and the bit-exact tests of the three kernels fail.
#pragma once
#include <math.h>

#include "common.h"

namespace p6 {

__device__ __forceinline__ int64_t floor_div(int64_t a, int64_t b) {   // b > 0
  const int64_t q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// unit quaternion (x, y, z, w) -> rotation matrix, row-major (scipy's Rotation.as_matrix)
__device__ __forceinline__ void quat_to_mat(const double* q, double* R) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
  const double xy = x * y, zw = z * w, xz = x * z, yw = y * w, yz = y * z, xw = x * w;
  R[0] = x2 - y2 - z2 + w2; R[1] = 2.0 * (xy - zw);    R[2] = 2.0 * (xz + yw);
  R[3] = 2.0 * (xy + zw);   R[4] = -x2 + y2 - z2 + w2; R[5] = 2.0 * (yz - xw);
  R[6] = 2.0 * (xz - yw);   R[7] = 2.0 * (yz + xw);    R[8] = -x2 - y2 + z2 + w2;
}

// fp32 quaternion -> q in double, as read; returns its norm (which norms are valid is the
// caller's rule).  quat_unit divides by it with w >= 0; the sign cancels in quat_to_mat.
__device__ __forceinline__ double quat_load(const float* q32, double* q) {
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = (double)q32[k];
  return sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
}
__device__ __forceinline__ void quat_unit(double* q, double qn) {
  const double sg = q[3] < 0.0 ? -1.0 : 1.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = sg * q[k] / qn;
}

// the leading arguments of pose6d_depth_refine and pose6d_pose_verify
struct FrameArgs {
  const uint16_t* depth; int F, H, W; double depth_scale;
  const double* K; int K_per_frame;
  const int32_t* boxes; const int32_t* frame_of; const int64_t* obj;
};

// One detection's header (the same words for every thread: branches on them are uniform).
// n: count[ob], the slot's points or triangles (0 for a slot outside [0, n_slots)); q: the unit
// quaternion when its norm is positive and finite, else as read (zero, NaN, infinite); ok: that,
// n > 0 and f in [0, F) -- when false, nothing may be read through ob or f; k: K's row of f.
struct Detection { int64_t ob; int f, n; bool ok; double q[4]; const double* k; const int32_t* box; };
__device__ __forceinline__ Detection read_detection(const FrameArgs& a, int n_slots, const int32_t* count,
                                                     const float* quat, int b) {
  Detection d;
  d.ob = a.obj[b];
  d.f = a.frame_of ? a.frame_of[b] : 0;
  d.n = (d.ob >= 0 && d.ob < n_slots) ? count[d.ob] : 0;
  const double qn = quat_load(quat + 4 * b, d.q);
  const bool q_ok = qn > 0.0 && qn < __builtin_inf();
  if (q_ok) quat_unit(d.q, qn);
  d.ok = q_ok && d.n > 0 && d.f >= 0 && d.f < a.F;
  d.k = a.K + ((d.ok && a.K_per_frame && a.frame_of) ? 9 * (int64_t)d.f : 0);
  d.box = a.boxes + 4 * b;
  return d;
}

// pixel of sample i of G over [x1, x2), x1 + floor((2i + 1)(x2 - x1) / 2G): the one grid of
// pose6d_depth_refine and pose6d_pose_verify (tests/refine_ref.py sample_pixels)
__device__ __forceinline__ int64_t sample_pixel(int x1, int x2, int i, int G) {
  return (int64_t)x1 + floor_div((int64_t)(2 * i + 1) * ((int64_t)x2 - (int64_t)x1), 2 * G);
}

// depth of pixel (u, v) of frame f (in [0, F)); 0, "no depth", outside the frame
__device__ __forceinline__ uint16_t depth_at(const FrameArgs& a, int f, int64_t u, int64_t v) {
  return (u >= 0 && u < a.W && v >= 0 && v < a.H) ? a.depth[((int64_t)f * a.H + v) * a.W + u] : (uint16_t)0;
}

}  // namespace p6
