// What the reference's inference scripts do AFTER the model call, for N detections in
// one launch: the bbox-centre translation correction of the RGB / RGBD scripts
// (inference_rgb.py:99-104, inference_rgbd.py:159-164) and the projection of the
// object's 3D box and axes (utils/visualization.py:8-32 project_points, :63-66 the axis
// points).  The reference does this on the host in numpy double, so everything here is
// fp64 (a few hundred flops per detection: latency, not throughput).  One thread per
// (detection, point); 12 points: the 8 box corners, the origin, the x / y / z axis tips
// at axis_scale.  Built with -ffp-contract=off: each product and sum rounds on its own,
// as numpy's do (numpy's 3-term matmul may still order or fuse its products differently).
#include "pose_geom.h"

namespace {

constexpr int kPts = 12;
constexpr int kThreads = 64;

// numpy's astype(int) of a double on x86-64: truncation toward zero; a NaN, an infinity or
// a value outside int64 gives INT64_MIN (cvttsd2si's "integer indefinite")
__device__ __forceinline__ int64_t trunc_i64(double v) {
  return fabs(v) < 9223372036854775808.0 ? (int64_t)v : INT64_MIN;
}

__global__ __launch_bounds__(kThreads) void pose_project_kernel(
    const float* __restrict__ quat, const float* __restrict__ trans, const int32_t* __restrict__ boxes,
    const double* __restrict__ K, int K_per_frame, const int32_t* __restrict__ frame_of, int F,
    const int64_t* __restrict__ obj, const double* __restrict__ corners, int64_t n_obj, double axis_scale, int N,
    double* __restrict__ trans_out, double* __restrict__ pts_out, int64_t* __restrict__ pix_out,
    uint8_t* __restrict__ valid_out) {
  const int gid = blockIdx.x * kThreads + threadIdx.x;
  if (gid >= N * kPts) return;
  const int i = gid / kPts, p = gid - i * kPts;
  const int f = (K_per_frame && frame_of) ? frame_of[i] : 0;
  const int64_t ob = obj[i];
  // scipy Rotation.from_quat: float64, q / sqrt(x^2 + y^2 + z^2 + w^2)
  double q[4];
  const double nrm = p6::quat_load(quat + 4 * i, q);
  const bool ok = ob >= 0 && ob < n_obj && nrm > 0.0 && f >= 0 && f < F;
  if (!ok) {   // nothing is read through the bad index
    if (p == 0) {
      if (valid_out) valid_out[i] = 0;
      if (trans_out) trans_out[3 * i] = trans_out[3 * i + 1] = trans_out[3 * i + 2] = 0.0;
    }
    if (pts_out) pts_out[2 * gid] = pts_out[2 * gid + 1] = 0.0;
    if (pix_out) pix_out[2 * gid] = pix_out[2 * gid + 1] = 0;
    return;
  }
  const double* k = K + 9 * (int64_t)f;
  double tx = (double)trans[3 * i], ty = (double)trans[3 * i + 1];
  const double tz = (double)trans[3 * i + 2];
  if (boxes) {   // inference_rgb.py:99-104: x, y from the box centre's ray at the predicted z
    const int32_t* bx = boxes + 4 * i;
    const double c_x = ((double)bx[0] + (double)bx[2]) / 2.0, c_y = ((double)bx[1] + (double)bx[3]) / 2.0;
    tx = (c_x - k[2]) * tz / k[0];
    ty = (c_y - k[5]) * tz / k[4];
  }
  if (p == 0) {
    if (valid_out) valid_out[i] = 1;
    if (trans_out) { trans_out[3 * i] = tx; trans_out[3 * i + 1] = ty; trans_out[3 * i + 2] = tz; }
  }
  double R[9];
  p6::quat_unit(q, nrm);   // (the sign it may flip cancels in every entry of R)
  p6::quat_to_mat(q, R);
  double c0 = 0.0, c1 = 0.0, c2 = 0.0;
  if (p < 8) {
    const double* c = corners + (ob * 8 + p) * 3;
    c0 = c[0]; c1 = c[1]; c2 = c[2];
  } else if (p == 9) {
    c0 = axis_scale;
  } else if (p == 10) {
    c1 = axis_scale;
  } else if (p == 11) {
    c2 = axis_scale;
  }
  // project_points (visualization.py:26-31)
  const double px = R[0] * c0 + R[1] * c1 + R[2] * c2 + tx;
  const double py = R[3] * c0 + R[4] * c1 + R[5] * c2 + ty;
  const double pz = R[6] * c0 + R[7] * c1 + R[8] * c2 + tz;
  const double zc = pz < 0.001 ? 0.001 : pz;   // np.clip(z, 0.001, None); a NaN stays a NaN
  const double u = px * k[0] / zc + k[2];
  const double v = py * k[4] / zc + k[5];
  if (pts_out) { pts_out[2 * gid] = u; pts_out[2 * gid + 1] = v; }
  if (pix_out) { pix_out[2 * gid] = trunc_i64(u); pix_out[2 * gid + 1] = trunc_i64(v); }
}

}  // namespace

extern "C" int pose6d_pose_project(const float* quat, const float* trans, const int32_t* boxes_xyxy, const double* K,
                                   int32_t K_per_frame, const int32_t* frame_of, int32_t F, const int64_t* obj,
                                   const double* corners, int64_t n_obj, double axis_scale, int32_t N,
                                   double* trans_out, double* pts_out, int64_t* pix_out, uint8_t* valid_out,
                                   void* stream) {
  P6_CHECK_ARG(quat != nullptr && trans != nullptr && K != nullptr && obj != nullptr && corners != nullptr,
               "pose6d_pose_project: quat, trans, K, obj and corners are required");
  P6_CHECK_ARG(N >= 0 && N <= (1 << 24) && n_obj >= 0 && F > 0, "pose6d_pose_project: bad shape");
  if (N == 0) return POSE6D_OK;
  pose_project_kernel<<<p6::ceil_div((int64_t)N * kPts, kThreads), kThreads, 0, p6::stream_of(stream)>>>(
      quat, trans, boxes_xyxy, K, K_per_frame, frame_of, F, obj, corners, n_obj, axis_scale, N, trans_out, pts_out,
      pix_out, valid_out);
  P6_LAUNCH_CHECK();
  return POSE6D_OK;
}
