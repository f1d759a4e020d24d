// Depth refinement of estimated poses: point-to-point ICP between the back-projected
// depth inside each detection box and the object's mesh points, N detections in ONE
// launch (pose6d_depth_refine).  The reference project has no refinement step; the
// yardstick is the fp64 numpy restatement tests/refine_ref.py.
//
// One workgroup per detection, one lane per sample of the G x G grid over the box
// (P = G * G <= 1024 lanes).  Per detection:
//   samples   pixel (u, v) by integer floor division, valid inside the frame with depth
//             > 0, back-projected in double; kept when within gate * diam of the INITIAL
//             translation (the gate centre never moves: it removes the background);
//   iterate   q = R^T (p - t) in double, rounded to float once; nearest mesh point by
//             direct float differences against the mesh staged in LDS (three float
//             arrays, 4096 points = 48 KiB per tile; every lane reads the same point: a
//             broadcast), first index on a tie; accepted when sqrt(s) <= trim * diam;
//             fp64 moments of the accepted pairs reduced per wave by shuffles and across
//             waves through LDS in wave order (no atomics, a fixed order: the bits
//             repeat); Horn's closed form on lane 0 -- the eigenvector of the largest
//             eigenvalue of the 4 x 4 symmetric matrix of the centred cross-covariance by
//             cyclic Jacobi, a fixed number of sweeps -- a unit quaternion, so a proper
//             rotation by construction; t = mean(p) - R mean(m); the new pose goes to
//             every lane through LDS behind a barrier.
// A mesh that fits one tile is staged once (the mesh stays in the model frame, the
// samples move); a larger one is streamed tile by tile in every iteration.  A wave
// without a kept sample skips the search (it still meets every barrier).
//
// Built with -ffp-contract=off: the back-projection and the gate round product by
// product, as numpy does, so the kept set equals the restatement's bit for bit; the
// only fused operations are the explicit fmaf calls of the squared distance.
#include "pose_geom.h"

namespace {

constexpr int kTile = 4096;      // mesh points per LDS tile (3 float arrays: 48 KiB)
constexpr int kMaxWaves = 16;    // 1024 lanes
constexpr int kMom = 17;         // n, sum p' [3], sum m [3], sum m p'^T [9], sum s
constexpr int kSweeps = 6;       // cyclic Jacobi sweeps on the 4 x 4 (quadratic convergence: 4 leave
                                 // 6e-8 rad, 5 reach fp64 roundoff on random pair sets; one is margin)

// one Jacobi rotation of the symmetric A (and the eigenvector matrix V) in the (P, Q) plane
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&A)[4][4], double (&V)[4][4]) {
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  // the smaller root of t^2 + 2 theta t - 1 = 0; a huge theta gives t = 0
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double akp = A[k][P], akq = A[k][Q];
    A[k][P] = c * akp - s * akq;
    A[k][Q] = s * akp + c * akq;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double apk = A[P][k], aqk = A[Q][k];
    A[P][k] = c * apk - s * aqk;
    A[Q][k] = s * apk + c * aqk;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double vkp = V[k][P], vkq = V[k][Q];
    V[k][P] = c * vkp - s * vkq;
    V[k][Q] = s * vkp + c * vkq;
  }
}

// Horn 1987: the rotation that takes the centred m onto the centred p, as a unit
// quaternion (x, y, z, w) with w >= 0.  S[3 a + c] = sum m_a p_c (centred).
__device__ void horn_quat(const double* S, double* q) {
  const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7],
               Szz = S[8];
  double A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                    {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                    {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                    {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < kSweeps; ++sweep) {
    jacobi_rotate<0, 1>(A, V);
    jacobi_rotate<0, 2>(A, V);
    jacobi_rotate<0, 3>(A, V);
    jacobi_rotate<1, 2>(A, V);
    jacobi_rotate<1, 3>(A, V);
    jacobi_rotate<2, 3>(A, V);
  }
  // the column of the largest eigenvalue (the first on a tie), (w, x, y, z)
  double best = A[0][0];
  double e[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    if (A[k][k] > best) {
      best = A[k][k];
#pragma unroll
      for (int r = 0; r < 4; ++r) e[r] = V[r][k];
    }
  }
  const double nrm = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2] + e[3] * e[3]);
  const double sg = e[0] < 0.0 ? -1.0 : 1.0;
  q[0] = sg * e[1] / nrm; q[1] = sg * e[2] / nrm; q[2] = sg * e[3] / nrm; q[3] = sg * e[0] / nrm;
}

struct RefineArgs : p6::FrameArgs {
  const float* points; const int32_t* off; const int32_t* npts; const double* diam; int n_slots;
  const float* quat; const double* trans;
  int G, iters; double gate, trim; int min_points;
  double* quat_out; double* trans_out; float* quat32_out; float* trans32_out;
  int32_t* n_corr; double* rms; uint8_t* refined;
  double* pose_trace; int32_t* corr_out; double* samples_out;
};

__global__ __launch_bounds__(1024) void depth_refine_kernel(const RefineArgs a) {
  __shared__ __attribute__((aligned(16))) float mx[kTile];
  __shared__ __attribute__((aligned(16))) float my[kTile];
  __shared__ __attribute__((aligned(16))) float mz[kTile];
  __shared__ double red[kMaxWaves][kMom];
  __shared__ double pose_s[16];   // R [9], t [3], q [4] (x, y, z, w)
  __shared__ int go_s;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int G = a.G, P = G * G, iters = a.iters;

  const p6::Detection det = p6::read_detection(a, a.n_slots, a.npts, a.quat, b);
  const int64_t ob = det.ob;
  const double* q0 = det.q;
  const double t0[3] = {a.trans[3 * b], a.trans[3 * b + 1], a.trans[3 * b + 2]};
  const int n = det.n;

  // the final outputs (thread 0) and the rest of the debug rows
  auto finish = [&](int done, const double* q, const double* t, int nc, double rms0, double rms1, int ref) {
    if (tid == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        a.quat_out[4 * b + k] = q[k];
        if (a.quat32_out) a.quat32_out[4 * b + k] = (float)q[k];
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        a.trans_out[3 * b + k] = t[k];
        if (a.trans32_out) a.trans32_out[3 * b + k] = (float)t[k];
      }
      a.n_corr[b] = nc;
      a.rms[2 * b] = rms0;
      a.rms[2 * b + 1] = rms1;
      a.refined[b] = (uint8_t)ref;
      if (a.pose_trace) {   // `done` iterations ran: rows 0 .. done are written, the last pose repeats
        for (int r = done + 1; r <= iters; ++r) {
          double* row = a.pose_trace + ((int64_t)b * (iters + 1) + r) * 7;
          for (int k = 0; k < 4; ++k) row[k] = q[k];
          for (int k = 0; k < 3; ++k) row[4 + k] = t[k];
        }
      }
    }
    if (a.corr_out && tid < P)
      for (int r = done; r < iters; ++r) a.corr_out[((int64_t)b * iters + r) * P + tid] = -2;
  };
  auto trace_row = [&](int r, const double* q, const double* t) {   // thread 0
    if (!a.pose_trace) return;
    double* row = a.pose_trace + ((int64_t)b * (iters + 1) + r) * 7;
    for (int k = 0; k < 4; ++k) row[k] = q[k];
    for (int k = 0; k < 3; ++k) row[4 + k] = t[k];
  };

  if (!det.ok) {   // nothing is read through the bad index
    if (tid == 0) trace_row(0, q0, t0);
    if (a.samples_out && tid < P)
      for (int k = 0; k < 3; ++k) a.samples_out[((int64_t)b * P + tid) * 3 + k] = __builtin_nan("");
    finish(0, q0, t0, 0, 0.0, 0.0, 0);
    return;
  }

  // ---- samples
  const double diam = a.diam[ob];
  const double gate_r = a.gate * diam, trim_r = a.trim * diam;
  bool kept = false;
  double pc[3] = {0.0, 0.0, 0.0};   // the sample relative to the initial translation
  if (tid < P) {
    const int64_t u = p6::sample_pixel(det.box[0], det.box[2], tid % G, G);
    const int64_t v = p6::sample_pixel(det.box[1], det.box[3], tid / G, G);
    double p[3] = {__builtin_nan(""), __builtin_nan(""), __builtin_nan("")};
    const uint16_t d = p6::depth_at(a, det.f, u, v);
    if (d > 0) {
      const double z = (double)d * a.depth_scale;
      const double x = ((double)u - det.k[2]) * z / det.k[0];
      const double y = ((double)v - det.k[5]) * z / det.k[4];
      const double dx = x - t0[0], dy = y - t0[1], dz = z - t0[2];
      kept = sqrt(dx * dx + dy * dy + dz * dz) <= gate_r;
      if (kept) { p[0] = x; p[1] = y; p[2] = z; pc[0] = dx; pc[1] = dy; pc[2] = dz; }
    }
    if (a.samples_out)
      for (int k = 0; k < 3; ++k) a.samples_out[((int64_t)b * P + tid) * 3 + k] = p[k];
  }
  const bool wave_any = __ballot(kept) != 0;

  // ---- the mesh: one tile is staged once, a larger mesh in every iteration
  const float* Pm = a.points + 3 * (int64_t)a.off[ob];
  auto stage = [&](int j0) {
    const int jn = min(kTile, n - j0), jpad = (jn + 3) & ~3;   // padded to whole trips with +inf (never a minimum)
    for (int jj = tid; jj < jpad; jj += blockDim.x) {
      const bool in = jj < jn;
      mx[jj] = in ? Pm[3 * (int64_t)(j0 + jj)] : __builtin_inff();
      my[jj] = in ? Pm[3 * (int64_t)(j0 + jj) + 1] : __builtin_inff();
      mz[jj] = in ? Pm[3 * (int64_t)(j0 + jj) + 2] : __builtin_inff();
    }
  };
  const bool one_tile = n <= kTile;
  if (one_tile) stage(0);
  if (tid == 0) {
    p6::quat_to_mat(q0, pose_s);
    for (int k = 0; k < 3; ++k) pose_s[9 + k] = t0[k];
    for (int k = 0; k < 4; ++k) pose_s[12 + k] = q0[k];
    trace_row(0, q0, t0);
  }
  __syncthreads();

  int done = 0, nc_last = 0;            // thread 0's bookkeeping
  double rms_first = 0.0, rms_last = 0.0;
  for (int it = 0; it < iters; ++it) {
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = pose_s[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = pose_s[9 + k];
    // q = R^T (p - t), p - t = pc + (t0 - t)
    const double dx = pc[0] + (t0[0] - t[0]), dy = pc[1] + (t0[1] - t[1]), dz = pc[2] + (t0[2] - t[2]);
    const float qx = (float)(R[0] * dx + R[3] * dy + R[6] * dz);
    const float qy = (float)(R[1] * dx + R[4] * dy + R[7] * dz);
    const float qz = (float)(R[2] * dx + R[5] * dy + R[8] * dz);
    // an idle lane never updates: nothing is below -inf
    float best = kept ? __builtin_inff() : -__builtin_inff();
    int bi = -1;
    for (int j0 = 0; j0 < n; j0 += kTile) {
      if (!one_tile) {
        __syncthreads();
        stage(j0);
        __syncthreads();
      }
      if (!wave_any) continue;
      const int jpad = (min(kTile, n - j0) + 3) & ~3;
      for (int jj = 0; jj < jpad; jj += 4) {
        const float4 gx = *reinterpret_cast<const float4*>(mx + jj);
        const float4 gy = *reinterpret_cast<const float4*>(my + jj);
        const float4 gz = *reinterpret_cast<const float4*>(mz + jj);
        const float ax[4] = {gx.x, gx.y, gx.z, gx.w}, ay[4] = {gy.x, gy.y, gy.z, gy.w},
                    az[4] = {gz.x, gz.y, gz.z, gz.w};
        float s[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float ex = qx - ax[u], ey = qy - ay[u], ez = qz - az[u];
          s[u] = fmaf(ez, ez, fmaf(ey, ey, ex * ex));
        }
        // one uniform branch per trip of four: does any lane of the wave improve?
        const float m = __builtin_fminf(__builtin_fminf(s[0], s[1]), __builtin_fminf(s[2], s[3]));
        if (__ballot(m < best) != 0) {
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (s[u] < best) { best = s[u]; bi = j0 + jj + u; }   // strict: the first index keeps a tie
        }
      }
    }
    const bool acc = kept && bi >= 0 && sqrt((double)best) <= trim_r;
    double mom[kMom];
#pragma unroll
    for (int k = 0; k < kMom; ++k) mom[k] = 0.0;
    if (acc) {
      const double m3[3] = {(double)Pm[3 * (int64_t)bi], (double)Pm[3 * (int64_t)bi + 1],
                            (double)Pm[3 * (int64_t)bi + 2]};
      mom[0] = 1.0;
#pragma unroll
      for (int c = 0; c < 3; ++c) { mom[1 + c] = pc[c]; mom[4 + c] = m3[c]; }
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) mom[7 + 3 * r + c] = m3[r] * pc[c];
      mom[16] = (double)best;
    }
#pragma unroll
    for (int k = 0; k < kMom; ++k) {
      const double v = p6::wave_sum(mom[k]);
      if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (tid == 0) {
      double T[kMom];
      for (int k = 0; k < kMom; ++k) {
        double v = 0.0;
        for (int w = 0; w < nw; ++w) v += red[w][k];   // wave order
        T[k] = v;
      }
      const int cnt = (int)T[0];
      if (cnt < a.min_points) {
        go_s = 0;
      } else {
        const double inv = 1.0 / T[0];
        const double pb[3] = {T[1] * inv, T[2] * inv, T[3] * inv}, mb[3] = {T[4] * inv, T[5] * inv, T[6] * inv};
        double S[9];
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) S[3 * r + c] = T[7 + 3 * r + c] - T[0] * mb[r] * pb[c];
        double qn4[4], Rn[9], tn[3];
        horn_quat(S, qn4);
        p6::quat_to_mat(qn4, Rn);
        for (int r = 0; r < 3; ++r)
          tn[r] = t0[r] + (pb[r] - (Rn[3 * r] * mb[0] + Rn[3 * r + 1] * mb[1] + Rn[3 * r + 2] * mb[2]));
        for (int k = 0; k < 9; ++k) pose_s[k] = Rn[k];
        for (int k = 0; k < 3; ++k) pose_s[9 + k] = tn[k];
        for (int k = 0; k < 4; ++k) pose_s[12 + k] = qn4[k];
        trace_row(it + 1, qn4, tn);
        const double r_ = sqrt(T[16] * inv);
        if (it == 0) rms_first = r_;
        rms_last = r_;
        nc_last = cnt;
        done = it + 1;
        go_s = 1;
      }
    }
    __syncthreads();
    const int go = go_s;
    if (!go) break;
    if (a.corr_out && tid < P) a.corr_out[((int64_t)b * iters + it) * P + tid] = acc ? bi : -1;
    done = it + 1;   // (every thread: the rows finish() fills start here)
  }
  double qf[4], tf[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) qf[k] = pose_s[12 + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) tf[k] = pose_s[9 + k];
  // fewer than min_points pairs in the first iteration: the input pose, unrefined
  finish(done, qf, tf, nc_last, rms_first, rms_last, done > 0 ? 1 : 0);
}

}  // namespace

extern "C" int pose6d_depth_refine(const uint16_t* depth, int32_t F, int32_t H, int32_t W, double depth_scale,
                                   const double* K, int32_t K_per_frame, const int32_t* boxes_xyxy,
                                   const int32_t* frame_of, const int64_t* obj, const float* points,
                                   const int32_t* off, const int32_t* npts, const double* diam, int32_t n_slots,
                                   const float* quat, const double* trans, int32_t N, int32_t G, int32_t iters,
                                   double gate, double trim, int32_t min_points, double* quat_out, double* trans_out,
                                   float* quat32_out, float* trans32_out, int32_t* n_corr, double* rms,
                                   uint8_t* refined, double* pose_trace, int32_t* corr_out, double* samples_out,
                                   void* stream) {
  P6_CHECK_ARG(G >= 1 && G <= 32, "pose6d_depth_refine: G must be in [1, 32] (got %d)", (int)G);
  P6_CHECK_ARG(iters >= 1 && iters <= 64, "pose6d_depth_refine: iters must be in [1, 64] (got %d)", (int)iters);
  P6_CHECK_ARG(min_points >= 3, "pose6d_depth_refine: min_points must be at least 3 (got %d)", (int)min_points);
  P6_CHECK_ARG(gate > 0.0 && gate < __builtin_inf() && trim > 0.0 && trim < __builtin_inf(),
               "pose6d_depth_refine: gate and trim must be positive and finite");
  P6_CHECK_ARG(depth_scale > 0.0 && depth_scale < __builtin_inf(),
               "pose6d_depth_refine: depth_scale must be positive and finite");
  P6_CHECK_ARG(N >= 0 && N <= 65535 && F > 0 && H > 0 && W > 0 && n_slots >= 0, "pose6d_depth_refine: bad shape");
  if (N == 0) return POSE6D_OK;
  P6_CHECK_ARG(depth && K && boxes_xyxy && obj && quat && trans, "pose6d_depth_refine: null input");
  P6_CHECK_ARG(n_slots == 0 || (points && off && npts && diam), "pose6d_depth_refine: null mesh table");
  P6_CHECK_ARG(quat_out && trans_out && n_corr && rms && refined, "pose6d_depth_refine: null output");
  const RefineArgs a = {{depth, F, H, W, depth_scale, K, K_per_frame, boxes_xyxy, frame_of, obj}, points, off, npts,
                        diam, n_slots, quat, trans, G, iters, gate, trim, min_points, quat_out, trans_out,
                        quat32_out, trans32_out, n_corr, rms, refined, pose_trace, corr_out, samples_out};
  const int threads = (G * G + 63) & ~63;
  depth_refine_kernel<<<(unsigned)N, threads, 0, p6::stream_of(stream)>>>(a);
  P6_LAUNCH_CHECK();
  return POSE6D_OK;
}
