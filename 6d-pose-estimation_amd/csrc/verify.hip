// Render-and-compare verification of estimated poses: the object's triangle mesh rendered
// at the pose into a G x G z-buffer over the detection box and compared, sample by sample,
// with the depth frame -- N detections in ONE launch (pose6d_pose_verify).  The reference
// project has no such step; the yardstick is the fp64 numpy restatement
// tests/verify_ref.py, which tests every triangle against every sample.
//
// One workgroup of 1024 lanes per detection.  Per detection:
//   samples   the refiner's grid (pose_geom.h sample_pixel), G doubles per axis in LDS;
//   render    lanes stride over the triangles.  A lane projects its triangle's three
//             vertices in double (c = R m + t row by row, left to right; pu = c.x * fx / c.z
//             + cx), maps the triangle's pixel bounding box to a range of sample columns and
//             rows (a superset, derived at sample_range; the whole grid when the box is
//             inverted) and tests the samples of that range against the bounding box, exactly,
//             and with the three edge functions; a covered sample takes the minimum of its
//             rendered depth by an unsigned 64-bit atomic minimum on the bit pattern in LDS.  Every z
//             that reaches the buffer is positive and finite, so the unsigned order is the
//             order of the values and the result does not depend on who came first; all
//             ones is "no hit".  G = 64: 32 KiB of LDS.
//   compare   lanes stride over the samples: class 0 no hit, 1 hit without depth, 2
//             consistent, 3 occluded, 4 violated; the five counts and the sum of |z_obs - z|
//             over class 2 are reduced per wave by shuffles and across waves through LDS in
//             wave order (no floating-point atomics: the bits repeat).
// The vertices are projected once per triangle that uses them, not once each: a table of
// projected vertices would not fit LDS for a mesh of LineMOD's size (14 406 vertices x 24
// bytes), and the arithmetic is the same either way.
//
// Built with -ffp-contract=off: every product rounds on its own, as numpy's do, so the
// z-buffer equals the restatement's bit for bit.  Plain C++ only.
#include "pose_geom.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxG = 64;
constexpr unsigned long long kNoHit = ~0ull;

// A superset of the sample indices i in [0, G) whose pixel x1 + floor((2i + 1) w / 2G) lies in
// [lo, hi] (finite), for w = x2 - x1 > 0.  With r_i = (2i + 1) w / 2G the pixel is in (x1 + r_i
// - 1, x1 + r_i], so a pixel >= lo needs i >= X = ((lo - x1) 2G / w - 1) / 2 and a pixel <= hi
// needs i < Y = ((hi + 1 - x1) 2G / w - 1) / 2, that is i <= ceil(Y) - 1.  Sample pixels are
// below 2^33 in magnitude, so lo and hi are clamped to +-2^33 first: X and Y stay below 2^41
// and their computed values X', Y' are within 2^-10 of them, hence floor(X') <= ceil(X) and
// ceil(Y') >= ceil(Y) - 1: [floor(X'), ceil(Y')] misses nothing.  An inverted or empty box
// keeps the whole grid.  (The range only saves work: the loop tests every sample of it
// against [lo, hi] exactly.)
__device__ __forceinline__ void sample_range(double lo, double hi, int x1, int x2, int G, int& i0, int& i1) {
  i0 = 0;
  i1 = G - 1;
  const double w = (double)x2 - (double)x1, lim = 8589934592.0;
  if (!(w > 0.0)) return;
  if (lo > lim || hi < -lim) { i1 = -1; return; }
  lo = fmax(lo, -lim);
  hi = fmin(hi, lim);
  const double k = 2.0 * (double)G / w;
  const double a = floor(((lo - (double)x1) * k - 1.0) * 0.5);
  const double b = ceil(((hi + 1.0 - (double)x1) * k - 1.0) * 0.5);
  i0 = (int)fmin(fmax(a, 0.0), (double)G);          // G: an empty range
  i1 = (int)fmax(fmin(b, (double)(G - 1)), -1.0);   // -1: an empty range
}

struct VerifyArgs : p6::FrameArgs {
  const float* verts; const int32_t* faces; const int32_t* voff; const int32_t* nverts; const int32_t* toff;
  const int32_t* ntri; const double* diam; int n_slots;
  const float* quat; const double* trans;
  int G; double tau;
  int32_t* counts; double* fit; double* agree; double* resid; uint8_t* verified;
  double* zbuf_out; uint8_t* cls_out;
  const double* base_fit; const uint8_t* base_flag; uint8_t* best;
};

__global__ __launch_bounds__(kThreads) void pose_verify_kernel(const VerifyArgs a) {
  __shared__ unsigned long long zb[kMaxG * kMaxG];
  __shared__ double us[kMaxG], vs[kMaxG];
  __shared__ int red_n[kWaves][5];
  __shared__ double red_r[kWaves];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = a.G, P = G * G;

  const p6::Detection det = p6::read_detection(a, a.n_slots, a.ntri, a.quat, b);
  const int64_t ob = det.ob;
  const int nt = det.n;
  if (!det.ok) {   // nothing is read through the bad index
    if (tid == 0) {
      for (int k = 0; k < 5; ++k) a.counts[5 * b + k] = 0;
      a.fit[b] = a.agree[b] = a.resid[b] = 0.0;
      a.verified[b] = 0;
      if (a.best) a.best[b] = 0;
    }
    for (int k = tid; k < P; k += kThreads) {
      if (a.zbuf_out) a.zbuf_out[(int64_t)b * P + k] = __builtin_inf();
      if (a.cls_out) a.cls_out[(int64_t)b * P + k] = 0;
    }
    return;
  }
  double R[9];
  p6::quat_to_mat(det.q, R);
  const double t[3] = {a.trans[3 * b], a.trans[3 * b + 1], a.trans[3 * b + 2]};
  const double fx = det.k[0], cx = det.k[2], fy = det.k[4], cy = det.k[5];
  const int x1 = det.box[0], y1 = det.box[1], x2 = det.box[2], y2 = det.box[3];

  // ---- samples and an empty z-buffer
  if (tid < G) {
    us[tid] = (double)p6::sample_pixel(x1, x2, tid, G);   // exact: below 2^33
    vs[tid] = (double)p6::sample_pixel(y1, y2, tid, G);
  }
  for (int k = tid; k < P; k += kThreads) zb[k] = kNoHit;
  __syncthreads();

  // ---- render: lanes stride over the triangles
  const int nv = a.nverts[ob];
  const float* V = a.verts + 3 * (int64_t)a.voff[ob];
  const int32_t* T = a.faces + 3 * (int64_t)a.toff[ob];
  // The loads of a triangle are issued together, its three indices one trip ahead: per trip
  // a lane waits for memory once (the nine coordinates), not six times in a chain.
  int32_t nxt[3] = {0, 0, 0};
  if (tid < nt)
    for (int c = 0; c < 3; ++c) nxt[c] = T[3 * (int64_t)tid + c];
  for (int tri = tid; tri < nt; tri += kThreads) {
    const int32_t idx[3] = {nxt[0], nxt[1], nxt[2]};
    if (tri + kThreads < nt)
      for (int c = 0; c < 3; ++c) nxt[c] = T[3 * (int64_t)(tri + kThreads) + c];
    bool use = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) use = use && idx[c] >= 0 && idx[c] < nv;
    if (!use) continue;   // never dereferenced
    float m[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int k = 0; k < 3; ++k) m[c][k] = V[3 * (int64_t)idx[c] + k];
    double pu[3], pv[3], pz[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double mx = (double)m[c][0], my = (double)m[c][1], mz = (double)m[c][2];
      const double px = ((R[0] * mx + R[1] * my) + R[2] * mz) + t[0];
      const double py = ((R[3] * mx + R[4] * my) + R[5] * mz) + t[1];
      pz[c] = ((R[6] * mx + R[7] * my) + R[8] * mz) + t[2];
      pu[c] = px * fx / pz[c] + cx;
      pv[c] = py * fy / pz[c] + cy;
      use = use && pz[c] > 0.001 && fabs(pu[c]) < __builtin_inf() && fabs(pv[c]) < __builtin_inf();
    }
    if (!use) continue;
    // the triangle's pixel bounding box: part of the coverage test (exact comparisons), which
    // is what makes culling by it exact whatever the edge functions round to
    const double ulo = fmin(fmin(pu[0], pu[1]), pu[2]), uhi = fmax(fmax(pu[0], pu[1]), pu[2]);
    const double vlo = fmin(fmin(pv[0], pv[1]), pv[2]), vhi = fmax(fmax(pv[0], pv[1]), pv[2]);
    int i0, i1, j0, j1;
    sample_range(ulo, uhi, x1, x2, G, i0, i1);
    sample_range(vlo, vhi, y1, y2, G, j0, j1);
    if (i0 > i1 || j0 > j1) continue;
    // e(a, b, p) = (b.u - a.u)(p.v - a.v) - (b.v - a.v)(p.u - a.u)
    const double du0 = pu[2] - pu[1], dv0 = pv[2] - pv[1];   // w0 = e(v1, v2, p)
    const double du1 = pu[0] - pu[2], dv1 = pv[0] - pv[2];   // w1 = e(v2, v0, p)
    const double du2 = pu[1] - pu[0], dv2 = pv[1] - pv[0];   // w2 = e(v0, v1, p)
    for (int j = j0; j <= j1; ++j) {
      const double sv = vs[j];
      if (sv < vlo || sv > vhi) continue;
      const double a0 = du0 * (sv - pv[1]), a1 = du1 * (sv - pv[2]), a2 = du2 * (sv - pv[0]);
      for (int i = i0; i <= i1; ++i) {
        const double su = us[i];
        if (su < ulo || su > uhi) continue;
        const double w0 = a0 - dv0 * (su - pu[1]);
        const double w1 = a1 - dv1 * (su - pu[2]);
        const double w2 = a2 - dv2 * (su - pu[0]);
        const double s = (w0 + w1) + w2;
        const bool cov = (w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0 && s > 0.0) ||
                         (w0 <= 0.0 && w1 <= 0.0 && w2 <= 0.0 && s < 0.0);
        if (!cov) continue;
        const double z = s / ((w0 / pz[0] + w1 / pz[1]) + w2 / pz[2]);
        if (z > 0.0 && z < __builtin_inf())
          atomicMin(&zb[j * G + i], (unsigned long long)__double_as_longlong(z));
      }
    }
  }
  __syncthreads();

  // ---- compare: lanes stride over the samples
  const double thr = a.tau * a.diam[ob];
  int n[5] = {0, 0, 0, 0, 0};
  double rsum = 0.0;
  for (int k = tid; k < P; k += kThreads) {
    const unsigned long long bits = zb[k];
    const bool hit = bits != kNoHit;
    const double z = hit ? __longlong_as_double((long long)bits) : __builtin_inf();
    int cls = 0;
    if (hit) {
      const uint16_t d = p6::depth_at(a, det.f, (int64_t)us[k % G], (int64_t)vs[k / G]);
      if (d == 0) {
        cls = 1;
      } else {
        const double diff = (double)d * a.depth_scale - z;
        cls = fabs(diff) <= thr ? 2 : (diff < -thr ? 3 : 4);
        if (cls == 2) rsum += fabs(diff);
      }
    }
#pragma unroll
    for (int c = 0; c < 5; ++c) n[c] += (cls == c) ? 1 : 0;
    if (a.zbuf_out) a.zbuf_out[(int64_t)b * P + k] = z;
    if (a.cls_out) a.cls_out[(int64_t)b * P + k] = (uint8_t)cls;
  }
#pragma unroll
  for (int c = 0; c < 5; ++c) {
    const int v = p6::wave_sum(n[c]);
    if (lane == 0) red_n[wave][c] = v;
  }
  rsum = p6::wave_sum(rsum);
  if (lane == 0) red_r[wave] = rsum;
  __syncthreads();
  if (tid == 0) {
    int tot[5] = {0, 0, 0, 0, 0};
    double r = 0.0;
    for (int w = 0; w < kWaves; ++w) {   // wave order
      for (int c = 0; c < 5; ++c) tot[c] += red_n[w][c];
      r += red_r[w];
    }
    for (int c = 0; c < 5; ++c) a.counts[5 * b + c] = tot[c];
    const int seen = tot[2] + tot[3] + tot[4], solid = tot[2] + tot[4];
    const double fit = seen > 0 ? (double)tot[2] / (double)seen : 0.0;
    a.fit[b] = fit;
    a.agree[b] = solid > 0 ? (double)tot[2] / (double)solid : 0.0;
    a.resid[b] = tot[2] > 0 ? r / (double)tot[2] : 0.0;
    a.verified[b] = 1;
    if (a.best) a.best[b] = (a.base_flag[b] != 0 && fit >= a.base_fit[b]) ? 1 : 0;
  }
}

}  // namespace

extern "C" int pose6d_pose_verify(const uint16_t* depth, int32_t F, int32_t H, int32_t W, double depth_scale,
                                  const double* K, int32_t K_per_frame, const int32_t* boxes_xyxy,
                                  const int32_t* frame_of, const int64_t* obj, const float* verts, const int32_t* faces,
                                  const int32_t* voff, const int32_t* nverts, const int32_t* toff, const int32_t* ntri,
                                  const double* diam, int32_t n_slots, const float* quat, const double* trans,
                                  int32_t N, int32_t G, double tau, int32_t* counts, double* fit, double* agree,
                                  double* resid, uint8_t* verified, double* zbuf_out, uint8_t* cls_out,
                                  const double* base_fit, const uint8_t* base_flag, uint8_t* best, void* stream) {
  P6_CHECK_ARG(G >= 1 && G <= kMaxG, "pose6d_pose_verify: G must be in [1, 64] (got %d)", (int)G);
  P6_CHECK_ARG(tau > 0.0 && tau < __builtin_inf(), "pose6d_pose_verify: tau must be positive and finite");
  P6_CHECK_ARG(depth_scale > 0.0 && depth_scale < __builtin_inf(),
               "pose6d_pose_verify: depth_scale must be positive and finite");
  P6_CHECK_ARG(N >= 0 && F >= 0 && H >= 0 && W >= 0 && n_slots >= 0,
               "pose6d_pose_verify: bad shape (N, F, H, W and n_slots must not be negative)");
  if (N == 0) return POSE6D_OK;
  P6_CHECK_ARG(depth && K && boxes_xyxy && obj && quat && trans, "pose6d_pose_verify: null input");
  P6_CHECK_ARG(n_slots == 0 || (verts && faces && voff && nverts && toff && ntri && diam),
               "pose6d_pose_verify: null triangle table");
  P6_CHECK_ARG(counts && fit && agree && resid && verified, "pose6d_pose_verify: null output");
  P6_CHECK_ARG(!best || (base_fit && base_flag), "pose6d_pose_verify: best needs base_fit and base_flag");
  const VerifyArgs a = {{depth, F, H, W, depth_scale, K, K_per_frame, boxes_xyxy, frame_of, obj}, verts, faces, voff,
                        nverts, toff, ntri, diam, n_slots, quat, trans, G, tau, counts, fit, agree, resid, verified,
                        zbuf_out, cls_out, base_fit, base_flag, best};
  pose_verify_kernel<<<(unsigned)N, kThreads, 0, p6::stream_of(stream)>>>(a);
  P6_LAUNCH_CHECK();
  return POSE6D_OK;
}
