// Batched ADD / ADD-S evaluation — replaces ADDLoss.eval_metrics / ADDLoss.forward
// (reference models/add_loss.py:101-201).
//
// One launch covers the whole batch (no per-sample host loop, no .item() syncs):
//   add_points_kernel  grid (ceil(maxN/512), B): each block owns 512 predicted
//                      points of one sample (2 per lane: at 4 per lane the 2000-point
//                      meshes left 2 waves per SIMD and the loop latency-bound; at 1,
//                      every gt tile is transformed and read for half the work), streams that sample's
//                      transformed ground-truth mesh through LDS in 2048-point tiles
//                      (broadcast reads, no bank conflicts) and keeps a running
//                      nearest-point minimum per predicted point in registers: 4 gt
//                      points per trip, one scalar branch per trip (round 6).  The
//                      minimum starts from the point's own ground-truth point and a
//                      two-hop walk on the mesh's model-space neighbour table
//                      (add_neighbors_kernel, built once per mesh table), so the sweep
//                      almost never takes its update branch; the first-index tie rule
//                      is order-free, so the bits do not depend on the seeds.
//   add_reduce_kernel  grid B: fixed-order fp64 means (deterministic), 0.1d test.
//   val_append_kernel  one workgroup: the batch's per-sample results become rows of a
//                      device-resident epoch table (the validation pass, pose6d.validate).
//   add_head_loss_kernel / add_head_loss_finish_kernel  ADDLoss.forward and its gradient as a
//                      term of the whole-step trainers' criterion (pose6d_add_head_loss, below).
//
// Bit-exactness contract (pinned by tests/golden/add_loss.npz):
// this file is built with -ffp-contract=off; the only fused ops are the explicit
// fmaf calls that reproduce torch-CPU's mm/norm rounding.  The nearest point is
// tracked on squared distance s; the reference takes the min of sqrtf(s) with the
// FIRST index among equal values, so a new squared minimum keeps the old index
// whenever sqrtf(new) == sqrtf(old) (same sqrt value => the old, earlier j wins).
#include "common.h"

namespace {

// neighbour-table hops of the seed walk (1 = the point's own row only;
// profiles/r06_add_variants.txt)
constexpr int kAddHops = 2;

constexpr int kThreads = 256;
constexpr int kTile = 2048;                   // gt points per LDS tile (32 KiB)

struct Mat3 { float r[9]; };

// add_loss.py:203-215, every op rounded separately
__device__ __forceinline__ Mat3 quat_to_mat(const float* q) {
  const float x = q[0], y = q[1], z = q[2], w = q[3];
  const float x2 = x * x, y2 = y * y, z2 = z * z;
  const float xy = x * y, xz = x * z, yz = y * z;
  const float wx = w * x, wy = w * y, wz = w * z;
  Mat3 m;
  m.r[0] = (1.0f - 2.0f * y2) - 2.0f * z2;
  m.r[1] = 2.0f * xy - 2.0f * wz;
  m.r[2] = 2.0f * xz + 2.0f * wy;
  m.r[3] = 2.0f * xy + 2.0f * wz;
  m.r[4] = (1.0f - 2.0f * x2) - 2.0f * z2;
  m.r[5] = 2.0f * yz - 2.0f * wx;
  m.r[6] = 2.0f * xz - 2.0f * wy;
  m.r[7] = 2.0f * yz + 2.0f * wx;
  m.r[8] = (1.0f - 2.0f * x2) - 2.0f * y2;
  return m;
}

// add_loss.py:178-179: torch.mm(P, R.T) + t with torch-CPU's kernel choice:
// N >= 11 fma chain; 2..10 unfused (p0 r0 + p2 r2) + p1 r1; N == 1 (p1 r1 + p2 r2) + p0 r0.
__device__ __forceinline__ float rowdot(float p0, float p1, float p2, const float* r, int n) {
  const float m0 = p0 * r[0];
  if (n >= 11) return fmaf(p2, r[2], fmaf(p1, r[1], m0));
  const float m1 = p1 * r[1], m2 = p2 * r[2];
  return n >= 2 ? (m0 + m2) + m1 : (m1 + m2) + m0;
}

__device__ __forceinline__ float4 xform(const float* p, const Mat3& R, const float* t, int n) {
  const float p0 = p[0], p1 = p[1], p2 = p[2];
  float4 o;
  o.x = rowdot(p0, p1, p2, R.r + 0, n) + t[0];
  o.y = rowdot(p0, p1, p2, R.r + 3, n) + t[1];
  o.z = rowdot(p0, p1, p2, R.r + 6, n) + t[2];
  o.w = 0.f;
  return o;
}

// torch.norm(d, dim=-1) over 3 = sqrtf(fma(dz,dz, fma(dy,dy, dx*dx)))  (squared part)
__device__ __forceinline__ float sqdist(float ax, float ay, float az, float4 g) {
  const float dx = ax - g.x, dy = ay - g.y, dz = az - g.z;
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// PPT predicted points per lane, U ground-truth points per loop trip: the PPT * U
// squared distances of a trip are independent chains (3 sub, mul, 2 fma each), and
// ONE compare-and-branch per trip asks whether any of them beat its running minimum
// -- after the first few hundred ground-truth points almost never -- instead of a
// branch per (point, gt point).  The rare update replays the trip's candidates.
//   SEED = false: the plain in-order sweep (pose6d_add_eval without a neighbour table);
//          a new squared minimum keeps the old, earlier index iff the roots are equal.
//   SEED = true: the minimum starts from the point's own ground-truth point and a walk
//          on the mesh's neighbour table, so the sweep seldom finds a better candidate;
//          the tie rule is then order-free (below), so the bits are the same.
template <int PPT, int U, bool SEED>
__global__ __launch_bounds__(kThreads) void add_points_kernel(
    const float* __restrict__ pred_rot, const float* __restrict__ pred_trans,
    const float* __restrict__ gt_rot, const float* __restrict__ gt_trans,
    const int64_t* __restrict__ obj_ids, const float* __restrict__ points,
    const int32_t* __restrict__ off, const int32_t* __restrict__ npts, int n_slots, int max_npts,
    float* __restrict__ min_dist, int32_t* __restrict__ argmin, float* __restrict__ pt_add,
    const uint16_t* __restrict__ nbr, int K) {
  constexpr int kPts = kThreads * PPT;
  __shared__ float4 gs[kTile];
  const int b = blockIdx.y;
  const int64_t oid = obj_ids[b];
  if (oid < 0 || oid >= n_slots) return;
  const int n = npts[oid];
  const int base = blockIdx.x * kPts;
  if (n <= 0 || base >= n) return;
  const Mat3 Rp = quat_to_mat(pred_rot + 4 * b);
  const Mat3 Rg = quat_to_mat(gt_rot + 4 * b);
  const float* tp = pred_trans + 3 * b;
  const float* tg = gt_trans + 3 * b;
  const float* P = points + 3 * (int64_t)off[oid];
  const int tid = threadIdx.x;

  // best = smallest squared distance seen, bi = the SMALLEST index among the seen
  // candidates whose sqrtf equals sqrtf(best) (the reference's first-index argmin over
  // the roots); SEED: thr = the largest squared distance that can still matter -- a root
  // equal to sqrtf(best) needs the two within 2^-20 relative (a correctly rounded sqrt
  // of values farther apart differs by >= 8 ulps of the root), so thr = best (1 + 2^-19).
  float qx[PPT], qy[PPT], qz[PPT], best[PPT], thr[PPT];
  int bi[PPT];
#pragma unroll
  for (int i = 0; i < PPT; ++i) {
    const int k = base + tid + kThreads * i;
    best[i] = __builtin_inff();
    bi[i] = 0;
    qx[i] = qy[i] = qz[i] = 0.f;
    if (k < n) {
      const float4 q = xform(P + 3 * k, Rp, tp, n);
      qx[i] = q.x; qy[i] = q.y; qz[i] = q.z;
      const float4 g = xform(P + 3 * k, Rg, tg, n);
      const float skk = sqdist(q.x, q.y, q.z, g);
      pt_add[(int64_t)b * max_npts + k] = sqrtf(skk);  // add_loss.py:182
      // SEED: the point's own ground-truth point (the ADD pair, already at hand) is the
      // first candidate (NaN never becomes a minimum, as in the sweep)
      if (SEED && skk == skk) { best[i] = skk; bi[i] = k; }
    } else {
      best[i] = -__builtin_inff();   // idle lane: nothing beats it (its result is never stored)
    }
    thr[i] = best[i] + best[i] * 0x1p-19f;
  }

  // in order (SEED = false): the common update is a subtract, a multiply and a compare;
  // the two square roots are taken only when the minima are within 2^-20 relative.
  // order-free (SEED): a new squared minimum keeps the old index, or takes j if smaller,
  // iff the roots are equal; a candidate in [best, thr] is a possible root tie and wins
  // only with a smaller index.
  auto update = [&](int i, float s, int j) {
    if (s < best[i]) {
      const float gap = best[i] - s;   // exact when the two are close (Sterbenz)
      if (!(gap <= best[i] * 0x1p-20f) || sqrtf(s) != sqrtf(best[i])) bi[i] = j;
      else if (SEED) bi[i] = min(bi[i], j);
      best[i] = s;
      if (SEED) thr[i] = s + s * 0x1p-19f;
    } else if (SEED && j < bi[i] && s <= thr[i] && sqrtf(s) == sqrtf(best[i])) {
      bi[i] = j;
    }
  };
  // the first tile goes to LDS before the seeds (they read it when the mesh fits one tile)
  for (int jj = tid; jj < min(kTile, n); jj += kThreads) gs[jj] = xform(P + 3 * jj, Rg, tg, n);
  __syncthreads();
  if constexpr (SEED) {
    // the point's neighbours in model space (pose6d_add_neighbors, [point][K] local
    // indices) in a greedy walk: the row of the point's own index, then the row of the
    // best candidate found so far while that keeps moving (the nearest transformed point
    // sits near x = Rg^T (q - tg) in model space, a short walk from k).  Every seed is a
    // genuine candidate (index clamped into the mesh, distance computed as the sweep
    // computes it), so a poor or even wrong table costs time, never bits.
    const uint16_t* nb = nbr + (int64_t)off[oid] * K;
    const bool in_lds = n <= kTile;
    auto cand = [&](int j) { return in_lds ? gs[j] : xform(P + 3 * j, Rg, tg, n); };
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      const int k = base + tid + kThreads * i;
      if (k >= n) continue;
      int cur = k;
      for (int h = 0; h < kAddHops; ++h) {
        const uint16_t* row = nb + (int64_t)cur * K;
        for (int t = 0; t < K; t += 8) {
          const uint4 w = *reinterpret_cast<const uint4*>(row + t);   // 8 indices (K % 8 == 0, 16-B rows)
          const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
          for (int e2 = 0; e2 < 4; ++e2) {   // two candidates at a time (register footprint)
            const int ja = min((int)(ww[e2] & 0xffffu), n - 1), jb = min((int)(ww[e2] >> 16), n - 1);
            const float sa = sqdist(qx[i], qy[i], qz[i], cand(ja)), sb = sqdist(qx[i], qy[i], qz[i], cand(jb));
            update(i, sa, ja);
            update(i, sb, jb);
          }
        }
        if (bi[i] == cur) break;   // nothing nearer around cur
        cur = bi[i];
      }
      // the candidates of the best's own trip that precede it (<= U - 1 of them): the
      // sweep's trip test only asks for strict improvements there (see below)
      for (int j = bi[i] & ~(U - 1); j < bi[i]; ++j) update(i, sqdist(qx[i], qy[i], qz[i], cand(j)), j);
    }
  }
  for (int j0 = 0; j0 < n; j0 += kTile) {
    const int jn = min(kTile, n - j0);
    if (j0 > 0) {
      __syncthreads();
      for (int jj = tid; jj < jn; jj += kThreads) gs[jj] = xform(P + 3 * (j0 + jj), Rg, tg, n);
      __syncthreads();
    }
    int jj = 0;
    for (; jj + U <= jn; jj += U) {
      float s[U][PPT];
      float4 g[U];
#pragma unroll
      for (int u = 0; u < U; ++u) g[u] = gs[jj + u];   // the trip's LDS reads issued together
      // one wave-wide mask of the points that have a candidate beating their minimum:
      // each compare writes a scalar mask (ballot), the masks are OR-ed on the scalar
      // unit and the branch is uniform -- no per-lane bit packing of the flags
      uint64_t hit = 0;
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int i = 0; i < PPT; ++i) s[u][i] = sqdist(qx[i], qy[i], qz[i], g[u]);
      // min over the trip first (v_min3), one compare per point: any s < best <=> min(s) < best
      // (SEED: any s <= thr <=> min(s) <= thr)
      float m[PPT];
#pragma unroll
      for (int i = 0; i < PPT; ++i) {
        m[i] = s[0][i];
#pragma unroll
        for (int u = 1; u < U; ++u) m[i] = __builtin_fminf(m[i], s[u][i]);
        hit |= __ballot(SEED ? m[i] <= thr[i] : m[i] < best[i]);
      }
      if (SEED && __builtin_expect(hit != 0, 0)) {
        // most of these are a point meeting its own current best (m == best <= thr):
        // only a trip wholly before the best's trip can hold a root tie that wins (a
        // smaller index), so elsewhere only a strict improvement counts.  (The best's
        // own trip, up to the best, was replayed when the best was taken -- by the
        // sweep's replay below, or after the seed walk.)
        uint64_t real = 0;
        const int jb = j0 + jj;
#pragma unroll
        for (int i = 0; i < PPT; ++i)
          real |= __ballot(m[i] < best[i] || (jb < (bi[i] & ~(U - 1)) && m[i] <= thr[i]));
        hit = real;
      }
      if (__builtin_expect(hit != 0, 0)) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int i = 0; i < PPT; ++i) update(i, s[u][i], j0 + jj + u);
      }
    }
    for (; jj < jn; ++jj) {
      const float4 g = gs[jj];
#pragma unroll
      for (int i = 0; i < PPT; ++i) update(i, sqdist(qx[i], qy[i], qz[i], g), j0 + jj);
    }
  }
#pragma unroll
  for (int i = 0; i < PPT; ++i) {
    const int k = base + tid + kThreads * i;
    if (k < n) {
      min_dist[(int64_t)b * max_npts + k] = sqrtf(best[i]);  // add_loss.py:187-188
      if (argmin) argmin[(int64_t)b * max_npts + k] = bi[i];
    }
  }
}

// pose6d_add_neighbors: every mesh point's K nearest other points in model space
// (plain fp32 distances -- the table only seeds add_points_kernel's search, it never
// decides a result); one thread per point, a sorted K-list in registers, the mesh read
// as broadcast loads.  A one-time setup per mesh table.
template <int K>
__global__ __launch_bounds__(kThreads) void add_neighbors_kernel(const float* __restrict__ points,
                                                                 const int32_t* __restrict__ off,
                                                                 const int32_t* __restrict__ npts,
                                                                 uint16_t* __restrict__ nbr) {
  const int oid = blockIdx.y;
  const int n = npts[oid];
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= n) return;
  const float* P = points + 3 * (int64_t)off[oid];
  const float px = P[3 * k], py = P[3 * k + 1], pz = P[3 * k + 2];
  float d[K];
  int id[K];
#pragma unroll
  for (int t = 0; t < K; ++t) { d[t] = __builtin_inff(); id[t] = k; }
  for (int j = 0; j < n; ++j) {
    const float dx = P[3 * j] - px, dy = P[3 * j + 1] - py, dz = P[3 * j + 2] - pz;
    float cd = dx * dx + dy * dy + dz * dz;
    if (j == k || !(cd < d[K - 1])) continue;
    int cj = j;
#pragma unroll
    for (int t = 0; t < K; ++t) {
      if (cd < d[t]) {
        const float td = d[t]; const int tj = id[t];
        d[t] = cd; id[t] = cj;
        cd = td; cj = tj;
      }
    }
  }
  uint16_t* row = nbr + ((int64_t)off[oid] + k) * K;
#pragma unroll
  for (int t = 0; t < K; ++t) row[t] = (uint16_t)id[t];
}

__global__ __launch_bounds__(kThreads) void add_reduce_kernel(
    const int64_t* __restrict__ obj_ids, const int32_t* __restrict__ npts, const uint8_t* __restrict__ sym,
    const double* __restrict__ diam, int n_slots, int max_npts, const float* __restrict__ min_dist,
    const float* __restrict__ pt_add, double* __restrict__ add, double* __restrict__ adds,
    int32_t* __restrict__ valid, int32_t* __restrict__ correct) {
  __shared__ double red[2][kThreads / 64];
  const int b = blockIdx.x;
  const int64_t oid = obj_ids[b];
  const int n = (oid >= 0 && oid < n_slots) ? npts[oid] : 0;
  if (n <= 0) {
    if (threadIdx.x == 0) { valid[b] = 0; correct[b] = 0; add[b] = 0.0; adds[b] = 0.0; }
    return;
  }
  double sa = 0.0, ss = 0.0;
  for (int k = threadIdx.x; k < n; k += kThreads) {
    sa += (double)pt_add[(int64_t)b * max_npts + k];
    ss += (double)min_dist[(int64_t)b * max_npts + k];
  }
  sa = p6::wave_sum(sa);
  ss = p6::wave_sum(ss);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][w] = sa; red[1][w] = ss; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double ta = 0.0, ts = 0.0;
    for (int i = 0; i < kThreads / 64; ++i) { ta += red[0][i]; ts += red[1][i]; }
    // the reference's means are fp32 tensors read back with .item() (add_loss.py:183,190)
    const double ma = (double)(float)(ta / n), ms = (double)(float)(ts / n);
    add[b] = ma;
    adds[b] = ms;
    valid[b] = 1;
    const double eff = sym[oid] ? ms : ma;
    correct[b] = eff < 0.1 * diam[oid] ? 1 : 0;  // add_loss.py:176,195
  }
}

// pose6d_val_append: one batch's per-sample results (what add_reduce_kernel wrote) become
// rows of the epoch table at the device-resident cursor state[0], so a replayed graph
// appends without the host knowing the row.  ONE workgroup: every thread reads the cursor
// before the barrier, thread 0 writes it after, and stream order does the rest (no atomics,
// no inter-workgroup protocol).  A batch that does not fit writes no row and counts itself
// in state[1].  The values are copied as they are (doubles; the int32 flags convert exactly).
__global__ __launch_bounds__(kThreads) void val_append_kernel(
    const double* __restrict__ add, const double* __restrict__ adds, const int32_t* __restrict__ valid,
    const int32_t* __restrict__ correct, int B, double* __restrict__ table, int64_t capacity,
    int64_t* __restrict__ state) {
  const int64_t row0 = state[0];
  const bool fits = row0 >= 0 && row0 <= capacity - (int64_t)B;
  if (fits) {
    for (int b = threadIdx.x; b < B; b += kThreads) {
      double* r = table + 4 * (row0 + b);
      r[0] = add[b];
      r[1] = adds[b];
      r[2] = (double)valid[b];
      r[3] = (double)correct[b];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (fits) state[0] = row0 + B;
    else state[1] += 1;
  }
}

// ---------------------------------------------------------------- ADD loss backward
// d loss / d (pred_rot, pred_trans) of ADDLoss.forward (add_loss.py:101-150):
//   loss = (1 / count) sum_i mean_k ||Q_ik - G*_ik||,  Q = P R(q)^T + t,
//   G* = G_k (ADD) or G_argmin(k) (ADD-S: torch.min routes the gradient to the
//   first-index minimum the forward found).  ||.|| backward is 0 at distance 0
//   (torch's norm backward).  One block per sample: fp64 block sums of
//   g = (Q - G*) / d and g P^T, then the chain rule through _quat_to_mat.
__global__ __launch_bounds__(kThreads) void add_loss_bwd_kernel(
    const float* __restrict__ pred_rot, const float* __restrict__ pred_trans, const float* __restrict__ gt_rot,
    const float* __restrict__ gt_trans, const int64_t* __restrict__ obj_ids, int B, const float* __restrict__ points,
    const int32_t* __restrict__ off, const int32_t* __restrict__ npts, const uint8_t* __restrict__ sym, int n_slots,
    int max_npts, const int32_t* __restrict__ argmin, const float* __restrict__ dloss, float* __restrict__ grad_rot,
    float* __restrict__ grad_trans) {
  __shared__ double red[12][kThreads / 64];
  __shared__ int cnt_s;
  const int b = blockIdx.x;
  const int64_t oid = obj_ids[b];
  const int n = (oid >= 0 && oid < n_slots) ? npts[oid] : 0;
  // count of samples that enter the loss (known objects with points)
  int c = 0;
  for (int i = threadIdx.x; i < B; i += kThreads) {
    const int64_t o = obj_ids[i];
    c += (o >= 0 && o < n_slots && npts[o] > 0) ? 1 : 0;
  }
  c = (int)p6::wave_sum((float)c);
  if (threadIdx.x == 0) cnt_s = 0;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) atomicAdd(&cnt_s, c);
  __syncthreads();
  if (n <= 0) {
    if (threadIdx.x < 4) grad_rot[4 * b + threadIdx.x] = 0.f;
    if (threadIdx.x < 3) grad_trans[3 * b + threadIdx.x] = 0.f;
    return;
  }
  const Mat3 Rp = quat_to_mat(pred_rot + 4 * b);
  const Mat3 Rg = quat_to_mat(gt_rot + 4 * b);
  const float* tp = pred_trans + 3 * b;
  const float* tg = gt_trans + 3 * b;
  const float* P = points + 3 * (int64_t)off[oid];
  const bool is_sym = sym[oid] != 0;
  double acc[12];   // gt[3], gR[3][3] (row a = output coordinate, col = point coordinate)
#pragma unroll
  for (int i = 0; i < 12; ++i) acc[i] = 0.0;
  for (int k = threadIdx.x; k < n; k += kThreads) {
    const float4 q = xform(P + 3 * k, Rp, tp, n);
    const int j = is_sym ? argmin[(int64_t)b * max_npts + k] : k;
    const float4 g = xform(P + 3 * j, Rg, tg, n);
    const float dx = q.x - g.x, dy = q.y - g.y, dz = q.z - g.z;
    const float d = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
    if (!(d > 0.f)) continue;
    const double gx = dx / d, gy = dy / d, gz = dz / d;
    const double p0 = P[3 * k], p1 = P[3 * k + 1], p2 = P[3 * k + 2];
    acc[0] += gx; acc[1] += gy; acc[2] += gz;
    acc[3] += gx * p0; acc[4] += gx * p1; acc[5] += gx * p2;
    acc[6] += gy * p0; acc[7] += gy * p1; acc[8] += gy * p2;
    acc[9] += gz * p0; acc[10] += gz * p1; acc[11] += gz * p2;
  }
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    const double v = p6::wave_sum(acc[i]);
    if ((threadIdx.x & 63) == 0) red[i][w] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double t[12];
  const double scale = (double)dloss[0] / ((double)cnt_s * (double)n);
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    double v = 0.0;
    for (int k = 0; k < kThreads / 64; ++k) v += red[i][k];
    t[i] = v * scale;
  }
  grad_trans[3 * b + 0] = (float)t[0];
  grad_trans[3 * b + 1] = (float)t[1];
  grad_trans[3 * b + 2] = (float)t[2];
  const double* G = t + 3;   // dL/dR[a][c], row-major r0..r8
  const double x = pred_rot[4 * b], y = pred_rot[4 * b + 1], z = pred_rot[4 * b + 2], ww = pred_rot[4 * b + 3];
  // d r / d(x, y, z, w) of add_loss.py:203-215
  const double drx[9] = {0, 2 * y, 2 * z, 2 * y, -4 * x, -2 * ww, 2 * z, 2 * ww, -4 * x};
  const double dry[9] = {-4 * y, 2 * x, 2 * ww, 2 * x, 0, 2 * z, -2 * ww, 2 * z, -4 * y};
  const double drz[9] = {-4 * z, -2 * ww, 2 * x, 2 * ww, -4 * z, 2 * y, 2 * x, 2 * y, 0};
  const double drw[9] = {0, -2 * z, 2 * y, 2 * z, 0, -2 * x, -2 * y, 2 * x, 0};
  double gq[4] = {0, 0, 0, 0};
  for (int i = 0; i < 9; ++i) {
    gq[0] += G[i] * drx[i];
    gq[1] += G[i] * dry[i];
    gq[2] += G[i] * drz[i];
    gq[3] += G[i] * drw[i];
  }
  for (int i = 0; i < 4; ++i) grad_rot[4 * b + i] = (float)gq[i];
}

// ---------------------------------------------------------------- ADD loss in the training step
// pose6d_add_head_loss: ADDLoss.forward (add_loss.py:101-150) and its gradient on the head's
// unnormalised quaternion, ADDED to what the step's head + PoseLoss launch wrote.  One
// workgroup per sample: q = normalize(raw) (rownorm_fwd_kernel's arithmetic), Q and G as
// add_points_kernel computes them, the ADD-S nearest-point search only for a symmetric
// sample, fp64 block sums of d, g = (Q - G*) / d and g P^T (add_loss_bwd_kernel's), then the
// chain rule through _quat_to_mat and the normalise.  Every workgroup counts the batch's
// known samples itself, so the gradient waits for no other workgroup; the one cross-sample
// sum (the loss) is add_head_loss_finish_kernel's, a launch of its own.
//
// The search is the in-order sweep of add_points_kernel<.., false> (the same first-index
// rule, so the same index), pruned by a bound: any candidate gives an upper bound S on the
// smallest squared distance, and only candidates with s <= S (1 + 2^-19) can be the minimum
// or share its root (see add_points_kernel), so a trip of four ground-truth points in which
// no lane of the wave has such a candidate is skipped.  The bound starts from the point's
// own ground-truth point and, with a neighbour table, a two-hop walk on it; it only decides
// which trips are skipped, never an index, so the result does not depend on the table.
constexpr float kNormEps = 1e-12f;   // F.normalize default eps (pose_head.hip)
constexpr float kGeoEps = 1e-8f;     // pose_net_rgb_geometric.py:75

__global__ __launch_bounds__(kThreads) void add_head_loss_kernel(
    const float* __restrict__ raw, int norm_mode, const float* __restrict__ trans, const float* __restrict__ gt_rot,
    const float* __restrict__ gt_trans, const int64_t* __restrict__ obj_ids, int B, const float* __restrict__ points,
    const int32_t* __restrict__ off, const int32_t* __restrict__ npts, const uint8_t* __restrict__ sym, int n_slots,
    int max_npts, const uint16_t* __restrict__ nbr, int K, float add_weight, int trans_mode,
    const float* __restrict__ bbox, const float* __restrict__ cam_K, int Kb, float* __restrict__ grad_raw,
    float* __restrict__ grad_trans, double* __restrict__ per, int32_t* __restrict__ nearest) {
  __shared__ float4 gs[kTile];
  __shared__ double red[13][kThreads / 64];
  __shared__ int cnt_s[kThreads / 64];
  const int b = blockIdx.x, tid = threadIdx.x, w = tid >> 6;
  const int64_t oid = obj_ids[b];
  const int n = (oid >= 0 && oid < n_slots) ? npts[oid] : 0;
  if (n <= 0) {
    if (tid == 0) per[b] = 0.0;
    return;
  }
  // count of samples that enter the loss (known objects with points)
  int c = 0;
  for (int i = tid; i < B; i += kThreads) {
    const int64_t o = obj_ids[i];
    c += (o >= 0 && o < n_slots && npts[o] > 0) ? 1 : 0;
  }
  c = p6::wave_sum(c);
  if ((tid & 63) == 0) cnt_s[w] = c;

  // q = normalize(raw): rownorm_fwd_kernel's arithmetic (the bits of the step's `rot`)
  const float* xr = raw + 4 * b;
  const float nrm = sqrtf(fmaf(xr[3], xr[3], fmaf(xr[2], xr[2], fmaf(xr[1], xr[1], fmaf(xr[0], xr[0], 0.f)))));
  const float den = norm_mode == 0 ? fmaxf(nrm, kNormEps) : nrm + kGeoEps;
  const float q[4] = {xr[0] / den, xr[1] / den, xr[2] / den, xr[3] / den};
  const Mat3 Rp = quat_to_mat(q);
  const Mat3 Rg = quat_to_mat(gt_rot + 4 * b);
  const float* tp = trans + 3 * b;
  const float* tg = gt_trans + 3 * b;
  const float* P = points + 3 * (int64_t)off[oid];
  const bool is_sym = sym[oid] != 0;
  const bool in_lds = n <= kTile;   // the whole ground truth is one tile, staged once
  const uint16_t* nb = nbr ? nbr + (int64_t)off[oid] * K : nullptr;
  auto cand = [&](int j) { return in_lds ? gs[j] : xform(P + 3 * j, Rg, tg, n); };
  if (is_sym && in_lds) {
    for (int jj = tid; jj < n; jj += kThreads) gs[jj] = xform(P + 3 * jj, Rg, tg, n);
    __syncthreads();
  }

  double acc[13];   // sum d, gt[3], gR[3][3] (row = output coordinate, col = point coordinate)
#pragma unroll
  for (int i = 0; i < 13; ++i) acc[i] = 0.0;
  for (int k0 = 0; k0 < n; k0 += kThreads) {
    const int k = k0 + tid;
    const bool act = k < n;
    float4 qp = {0.f, 0.f, 0.f, 0.f};
    if (act) qp = xform(P + 3 * k, Rp, tp, n);
    int j = k;
    if (is_sym) {
      // idle lanes: nothing beats -inf, nothing is <= a -inf bound
      float best = act ? __builtin_inff() : -__builtin_inff(), thr = best;
      int bi = 0;
      if (act) {
        float s0 = sqdist(qp.x, qp.y, qp.z, cand(k));
        if (!(s0 == s0)) s0 = __builtin_inff();   // NaN never becomes a minimum
        if (nb) {
          int cur = k, sj = k;
          for (int h = 0; h < kAddHops; ++h) {
            const uint16_t* row = nb + (int64_t)cur * K;
            for (int t = 0; t < K; t += 8) {
              const uint4 wd = *reinterpret_cast<const uint4*>(row + t);   // 8 indices (K % 8 == 0, 16-B rows)
              const uint32_t ww[4] = {wd.x, wd.y, wd.z, wd.w};
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                const int ji = min((int)((ww[e >> 1] >> (16 * (e & 1))) & 0xffffu), n - 1);   // clamped: a genuine candidate
                const float s = sqdist(qp.x, qp.y, qp.z, cand(ji));
                if (s < s0) { s0 = s; sj = ji; }
              }
            }
            if (sj == cur) break;   // nothing nearer around cur
            cur = sj;
          }
        }
        thr = s0 + s0 * 0x1p-19f;
      }
      // in order: a new squared minimum keeps the old, earlier index iff the roots are equal
      auto update = [&](float s, int jn) {
        if (s < best) {
          const float gap = best - s;   // exact when the two are close (Sterbenz)
          if (!(gap <= best * 0x1p-20f) || sqrtf(s) != sqrtf(best)) bi = jn;
          best = s;
          thr = fminf(thr, s + s * 0x1p-19f);
        }
      };
      for (int j0 = 0; j0 < n; j0 += kTile) {
        const int jn = min(kTile, n - j0);
        if (!in_lds) {
          __syncthreads();
          for (int jj = tid; jj < jn; jj += kThreads) gs[jj] = xform(P + 3 * (j0 + jj), Rg, tg, n);
          __syncthreads();
        }
        int jj = 0;
        for (; jj + 4 <= jn; jj += 4) {
          float s[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) s[u] = sqdist(qp.x, qp.y, qp.z, gs[jj + u]);
          const float m = __builtin_fminf(__builtin_fminf(s[0], s[1]), __builtin_fminf(s[2], s[3]));
          if (__ballot(m <= thr) != 0) {
#pragma unroll
            for (int u = 0; u < 4; ++u) update(s[u], j0 + jj + u);
          }
        }
        for (; jj < jn; ++jj) update(sqdist(qp.x, qp.y, qp.z, gs[jj]), j0 + jj);
      }
      j = bi;
    }
    if (!act) continue;
    const float4 g = is_sym ? cand(j) : xform(P + 3 * k, Rg, tg, n);
    if (nearest) nearest[(int64_t)b * max_npts + k] = j;
    const float dx = qp.x - g.x, dy = qp.y - g.y, dz = qp.z - g.z;
    const float d = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
    if (d == 0.f) continue;   // torch's norm backward: 0 at distance 0
    acc[0] += (double)d;
    const double gx = dx / d, gy = dy / d, gz = dz / d;
    const double p0 = P[3 * k], p1 = P[3 * k + 1], p2 = P[3 * k + 2];
    acc[1] += gx; acc[2] += gy; acc[3] += gz;
    acc[4] += gx * p0; acc[5] += gx * p1; acc[6] += gx * p2;
    acc[7] += gy * p0; acc[8] += gy * p1; acc[9] += gy * p2;
    acc[10] += gz * p0; acc[11] += gz * p1; acc[12] += gz * p2;
  }
#pragma unroll
  for (int i = 0; i < 13; ++i) {
    const double v = p6::wave_sum(acc[i]);
    if ((tid & 63) == 0) red[i][w] = v;
  }
  __syncthreads();
  if (tid != 0) return;
  int cnt = 0;
  for (int i = 0; i < kThreads / 64; ++i) cnt += cnt_s[i];
  double t[13];
#pragma unroll
  for (int i = 0; i < 13; ++i) {
    double v = 0.0;
    for (int i2 = 0; i2 < kThreads / 64; ++i2) v += red[i][i2];
    t[i] = v;
  }
  per[b] = t[0] / (double)n;
  const double scale = (double)add_weight / ((double)cnt * (double)n);
  for (int i = 1; i < 13; ++i) t[i] *= scale;
  if (trans_mode == 0) {
    for (int i = 0; i < 3; ++i) grad_trans[3 * b + i] += (float)t[1 + i];
  } else if (trans_mode == 2) {
    // back through the pinhole of the predicted depth (pinhole_z_bwd_kernel's formula)
    const float* kk = Kb ? cam_K + 9 * (int64_t)b : cam_K;
    const double fx = kk[0], cx = kk[2], fy = kk[4], cy = kk[5];
    grad_trans[b] += (float)(t[1] * ((double)bbox[2 * b] - cx) / fx + t[2] * ((double)bbox[2 * b + 1] - cy) / fy + t[3]);
  }
  const double* G = t + 4;   // dL/dR[a][c], row-major r0..r8
  const double x = q[0], y = q[1], z = q[2], qw = q[3];
  // d r / d(x, y, z, w) of add_loss.py:203-215
  const double drx[9] = {0, 2 * y, 2 * z, 2 * y, -4 * x, -2 * qw, 2 * z, 2 * qw, -4 * x};
  const double dry[9] = {-4 * y, 2 * x, 2 * qw, 2 * x, 0, 2 * z, -2 * qw, 2 * z, -4 * y};
  const double drz[9] = {-4 * z, -2 * qw, 2 * x, 2 * qw, -4 * z, 2 * y, 2 * x, 2 * y, 0};
  const double drw[9] = {0, -2 * z, 2 * y, 2 * z, 0, -2 * x, -2 * y, 2 * x, 0};
  double gq[4] = {0, 0, 0, 0};
  for (int i = 0; i < 9; ++i) {
    gq[0] += G[i] * drx[i];
    gq[1] += G[i] * dry[i];
    gq[2] += G[i] * drz[i];
    gq[3] += G[i] * drw[i];
  }
  // back through the normalise (rownorm_bwd_row's cases, in fp64)
  const double xd[4] = {xr[0], xr[1], xr[2], xr[3]};
  const double nd = sqrt(xd[0] * xd[0] + xd[1] * xd[1] + xd[2] * xd[2] + xd[3] * xd[3]);
  const double xg = xd[0] * gq[0] + xd[1] * gq[1] + xd[2] * gq[2] + xd[3] * gq[3];
  double dxr[4];
  if (norm_mode == 0) {
    if (nd > (double)kNormEps) {
      for (int i = 0; i < 4; ++i) dxr[i] = gq[i] / nd - xd[i] * xg / (nd * nd * nd);
    } else {
      for (int i = 0; i < 4; ++i) dxr[i] = gq[i] / (double)kNormEps;   // clamp_min: no grad to the norm
    }
  } else {
    const double dd = nd + (double)kGeoEps;
    const double cc = nd > 0.0 ? xg / (dd * dd * nd) : 0.0;             // norm grad is 0 at 0
    for (int i = 0; i < 4; ++i) dxr[i] = gq[i] / dd - xd[i] * cc;
  }
  for (int i = 0; i < 4; ++i) grad_raw[4 * b + i] += (float)dxr[i];
}

// loss[0] += add_weight * (sum of per[] over the known samples) / count: ONE workgroup, per[]
// summed in a fixed order (per[b] is 0 for an unknown sample), so the bits repeat; nothing
// is added when no sample is known.
__global__ __launch_bounds__(kThreads) void add_head_loss_finish_kernel(
    const int64_t* __restrict__ obj_ids, int B, const int32_t* __restrict__ npts, int n_slots,
    const double* __restrict__ per, float add_weight, float* __restrict__ loss) {
  __shared__ double red[kThreads / 64];
  __shared__ int cnt_s[kThreads / 64];
  const int tid = threadIdx.x;
  int c = 0;
  double s = 0.0;
  for (int i = tid; i < B; i += kThreads) {
    const int64_t o = obj_ids[i];
    c += (o >= 0 && o < n_slots && npts[o] > 0) ? 1 : 0;
    s += per[i];
  }
  c = p6::wave_sum(c);
  s = p6::wave_sum(s);
  if ((tid & 63) == 0) { cnt_s[tid >> 6] = c; red[tid >> 6] = s; }
  __syncthreads();
  if (tid != 0) return;
  int cnt = 0;
  double tot = 0.0;
  for (int i = 0; i < kThreads / 64; ++i) { cnt += cnt_s[i]; tot += red[i]; }
  if (cnt > 0) loss[0] += add_weight * (float)(tot / (double)cnt);
}

}  // namespace

extern "C" int pose6d_add_neighbors(const float* points, const int32_t* off, const int32_t* npts, int32_t n_slots,
                                    int32_t max_npts, int32_t K, uint16_t* nbr, void* stream) {
  P6_CHECK_ARG(n_slots >= 0 && max_npts >= 0 && max_npts <= 65536, "pose6d_add_neighbors: bad table sizes");
  P6_CHECK_ARG(K == 8 || K == 16 || K == 32, "pose6d_add_neighbors: K must be 8, 16 or 32 (got %d)", (int)K);
  if (n_slots == 0 || max_npts == 0) return POSE6D_OK;
  P6_CHECK_ARG(points && off && npts && nbr, "pose6d_add_neighbors: null pointer");
  hipStream_t s = p6::stream_of(stream);
  const dim3 grid(p6::ceil_div(max_npts, kThreads), (unsigned)n_slots);
  if (K == 8) add_neighbors_kernel<8><<<grid, kThreads, 0, s>>>(points, off, npts, nbr);
  else if (K == 16) add_neighbors_kernel<16><<<grid, kThreads, 0, s>>>(points, off, npts, nbr);
  else add_neighbors_kernel<32><<<grid, kThreads, 0, s>>>(points, off, npts, nbr);
  P6_LAUNCH_CHECK();
  return POSE6D_OK;
}

extern "C" int pose6d_add_eval_nbr(const float* pred_rot, const float* pred_trans, const float* gt_rot,
                                   const float* gt_trans, const int64_t* obj_ids, int64_t B,
                                   const float* points, const int32_t* off, const int32_t* npts,
                                   const uint8_t* sym, const double* diam, int32_t n_slots, int32_t max_npts,
                                   const uint16_t* nbr, int32_t K, float* min_dist, int32_t* argmin,
                                   float* pt_add, double* add, double* adds, int32_t* valid, int32_t* correct,
                                   void* stream) {
  P6_CHECK_ARG(B >= 0 && B <= 65535, "pose6d_add_eval: batch %lld out of range", (long long)B);
  P6_CHECK_ARG(n_slots >= 0 && max_npts >= 0, "pose6d_add_eval: bad table sizes");
  P6_CHECK_ARG(!nbr || ((K == 8 || K == 16 || K == 32) && max_npts <= 65536 && ((uintptr_t)nbr & 15) == 0),
               "pose6d_add_eval_nbr: the neighbour table needs K in {8, 16, 32}, <= 65536 points per mesh and "
               "16-byte alignment");
  if (B == 0) return POSE6D_OK;
  P6_CHECK_ARG(min_dist && pt_add && add && adds && valid && correct, "pose6d_add_eval: null output");
  hipStream_t s = p6::stream_of(stream);
  if (max_npts > 0) {
    // 2 predicted points per lane, 4 ground-truth points per trip: A/B on one box
    // (tools/add_ab.py, profiles/r06_add_variants.txt) -- 4 points per lane, 6 or 8 gt
    // points per trip, or 2-4 wave groups of one block splitting the ground truth (twice
    // the waves per SIMD) were all slower
    constexpr int kPPT = 2;
    dim3 grid(p6::ceil_div(max_npts, kThreads * kPPT), (unsigned)B);
    if (nbr)
      add_points_kernel<kPPT, 4, true><<<grid, kThreads, 0, s>>>(pred_rot, pred_trans, gt_rot, gt_trans, obj_ids,
                                                                 points, off, npts, n_slots, max_npts, min_dist,
                                                                 argmin, pt_add, nbr, K);
    else
      add_points_kernel<kPPT, 4, false><<<grid, kThreads, 0, s>>>(pred_rot, pred_trans, gt_rot, gt_trans, obj_ids,
                                                                  points, off, npts, n_slots, max_npts, min_dist,
                                                                  argmin, pt_add, nullptr, 0);
    P6_LAUNCH_CHECK();
  }
  add_reduce_kernel<<<(unsigned)B, kThreads, 0, s>>>(obj_ids, npts, sym, diam, n_slots, max_npts, min_dist, pt_add,
                                                      add, adds, valid, correct);
  P6_LAUNCH_CHECK();
  return POSE6D_OK;
}

extern "C" int pose6d_add_eval(const float* pred_rot, const float* pred_trans, const float* gt_rot,
                               const float* gt_trans, const int64_t* obj_ids, int64_t B,
                               const float* points, const int32_t* off, const int32_t* npts,
                               const uint8_t* sym, const double* diam, int32_t n_slots, int32_t max_npts,
                               float* min_dist, int32_t* argmin, float* pt_add, double* add, double* adds,
                               int32_t* valid, int32_t* correct, void* stream) {
  return pose6d_add_eval_nbr(pred_rot, pred_trans, gt_rot, gt_trans, obj_ids, B, points, off, npts, sym, diam,
                             n_slots, max_npts, nullptr, 0, min_dist, argmin, pt_add, add, adds, valid, correct,
                             stream);
}

extern "C" int pose6d_val_append(const double* add, const double* adds, const int32_t* valid, const int32_t* correct,
                                 int64_t B, double* table, int64_t capacity, int64_t* state, void* stream) {
  P6_CHECK_ARG(B >= 0 && B <= 65535, "pose6d_val_append: batch %lld out of range", (long long)B);
  P6_CHECK_ARG(capacity >= 0, "pose6d_val_append: capacity %lld is negative", (long long)capacity);
  if (B == 0) return POSE6D_OK;
  P6_CHECK_ARG(add && adds && valid && correct && table && state, "pose6d_val_append: null pointer");
  val_append_kernel<<<1, kThreads, 0, p6::stream_of(stream)>>>(add, adds, valid, correct, (int)B, table, capacity,
                                                                state);
  P6_LAUNCH_CHECK();
  return POSE6D_OK;
}

extern "C" int pose6d_add_loss_bwd(const float* pred_rot, const float* pred_trans, const float* gt_rot,
                                   const float* gt_trans, const int64_t* obj_ids, int64_t B, const float* points,
                                   const int32_t* off, const int32_t* npts, const uint8_t* sym, int32_t n_slots,
                                   int32_t max_npts, const int32_t* argmin, const float* dloss, float* grad_rot,
                                   float* grad_trans, void* stream) {
  P6_CHECK_ARG(B >= 0 && B <= 65535, "pose6d_add_loss_bwd: batch %lld out of range", (long long)B);
  P6_CHECK_ARG(argmin && dloss && grad_rot && grad_trans, "pose6d_add_loss_bwd: null argument");
  if (B == 0) return POSE6D_OK;
  add_loss_bwd_kernel<<<(unsigned)B, kThreads, 0, p6::stream_of(stream)>>>(
      pred_rot, pred_trans, gt_rot, gt_trans, obj_ids, (int)B, points, off, npts, sym, n_slots, max_npts, argmin,
      dloss, grad_rot, grad_trans);
  P6_LAUNCH_CHECK();
  return POSE6D_OK;
}

extern "C" int pose6d_add_head_loss(const float* raw, int32_t norm_mode, const float* trans, const float* gt_rot,
                                    const float* gt_trans, const int64_t* obj_ids, int64_t B, const float* points,
                                    const int32_t* off, const int32_t* npts, const uint8_t* sym, int32_t n_slots,
                                    int32_t max_npts, const uint16_t* nbr, int32_t K, float add_weight,
                                    int32_t trans_mode, const float* bbox_center, const float* cam_K,
                                    int32_t K_batched, float* loss, float* grad_raw, float* grad_trans, double* per,
                                    int32_t* nearest, void* stream) {
  P6_CHECK_ARG(B > 0 && B <= 65535, "pose6d_add_head_loss: batch %lld out of range", (long long)B);
  P6_CHECK_ARG(norm_mode == 0 || norm_mode == 1, "pose6d_add_head_loss: bad norm_mode %d", (int)norm_mode);
  P6_CHECK_ARG(trans_mode >= 0 && trans_mode <= 2, "pose6d_add_head_loss: bad trans_mode %d", (int)trans_mode);
  P6_CHECK_ARG(n_slots >= 0 && max_npts >= 0, "pose6d_add_head_loss: bad table sizes");
  P6_CHECK_ARG(!nbr || ((K == 8 || K == 16 || K == 32) && max_npts <= 65536 && ((uintptr_t)nbr & 15) == 0),
               "pose6d_add_head_loss: the neighbour table needs K in {8, 16, 32}, <= 65536 points per mesh and "
               "16-byte alignment");
  P6_CHECK_ARG(raw && trans && gt_rot && gt_trans && obj_ids && loss && grad_raw && per,
               "pose6d_add_head_loss: null argument");
  P6_CHECK_ARG(n_slots == 0 || (points && off && npts && sym), "pose6d_add_head_loss: null mesh table");
  P6_CHECK_ARG(trans_mode == 1 || grad_trans, "pose6d_add_head_loss: trans_mode %d needs grad_trans",
               (int)trans_mode);
  P6_CHECK_ARG(trans_mode != 2 || (bbox_center && cam_K),
               "pose6d_add_head_loss: trans_mode 2 needs bbox_center and the intrinsics");
  hipStream_t s = p6::stream_of(stream);
  add_head_loss_kernel<<<(unsigned)B, kThreads, 0, s>>>(raw, norm_mode, trans, gt_rot, gt_trans, obj_ids, (int)B,
                                                        points, off, npts, sym, n_slots, max_npts, nbr, K, add_weight,
                                                        trans_mode, bbox_center, cam_K, K_batched, grad_raw,
                                                        grad_trans, per, nearest);
  P6_LAUNCH_CHECK();
  add_head_loss_finish_kernel<<<1, kThreads, 0, s>>>(obj_ids, (int)B, npts, n_slots, per, add_weight, loss);
  P6_LAUNCH_CHECK();
  return POSE6D_OK;
}
