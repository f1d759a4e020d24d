// The epoch's device-side bookkeeping (pose6d/fit.py): the plan of a training epoch
// handed to the captured step one row per replay, and the step's loss kept in an epoch
// table until the host reads it once.  Both follow pose6d_val_append's rule
// (add_eval.hip): ONE workgroup, every thread reads the cursor before the barrier, thread
// 0 writes it after, and stream order does the rest -- no atomics, no inter-workgroup
// protocol, plain C++ stores.
//
//   plan_next_kernel    row `cursor` of (idx_plan, bbox_plan, seed_plan) -> the step's inputs
//   loss_append_kernel  the step's fp32 loss -> table[rows], bits unchanged
#include "common.h"

namespace {

constexpr int kThreads = 256;

// state = {cursor, refused}.  cursor in [0, steps): copy the row, cursor += 1; otherwise
// (the plan is exhausted, or the cursor was set negative) write nothing, refused += 1.
__global__ __launch_bounds__(kThreads) void plan_next_kernel(
    const int64_t* __restrict__ idx_plan, const int32_t* __restrict__ bbox_plan,
    const uint64_t* __restrict__ seed_plan, int64_t steps, int B, int64_t* __restrict__ state,
    int64_t* __restrict__ sample_idx, int32_t* __restrict__ bbox_aug, uint64_t* __restrict__ seed_out) {
  const int64_t row = state[0];
  const bool ok = row >= 0 && row < steps;
  if (ok) {
    for (int b = threadIdx.x; b < B; b += kThreads) sample_idx[b] = idx_plan[row * B + b];
    if (bbox_plan)
      for (int i = threadIdx.x; i < 4 * B; i += kThreads) bbox_aug[i] = bbox_plan[row * 4 * B + i];
    if (seed_plan && threadIdx.x == 0) seed_out[0] = seed_plan[row];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (ok) state[0] = row + 1;
    else state[1] += 1;
  }
}

// state = {rows, refused, non-finite}.  The value travels as its 32 bits (a NaN's payload
// and the sign of zero survive); non-finite = exponent field all ones.
__global__ void loss_append_kernel(const uint32_t* __restrict__ loss, uint32_t* __restrict__ table, int64_t capacity,
                                   int64_t* __restrict__ state) {
  if (threadIdx.x != 0) return;
  const int64_t row = state[0];
  if (row < 0 || row >= capacity) {
    state[1] += 1;
    return;
  }
  const uint32_t bits = loss[0];
  table[row] = bits;
  state[0] = row + 1;
  if ((bits & 0x7F800000u) == 0x7F800000u) state[2] += 1;
}

}  // namespace

extern "C" int pose6d_plan_next(const int64_t* idx_plan, const int32_t* bbox_plan, const uint64_t* seed_plan,
                                int64_t steps, int64_t B, int64_t* state, int64_t* sample_idx, int32_t* bbox_aug,
                                uint64_t* seed_out, void* stream) {
  P6_CHECK_ARG(B >= 0 && B <= 65535, "pose6d_plan_next: batch %lld out of range", (long long)B);
  P6_CHECK_ARG(steps >= 0, "pose6d_plan_next: steps %lld is negative", (long long)steps);
  P6_CHECK_ARG((bbox_plan != nullptr) == (bbox_aug != nullptr),
               "pose6d_plan_next: bbox_aug is required exactly when bbox_plan is given");
  P6_CHECK_ARG((seed_plan != nullptr) == (seed_out != nullptr),
               "pose6d_plan_next: seed_out is required exactly when seed_plan is given");
  if (B == 0) return POSE6D_OK;
  P6_CHECK_ARG(idx_plan && state && sample_idx, "pose6d_plan_next: null pointer");
  plan_next_kernel<<<1, kThreads, 0, p6::stream_of(stream)>>>(idx_plan, bbox_plan, seed_plan, steps, (int)B, state,
                                                               sample_idx, bbox_aug, seed_out);
  P6_LAUNCH_CHECK();
  return POSE6D_OK;
}

extern "C" int pose6d_loss_append(const float* loss, float* table, int64_t capacity, int64_t* state, void* stream) {
  P6_CHECK_ARG(capacity >= 0, "pose6d_loss_append: capacity %lld is negative", (long long)capacity);
  P6_CHECK_ARG(loss && state && (table || capacity == 0), "pose6d_loss_append: null pointer");
  loss_append_kernel<<<1, 64, 0, p6::stream_of(stream)>>>(reinterpret_cast<const uint32_t*>(loss),
                                                          reinterpret_cast<uint32_t*>(table), capacity, state);
  P6_LAUNCH_CHECK();
  return POSE6D_OK;
}
