// K13 — the device-resident learning rate of a schedule (schedule.py builds the float32 table on
// the host; the device evaluates no formula).
//
//   lr_advance   one wave, one lane:  pos = from_device ? *step : host_pos
//                                     *lr = table[clamp(pos, 0, T - 1)] ; *step = pos + 1
//
// The update kernels' device-rate instances (sgd_flat_kernel in sgd.hip and sgd_segmented_kernel in
// lars.hip with the rate source LrWord, sgd_update.h) read *lr once per thread.  Eager steps pass
// the host's step count (host_pos), so the host count stays the single truth; a captured step is
// launched with from_device = 1 and advances by itself from replay to replay.
#include "api.h"
#include "common.h"

__global__ __launch_bounds__(64) void lr_advance_kernel(const float* __restrict__ table, long T,
                                                        long* __restrict__ step, float* __restrict__ lr,
                                                        long host_pos, int from_device) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const long pos = from_device ? step[0] : host_pos;
  long k = pos < T - 1 ? pos : T - 1;
  if (k < 0) k = 0;
  lr[0] = table[k];
  step[0] = pos + 1;
}

extern "C" int dpa_lr_advance(const float* table, long T, long* step, float* lr, long host_pos, int from_device,
                              hipStream_t s) {
  if (T < 1) return -1;
  lr_advance_kernel<<<1, 64, 0, s>>>(table, T, step, lr, host_pos, from_device);
  return (int)hipGetLastError();
}
