// Gradient accumulation: the streaming fold of one micro-step's gradients into the fp32
// accumulator arena (engine.gacc), over the arena or one bucket's slice of it.
//
//   mode 0  store : acc = g          first micro-step of a group
//   mode 1  add   : acc = acc + g    the micro-steps between
//   mode 2  merge : g   = acc + g    the group's last micro-step: g then goes to the collective and
//                                    the update as an ordinary step's gradient does
//
// Plain fp32 additions in the order (((g_0 + g_1) + g_2) + ...), one per element and micro-step, so
// the accumulated gradient is bitwise the torch.add chain of the micro-steps' gradients.  The shape
// is sgd_flat_kernel's (sgd.hip): one float4 per thread and iteration, 256 threads, grid-stride
// under the same block cap; 8 B (store) or 12 B (add, merge) of traffic per element.
#include "api.h"
#include "common.h"

template <int MODE>
__global__ __launch_bounds__(256) void grad_fold_kernel(float* acc, float* g, long n4) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    if constexpr (MODE == 0) {
      reinterpret_cast<float4*>(acc)[i] = gv;
    } else {
      const float4 av = reinterpret_cast<const float4*>(acc)[i];
      const float4 sv = make_float4(av.x + gv.x, av.y + gv.y, av.z + gv.z, av.w + gv.w);
      if constexpr (MODE == 1)
        reinterpret_cast<float4*>(acc)[i] = sv;
      else
        reinterpret_cast<float4*>(g)[i] = sv;
    }
  }
}

// (sgd.hip grid_for: at most 4096 blocks, the loop covers the rest)
static int fold_grid(long n4) {
  long g = (n4 + 255) / 256;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (int)g;
}

extern "C" int dpa_grad_fold(float* acc, float* g, long n, int mode, hipStream_t s) {
  if (n % 4 || n < 0 || mode < 0 || mode > 2) return -1;
  if (n == 0) return 0;
  const long n4 = n / 4;
  const int grid = fold_grid(n4);
  if (mode == 0)
    grad_fold_kernel<0><<<grid, 256, 0, s>>>(acc, g, n4);
  else if (mode == 1)
    grad_fold_kernel<1><<<grid, 256, 0, s>>>(acc, g, n4);
  else
    grad_fold_kernel<2><<<grid, 256, 0, s>>>(acc, g, n4);
  return (int)hipGetLastError();
}
