// The per-element SGD update shared by the flat kernel (sgd.hip) and the segmented LARS / clipping
// kernel (lars.hip): one float4 of the parameter / gradient / momentum arenas, plus the NP operand
// planes of the updated parameters.
//
//   d = (g*gmul + wd*p) * r ; buf = first ? d : momentum*buf + d ; p -= lr*buf
//
// r is the tensor's trust ratio (1 for plain SGD).  The product with r is kept out of FMA
// contraction, so that with r = 1 (x * 1 is exact) every remaining operation is the flat kernel's
// and both kernels give the same bits.
#pragma once
#include <type_traits>

#include "common.h"

// The learning rate of an update kernel, read once per thread before its loop: a kernel argument
// (the constant rate), or one float32 word in device memory (lr_sched.hip: the rate of a schedule,
// written by lr_advance earlier on the step's main stream).
struct LrValue {
  float v;
  __device__ __forceinline__ float get() const { return v; }
};
struct LrWord {
  const float* p;
  __device__ __forceinline__ float get() const { return p[0]; }
};

// f(rate source) for a launcher's (lr, lr_dev) pair: a non-null lr_dev selects the device word
template <class F>
inline void with_rate(float lr, const float* lr_dev, F&& f) {
  if (lr_dev)
    f(LrWord{lr_dev});
  else
    f(LrValue{lr});
}

// f(std::integral_constant<int, NP>) for a launcher's (planes, np) pair: NP in {0, 1, 2, 3}, 0
// without planes
template <class F>
inline void with_planes(const u16* planes, int np, F&& f) {
  if (planes && np == 3)
    f(std::integral_constant<int, 3>{});
  else if (planes && np == 2)
    f(std::integral_constant<int, 2>{});
  else if (planes && np == 1)
    f(std::integral_constant<int, 1>{});
  else
    f(std::integral_constant<int, 0>{});
}

__device__ __forceinline__ float mul_unfused(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// i: float4 index into p / g / buf (and the planes, plane stride ps)
template <int NP>
__device__ __forceinline__ void sgd_update4(float* __restrict__ p, const float* __restrict__ g,
                                            float* __restrict__ buf, long i, float lr, float momentum, float wd,
                                            float gmul, float r, int first, u16* __restrict__ planes, long ps) {
  float4 pv = reinterpret_cast<float4*>(p)[i];
  const float4 gv = reinterpret_cast<const float4*>(g)[i];
  float4 bv;
  float d0 = mul_unfused(gv.x * gmul + wd * pv.x, r);
  float d1 = mul_unfused(gv.y * gmul + wd * pv.y, r);
  float d2 = mul_unfused(gv.z * gmul + wd * pv.z, r);
  float d3 = mul_unfused(gv.w * gmul + wd * pv.w, r);
  if (first) {
    bv = make_float4(d0, d1, d2, d3);
  } else {
    bv = reinterpret_cast<float4*>(buf)[i];
    bv.x = momentum * bv.x + d0;
    bv.y = momentum * bv.y + d1;
    bv.z = momentum * bv.z + d2;
    bv.w = momentum * bv.w + d3;
  }
  pv.x -= lr * bv.x;
  pv.y -= lr * bv.y;
  pv.z -= lr * bv.z;
  pv.w -= lr * bv.w;
  reinterpret_cast<float4*>(buf)[i] = bv;
  reinterpret_cast<float4*>(p)[i] = pv;
  if constexpr (NP > 0) {
    u16 o[4][3];
    constexpr float s = NP == 2 ? H2_SW : 1.f;  // fp16 pairs: the weight planes' scale
    split_val<NP>(pv.x, o[0], s);
    split_val<NP>(pv.y, o[1], s);
    split_val<NP>(pv.z, o[2], s);
    split_val<NP>(pv.w, o[3], s);
#pragma unroll
    for (int q = 0; q < NP; ++q)
      reinterpret_cast<ushort4*>(planes + q * ps)[i] = make_ushort4(o[0][q], o[1][q], o[2][q], o[3][q]);
  }
}
