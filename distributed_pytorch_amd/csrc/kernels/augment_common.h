// What the augmentation kernels (augment.hip, augment_policy.hip) share: the per-slot hash and its
// crop / flip draws, and the scale + normalise arithmetic of one output pixel.
#pragma once
#include "common.h"

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct Norm {
  float m[3], inv_s[3];
};

inline Norm make_norm(const float* mean, const float* std) {
  Norm nm;
  for (int c = 0; c < 3; ++c) {
    nm.m[c] = mean[c];
    nm.inv_s[c] = 1.f / std[c];
  }
  return nm;
}

struct Slot {
  const unsigned char* im;
  int dy, dx, flip;
};

// the hash of batch slot s: every per-sample draw is a function of it
__device__ __forceinline__ unsigned long long slot_hash(unsigned long long seed, unsigned long long salt, int s) {
  return mix64(seed ^ mix64(salt * 0x100000001B3ull + (unsigned long long)s));
}

__device__ __forceinline__ Slot slot_of(const unsigned char* img, const long long* idx, int s, int Hs, int Ws, int pad,
                                        unsigned long long seed, unsigned long long salt) {
  const unsigned long long h = slot_hash(seed, salt, s);
  const int span = 2 * pad + 1;
  return Slot{img + (long)idx[s] * Hs * Ws * 3, (int)(h % span), (int)((h >> 16) % span), (int)((h >> 40) & 1)};
}

// One uint8 RGB pixel scaled and normalised.  Contraction is off so that the value is the separately
// rounded product / difference / product whatever surrounds the call (CutMix and the policy kernel
// are bitwise the plain augmentation).
__device__ __forceinline__ float4 norm_px(unsigned r8, unsigned g8, unsigned b8, const Norm& nm) {
#pragma clang fp contract(off)
  const float r = r8 * (1.f / 255.f), g = g8 * (1.f / 255.f), bl = b8 * (1.f / 255.f);
  return make_float4((r - nm.m[0]) * nm.inv_s[0], (g - nm.m[1]) * nm.inv_s[1], (bl - nm.m[2]) * nm.inv_s[2], 0.f);
}

// augment_kernel's pixel: crop, flip, scale, normalise (out-of-image pixels are 0 before the
// normalisation).
__device__ __forceinline__ float4 slot_px(const Slot& s, int y, int x, int Hs, int Ws, int pad, const Norm& nm) {
  const int xs = s.flip ? (Ws - 1 - x) : x;  // flip applied after the crop
  const int sy = y + s.dy - pad, sx = xs + s.dx - pad;
  unsigned r = 0, g = 0, bl = 0;
  if ((unsigned)sy < (unsigned)Hs && (unsigned)sx < (unsigned)Ws) {
    const unsigned char* q = s.im + ((long)sy * Ws + sx) * 3;
    r = q[0];
    g = q[1];
    bl = q[2];
  }
  return norm_px(r, g, bl, nm);
}
