// K10 — on-device CIFAR augmentation + normalisation.  Replaces the reference's DataLoader
// worker pipeline RandomCrop(32, padding=4) -> RandomHorizontalFlip -> ToTensor -> Normalize
// (/root/reference/main.py:71-82) for a device-resident uint8 dataset, so no host->device copy
// and no worker processes sit in the training loop.
//
// images: uint8 [Ntotal][Hs][Ws][3] (HWC), idx: int64 [B] dataset indices for this batch.
// out: fp32 NHWC [B][Hs][Ws][4] (channel 3 zero: the first conv is run with C padded to 4).
// Per-sample crop offsets / flip come from a counter-based hash of (seed, sample index, salt),
// so the stream is reproducible and independent of launch geometry.
#include "api.h"
#include "common.h"

namespace {

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct Norm {
  float m[3], inv_s[3];
};

__global__ __launch_bounds__(256) void augment_kernel(const unsigned char* __restrict__ img,
                                                      const long long* __restrict__ idx,
                                                      const long long* __restrict__ labels,
                                                      float* __restrict__ out, long long* __restrict__ target, int Hs,
                                                      int Ws, int pad, int train, unsigned long long seed,
                                                      unsigned long long salt, Norm nm) {
  const int b = blockIdx.x;
  const long long src = idx[b];
  int dy = pad, dx = pad, flip = 0;
  if (train) {
    const unsigned long long h = mix64(seed ^ mix64(salt * 0x100000001B3ull + (unsigned long long)b));
    const int span = 2 * pad + 1;
    dy = (int)(h % span);
    dx = (int)((h >> 16) % span);
    flip = (int)((h >> 40) & 1);
  }
  if (threadIdx.x == 0 && target) target[b] = labels[src];
  const unsigned char* im = img + (long)src * Hs * Ws * 3;
  float4* o = reinterpret_cast<float4*>(out) + (long)b * Hs * Ws;
  for (int p = threadIdx.x; p < Hs * Ws; p += blockDim.x) {
    const int y = p / Ws, x = p % Ws;
    const int xs = flip ? (Ws - 1 - x) : x;  // flip applied after the crop
    const int sy = y + dy - pad, sx = xs + dx - pad;
    float r = 0.f, g = 0.f, bl = 0.f;
    if ((unsigned)sy < (unsigned)Hs && (unsigned)sx < (unsigned)Ws) {
      const unsigned char* q = im + ((long)sy * Ws + sx) * 3;
      r = q[0] * (1.f / 255.f);
      g = q[1] * (1.f / 255.f);
      bl = q[2] * (1.f / 255.f);
    }
    o[p] = make_float4((r - nm.m[0]) * nm.inv_s[0], (g - nm.m[1]) * nm.inv_s[1], (bl - nm.m[2]) * nm.inv_s[2], 0.f);
  }
}

// Mixup / CutMix: slot b of a batch of B is mixed with slot B-1-b (timm's x.flip(0) pairing; the
// middle slot of an odd batch pairs with itself), one lambda and one box per batch.  aug(s) below
// is exactly what augment_kernel writes for slot s (training mode): the partner's crop offsets and
// flip are recomputed from the hash of slot B-1-b and its pixels read from image idx[B-1-b], so there
// is no second buffer and no second pass.
//   mode 0 (Mixup):  out[b] = lam * aug(b) + (1 - lam) * aug(B-1-b)      (two source pixels per pixel)
//   mode 1 (CutMix): out[b][y][x] = aug(B-1-b)[y][x] inside [y0,y1) x [x0,x1), else aug(b)[y][x]
//                    (a select: one source pixel per pixel, bitwise the plain values)
// target[b] = labels[idx[b]], target2[b] = labels[idx[B-1-b]], lam_out[b] = lam (the loss heads read
// lambda per row from device memory).
struct Mix {
  int mode;
  float lam;
  int y0, y1, x0, x1;
};

struct Slot {
  const unsigned char* im;
  int dy, dx, flip;
};

__device__ __forceinline__ Slot slot_of(const unsigned char* img, const long long* idx, int s, int Hs, int Ws, int pad,
                                        unsigned long long seed, unsigned long long salt) {
  const unsigned long long h = mix64(seed ^ mix64(salt * 0x100000001B3ull + (unsigned long long)s));
  const int span = 2 * pad + 1;
  return Slot{img + (long)idx[s] * Hs * Ws * 3, (int)(h % span), (int)((h >> 16) % span), (int)((h >> 40) & 1)};
}

// augment_kernel's pixel: crop, flip, scale, normalise.  Contraction is off so that the value is the
// separately rounded product / difference / product whatever surrounds the call (CutMix is bitwise).
__device__ __forceinline__ float4 slot_px(const Slot& s, int y, int x, int Hs, int Ws, int pad, const Norm& nm) {
#pragma clang fp contract(off)
  const int xs = s.flip ? (Ws - 1 - x) : x;  // flip applied after the crop
  const int sy = y + s.dy - pad, sx = xs + s.dx - pad;
  float r = 0.f, g = 0.f, bl = 0.f;
  if ((unsigned)sy < (unsigned)Hs && (unsigned)sx < (unsigned)Ws) {
    const unsigned char* q = s.im + ((long)sy * Ws + sx) * 3;
    r = q[0] * (1.f / 255.f);
    g = q[1] * (1.f / 255.f);
    bl = q[2] * (1.f / 255.f);
  }
  return make_float4((r - nm.m[0]) * nm.inv_s[0], (g - nm.m[1]) * nm.inv_s[1], (bl - nm.m[2]) * nm.inv_s[2], 0.f);
}

__global__ __launch_bounds__(256) void augment_mix_kernel(const unsigned char* __restrict__ img,
                                                          const long long* __restrict__ idx,
                                                          const long long* __restrict__ labels,
                                                          float* __restrict__ out, long long* __restrict__ target,
                                                          long long* __restrict__ target2,
                                                          float* __restrict__ lam_out, int Hs, int Ws, int pad,
                                                          unsigned long long seed, unsigned long long salt, Norm nm,
                                                          Mix mx) {
  const int b = blockIdx.x, pb = gridDim.x - 1 - b;
  const Slot own = slot_of(img, idx, b, Hs, Ws, pad, seed, salt);
  const Slot par = slot_of(img, idx, pb, Hs, Ws, pad, seed, salt);
  if (threadIdx.x == 0) {
    target[b] = labels[idx[b]];
    target2[b] = labels[idx[pb]];
    lam_out[b] = mx.lam;
  }
  float4* o = reinterpret_cast<float4*>(out) + (long)b * Hs * Ws;
  for (int p = threadIdx.x; p < Hs * Ws; p += blockDim.x) {
    const int y = p / Ws, x = p % Ws;
    if (mx.mode == 1) {
      const bool in = y >= mx.y0 && y < mx.y1 && x >= mx.x0 && x < mx.x1;
      o[p] = slot_px(in ? par : own, y, x, Hs, Ws, pad, nm);
    } else {
      const float4 a = slot_px(own, y, x, Hs, Ws, pad, nm), c = slot_px(par, y, x, Hs, Ws, pad, nm);
      const float l = mx.lam, k = 1.f - mx.lam;
      o[p] = make_float4(l * a.x + k * c.x, l * a.y + k * c.y, l * a.z + k * c.z, 0.f);
    }
  }
}

}  // namespace

extern "C" int dpa_augment_mix(const unsigned char* img, const long long* idx, const long long* labels, float* out,
                               long long* target, long long* target2, float* lam_out, int mode, float lam, int y0,
                               int y1, int x0, int x1, int B, int Hs, int Ws, int pad, unsigned long long seed,
                               unsigned long long salt, const float* mean, const float* std, hipStream_t st) {
  if (mode != 0 && mode != 1) return -2;
  if (!(lam >= 0.f && lam <= 1.f) || !target || !target2 || !lam_out) return -2;
  if (mode == 1 && (y0 < 0 || y1 > Hs || x0 < 0 || x1 > Ws)) return -2;
  Norm nm;
  for (int c = 0; c < 3; ++c) {
    nm.m[c] = mean[c];
    nm.inv_s[c] = 1.f / std[c];
  }
  augment_mix_kernel<<<B, 256, 0, st>>>(img, idx, labels, out, target, target2, lam_out, Hs, Ws, pad, seed, salt, nm,
                                        Mix{mode, lam, y0, y1, x0, x1});
  return (int)hipGetLastError();
}

extern "C" int dpa_augment(const unsigned char* img, const long long* idx, const long long* labels, float* out,
                           long long* target, int B, int Hs, int Ws, int pad, int train, unsigned long long seed,
                           unsigned long long salt, const float* mean, const float* std, hipStream_t st) {
  Norm nm;
  for (int c = 0; c < 3; ++c) {
    nm.m[c] = mean[c];
    nm.inv_s[c] = 1.f / std[c];
  }
  augment_kernel<<<B, 256, 0, st>>>(img, idx, labels, out, target, Hs, Ws, pad, train, seed, salt, nm);
  return (int)hipGetLastError();
}
