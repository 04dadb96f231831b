// RandAugment (n_ops ops of torchvision's 14 at one magnitude) + Cutout on the device, one block per
// sample, the whole policy resident in LDS: the sample's uint8 image is read from global memory once,
// every op maps uint8 -> uint8 in integer arithmetic between two LDS images, and the normalised fp32
// NHWC4 result is written once.  The CPU oracle (ops/cpu_ref.py augment_policy) computes the same
// integers, so the two agree bit for bit.
//
// LDS (4-byte words; HW = Hs * Ws <= 4096): two images of HW packed pixels (R | G << 8 | B << 16),
// 768 histogram / LUT words, 16 statistic words.  The raw bytes are staged in the second image
// (3 HW <= 4 HW bytes), the crop + flip of augment_kernel unpacks them into the first, and the ops
// then ping-pong: pointwise ops rewrite the current image in place (every thread owns pixels
// tid, tid + 256, ...), geometric ops and Sharpness gather from it into the other one.  Whole-image
// statistics (grey sum, channel min / max, channel histograms) are wave reductions followed by
// integer LDS atomics: integer sums are order-independent, so the result is deterministic.
//
// Draws (h = the slot hash of augment_common.h; crop and flip use it exactly as augment_kernel):
//   op k:   u = mix64(h ^ (0xA5A5A5A5 + k)), id = u % 14 (or force_op), sign = bit 32 of u
//   cutout: u = mix64(h ^ 0xC0C0C0C0), centre (u % Hs, (u >> 16) % Ws), box of side s around it
// The host-built int32 table (cpu_ref.policy_params) holds what the magnitude fixes.
#include "api.h"
#include "augment_common.h"

namespace {

constexpr int PT = 256;            // threads per block: one histogram bin per thread
constexpr int POLICY_MAX_PX = 4096;
// table layout (cpu_ref.policy_params): geometric ops 1..5, 6 Q16 coefficients for each sign
// (column: A, B, T; row: C, D, T) at ((op - 1) * 2 + sign) * 6; blend ops 6..9, the Q8 factor for
// each sign at 60 + (op - 6) * 2 + sign; 68 the Posterize mask; 69 the Solarize threshold
constexpr int T_BLEND = 60, T_POST = 68, T_SOL = 69;  // 72 words in all

struct Policy {
  int n_ops, cutout, force_op, vec;
};

__device__ __forceinline__ int wave_isum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_imin(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_imax(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_scan(int v) {  // inclusive
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

__device__ __forceinline__ int ch(unsigned px, int c) { return (px >> (8 * c)) & 255; }
__device__ __forceinline__ unsigned pack(int r, int g, int b) { return (unsigned)(r | (g << 8) | (b << 16)); }
__device__ __forceinline__ int grey(unsigned px) {
  return (19595 * ch(px, 0) + 38470 * ch(px, 1) + 7471 * ch(px, 2) + 32768) >> 16;
}
// deg and v in 0..255, f in 0..511: |numerator| < 2^18; >> of a negative int is the floor
__device__ __forceinline__ int blend(int deg, int v, int f) {
  return min(max((deg * (256 - f) + v * f + 128) >> 8, 0), 255);
}

__global__ __launch_bounds__(PT) void augment_policy_kernel(const unsigned char* __restrict__ img,
                                                            const long long* __restrict__ idx,
                                                            const long long* __restrict__ labels,
                                                            float* __restrict__ out, long long* __restrict__ target,
                                                            const int* __restrict__ tab, int Hs, int Ws, int pad,
                                                            unsigned long long seed, unsigned long long salt, Norm nm,
                                                            Policy pol) {
  extern __shared__ __attribute__((aligned(16))) unsigned smem[];
  const int HW = Hs * Ws, tid = threadIdx.x, b = blockIdx.x;
  unsigned* cur = smem;
  unsigned* oth = smem + HW;
  int* hist = reinterpret_cast<int*>(smem + 2 * HW);  // [3][256]
  int* stat = hist + 768;                             // [16]
  const long long src = idx[b];
  const unsigned long long h = slot_hash(seed, salt, b);
  if (tid == 0 && target) target[b] = labels[src];

  // 1. the one global read: the raw bytes into the second image
  {
    const unsigned char* im = img + (long)src * HW * 3;
    unsigned char* raw = reinterpret_cast<unsigned char*>(oth);
    const int nb = HW * 3;
    if (pol.vec) {  // 16-byte lanes (image size and base address are multiples of 16)
      for (int i = tid; i < nb / 16; i += PT)
        reinterpret_cast<uint4*>(raw)[i] = reinterpret_cast<const uint4*>(im)[i];
    } else {
      for (int i = tid; i < nb; i += PT) raw[i] = im[i];
    }
  }
  __syncthreads();
  // 2. augment_kernel's crop and flip (same hash, same bits), out-of-image pixels 0
  {
    const unsigned char* raw = reinterpret_cast<const unsigned char*>(oth);
    const int span = 2 * pad + 1;
    const int dy = (int)(h % span), dx = (int)((h >> 16) % span), flip = (int)((h >> 40) & 1);
    for (int p = tid; p < HW; p += PT) {
      const int y = p / Ws, x = p % Ws;
      const int xs = flip ? (Ws - 1 - x) : x;
      const int sy = y + dy - pad, sx = xs + dx - pad;
      unsigned px = 0;
      if ((unsigned)sy < (unsigned)Hs && (unsigned)sx < (unsigned)Ws) {
        const unsigned char* q = raw + (sy * Ws + sx) * 3;
        px = pack(q[0], q[1], q[2]);
      }
      cur[p] = px;
    }
  }
  __syncthreads();

  // 3. the policy ops; op and sign are uniform over the block
  for (int k = 0; k < pol.n_ops; ++k) {
    const unsigned long long u = mix64(h ^ (0xA5A5A5A5ull + (unsigned long long)k));
    const int op = pol.force_op >= 0 ? pol.force_op : (int)(u % 14);
    const int sg = (int)((u >> 32) & 1);
    if (op >= 1 && op <= 5) {  // ShearX/Y, TranslateX/Y, Rotate: inverse affine map, nearest neighbour
      const int* c = tab + ((op - 1) * 2 + sg) * 6;
      const int c0 = c[0], c1 = c[1], c2 = c[2] + Ws * 65536, c3 = c[3], c4 = c[4], c5 = c[5] + Hs * 65536;
      for (int p = tid; p < HW; p += PT) {
        const int y = p / Ws, x = p % Ws;
        const int X = 2 * x - (Ws - 1), Y = 2 * y - (Hs - 1);
        const int sx = (c0 * X + c1 * Y + c2) >> 17, sy = (c3 * X + c4 * Y + c5) >> 17;
        oth[p] = ((unsigned)sy < (unsigned)Hs && (unsigned)sx < (unsigned)Ws) ? cur[sy * Ws + sx] : 0u;
      }
      unsigned* t = cur;
      cur = oth;
      oth = t;
    } else if (op == 6) {  // Brightness: blend with black
      const int f = tab[T_BLEND + sg];
      for (int p = tid; p < HW; p += PT) {
        const unsigned px = cur[p];
        cur[p] = pack(blend(0, ch(px, 0), f), blend(0, ch(px, 1), f), blend(0, ch(px, 2), f));
      }
    } else if (op == 7) {  // Color: blend with the pixel's grey
      const int f = tab[T_BLEND + 2 + sg];
      for (int p = tid; p < HW; p += PT) {
        const unsigned px = cur[p];
        const int L = grey(px);
        cur[p] = pack(blend(L, ch(px, 0), f), blend(L, ch(px, 1), f), blend(L, ch(px, 2), f));
      }
    } else if (op == 8) {  // Contrast: blend with the image's mean grey
      const int f = tab[T_BLEND + 4 + sg];
      if (tid == 0) stat[0] = 0;
      __syncthreads();
      int s = 0;
      for (int p = tid; p < HW; p += PT) s += grey(cur[p]);
      s = wave_isum(s);
      if ((tid & 63) == 0) atomicAdd(&stat[0], s);
      __syncthreads();
      const int m = (stat[0] + HW / 2) / HW;
      for (int p = tid; p < HW; p += PT) {
        const unsigned px = cur[p];
        cur[p] = pack(blend(m, ch(px, 0), f), blend(m, ch(px, 1), f), blend(m, ch(px, 2), f));
      }
    } else if (op == 9) {  // Sharpness: blend with the 3x3 smooth (1 1 1 / 1 5 1 / 1 1 1) / 13
      const int f = tab[T_BLEND + 6 + sg];
      for (int p = tid; p < HW; p += PT) {
        const int y = p / Ws, x = p % Ws;
        const unsigned px = cur[p];
        unsigned o = px;  // border pixels: the smooth is the pixel itself
        if (y > 0 && y < Hs - 1 && x > 0 && x < Ws - 1) {
          unsigned rb = 0, g = 0;  // R and B in the halves of one word (9 * 255 < 2^16)
#pragma unroll
          for (int j = -1; j <= 1; ++j)
#pragma unroll
            for (int i = -1; i <= 1; ++i) {
              const unsigned q = cur[p + j * Ws + i];
              rb += q & 0x00FF00FFu;
              g += (q >> 8) & 255u;
            }
          const int r0 = ch(px, 0), g0 = ch(px, 1), b0 = ch(px, 2);
          o = pack(blend(((int)(rb & 0xFFFFu) + 4 * r0 + 6) / 13, r0, f), blend(((int)g + 4 * g0 + 6) / 13, g0, f),
                   blend(((int)(rb >> 16) + 4 * b0 + 6) / 13, b0, f));
        }
        oth[p] = o;
      }
      unsigned* t = cur;
      cur = oth;
      oth = t;
    } else if (op == 10) {  // Posterize
      const unsigned m = (unsigned)tab[T_POST] * 0x010101u;
      for (int p = tid; p < HW; p += PT) cur[p] &= m;
    } else if (op == 11) {  // Solarize
      const int th = tab[T_SOL];
      for (int p = tid; p < HW; p += PT) {
        const unsigned px = cur[p];
        const int r = ch(px, 0), g = ch(px, 1), bl = ch(px, 2);
        cur[p] = pack(r >= th ? 255 - r : r, g >= th ? 255 - g : g, bl >= th ? 255 - bl : bl);
      }
    } else if (op == 12) {  // AutoContrast: stretch each channel's [lo, hi] to [0, 255]
      if (tid < 3) {
        stat[tid] = 255;
        stat[3 + tid] = 0;
      }
      __syncthreads();
      int lo[3] = {255, 255, 255}, hi[3] = {0, 0, 0};
      for (int p = tid; p < HW; p += PT) {
        const unsigned px = cur[p];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          lo[c] = min(lo[c], ch(px, c));
          hi[c] = max(hi[c], ch(px, c));
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        lo[c] = wave_imin(lo[c]);
        hi[c] = wave_imax(hi[c]);
        if ((tid & 63) == 0) {
          atomicMin(&stat[c], lo[c]);
          atomicMax(&stat[3 + c], hi[c]);
        }
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        lo[c] = stat[c];
        hi[c] = stat[3 + c] - stat[c];  // the range
      }
      for (int p = tid; p < HW; p += PT) {
        const unsigned px = cur[p];
        int v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          v[c] = ch(px, c);
          if (hi[c] > 0) v[c] = (255 * (v[c] - lo[c]) + hi[c] / 2) / hi[c];
        }
        cur[p] = pack(v[0], v[1], v[2]);
      }
    } else if (op == 13) {  // Equalize: PIL's integer LUT from each channel's histogram
      for (int i = tid; i < 768; i += PT) hist[i] = 0;
      __syncthreads();
      for (int p = tid; p < HW; p += PT) {
        const unsigned px = cur[p];
        atomicAdd(&hist[ch(px, 0)], 1);
        atomicAdd(&hist[256 + ch(px, 1)], 1);
        atomicAdd(&hist[512 + ch(px, 2)], 1);
      }
      __syncthreads();
      // thread i owns bin i of every channel: wave scans, then the totals of the waves before it
      int hv[3], inc[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        hv[c] = hist[c * 256 + tid];
        inc[c] = wave_scan(hv[c]);
        if ((tid & 63) == 63) stat[c * 4 + (tid >> 6)] = inc[c];
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        inc[c] -= hv[c];  // pixels below bin i
        for (int w = 0; w < (tid >> 6); ++w) inc[c] += stat[c * 4 + w];
        // the last non-empty bin is the one bin that completes the image: its thread publishes step
        if (hv[c] > 0 && inc[c] + hv[c] == HW) stat[12 + c] = (HW - hv[c]) / 255;
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < 3; ++c) {  // the LUT takes the histogram's place (each thread read only its own bin)
        const int step = stat[12 + c];
        hist[c * 256 + tid] = step ? min((step / 2 + inc[c]) / max(step, 1), 255) : tid;
      }
      __syncthreads();
      for (int p = tid; p < HW; p += PT) {
        const unsigned px = cur[p];
        cur[p] = pack(hist[ch(px, 0)], hist[256 + ch(px, 1)], hist[512 + ch(px, 2)]);
      }
    }
    __syncthreads();  // the next op (or the output) may read any pixel
  }

  // 4. the one global write: slot_px's scale + normalise, 0.0 (the dataset mean) inside the Cutout box
  int y0 = 0, y1 = 0, x0 = 0, x1 = 0;
  if (pol.cutout > 0) {
    const unsigned long long u = mix64(h ^ 0xC0C0C0C0ull);
    const int ty = (int)(u % Hs) - pol.cutout / 2, tx = (int)((u >> 16) % Ws) - pol.cutout / 2;
    y0 = max(ty, 0);
    y1 = min(ty + pol.cutout, Hs);
    x0 = max(tx, 0);
    x1 = min(tx + pol.cutout, Ws);
  }
  float4* o = reinterpret_cast<float4*>(out) + (long)b * HW;
  for (int p = tid; p < HW; p += PT) {
    const int y = p / Ws, x = p % Ws;
    const unsigned px = cur[p];
    const bool cut = y >= y0 && y < y1 && x >= x0 && x < x1;
    o[p] = cut ? make_float4(0.f, 0.f, 0.f, 0.f) : norm_px(ch(px, 0), ch(px, 1), ch(px, 2), nm);
  }
}

}  // namespace

extern "C" int dpa_augment_policy(const unsigned char* img, const long long* idx, const long long* labels, float* out,
                                  long long* target, const int* table, int B, int Hs, int Ws, int pad,
                                  unsigned long long seed, unsigned long long salt, const float* mean,
                                  const float* std, int n_ops, int cutout, int force_op, hipStream_t st) {
  if (B < 1 || Hs < 1 || Ws < 1 || pad < 0 || (long)Hs * Ws > POLICY_MAX_PX || !table) return -2;
  if (n_ops < 0 || n_ops > 4 || cutout < 0 || cutout > (Hs < Ws ? Hs : Ws) || force_op < -1 || force_op > 13)
    return -2;
  const int HW = Hs * Ws;
  const int vec = (HW * 3) % 16 == 0 && reinterpret_cast<uintptr_t>(img) % 16 == 0;
  const size_t lds = (size_t)(2 * HW + 768 + 16) * sizeof(unsigned);
  augment_policy_kernel<<<B, PT, lds, st>>>(img, idx, labels, out, target, table, Hs, Ws, pad, seed, salt,
                                            make_norm(mean, std), Policy{n_ops, cutout, force_op, vec});
  return (int)hipGetLastError();
}
