// K12 — LARS (layer-wise adaptive rate scaling) and global-norm gradient clipping over the flat
// parameter / gradient / momentum arenas: three launches, no atomics, no host round trip.
//
//   (a) sqnorm_partials   one block per chunk:  partials[b] = (sum p^2, sum g^2) in fp64
//   (b) lars_finalize     one block:            per-segment sums, clip coefficient, trust ratios
//   (c) sgd_segmented     one block per chunk:  the update of sgd.hip with a per-segment ratio
//
// A segment is one arena entry with its 64-element padding (zero in p and g); a chunk is a run of
// at most OPT_CHUNK elements inside one segment (every length a multiple of 64).  The host builds
// the block map (segment, start, length per chunk) and the segment table (first chunk, chunks,
// adapted) once per arena; both live on the device as int64 [n, 3].
//
// With gs the sync's gradient scale, P_s = sum p^2 and G_s = sum g^2 of segment s, G = sum_s G_s:
//   c     = max_norm <= 0 ? 1 : min(1, max_norm / (gs sqrt(G) + 1e-6))     (clip_grad_norm_ of gs g)
//   gmul  = gs c
//   r_s   = adapted && |p| > 0 && |g| > 0 ? trust |p| / (|g| + wd |p| + eps) : 1
//           with |p| = sqrt(P_s), |g| = gs c sqrt(G_s)
//   d = (g gmul + wd p) r_s ; buf = first ? d : momentum buf + d ; p -= lr buf
// This is the "learning rate outside the momentum" form of LARS (apex LARC, torchlars): the trust
// ratio scales the gradient that enters the momentum buffer, the learning rate multiplies the
// buffer.  Weight decay is the configured value on every tensor.
//
// Every sum has a fixed order: the element -> thread mapping of (a) depends on the chunk alone,
// never on the grid, and (b) adds a segment's chunks lane-strided in ascending order and then by
// a fixed xor-shuffle tree, so the step is bitwise reproducible.
#include "api.h"
#include "common.h"
#include "sgd_update.h"

constexpr int OPT_CHUNK = 8192;
constexpr int OPT_MAX_SEGMENTS = 2048;  // (b) keeps two doubles per segment in LDS

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// a block-map entry the arena of n elements cannot hold is skipped (the map is device data)
__device__ __forceinline__ bool chunk_ok(long seg, long start, long len, long n, int nseg) {
  return seg >= 0 && seg < nseg && start >= 0 && len > 0 && len <= OPT_CHUNK && (start & 63) == 0 &&
         (len & 63) == 0 && start <= n - len;
}

// (a) squares of fp32 values are exact in fp64, so each thread's sum is the fp64 sum of its
// elements (float4 j, j + 256, ... of the chunk, x y z w in turn)
__global__ __launch_bounds__(256) void sqnorm_partials_kernel(const float* __restrict__ p,
                                                              const float* __restrict__ g,
                                                              const long* __restrict__ bmap, long n, int nseg,
                                                              double* __restrict__ partials) {
  __shared__ double red[4][2];
  const long b = blockIdx.x;
  const long seg = bmap[3 * b], start = bmap[3 * b + 1], len = bmap[3 * b + 2];
  double sp = 0.0, sg = 0.0;
  if (chunk_ok(seg, start, len, n, nseg)) {
    const float4* p4 = reinterpret_cast<const float4*>(p + start);
    const float4* g4 = reinterpret_cast<const float4*>(g + start);
    const int n4 = (int)(len >> 2);
    for (int j = threadIdx.x; j < n4; j += 256) {
      const float4 a = p4[j], c = g4[j];
      const double ax = a.x, ay = a.y, az = a.z, aw = a.w;
      const double cx = c.x, cy = c.y, cz = c.z, cw = c.w;
      sp += ax * ax;
      sp += ay * ay;
      sp += az * az;
      sp += aw * aw;
      sg += cx * cx;
      sg += cy * cy;
      sg += cz * cz;
      sg += cw * cw;
    }
  }
  sp = wave_sum_f64(sp);
  sg = wave_sum_f64(sg);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[w][0] = sp;
    red[w][1] = sg;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double2 out;
    out.x = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
    out.y = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    reinterpret_cast<double2*>(partials)[b] = out;
  }
}

// (b) one block of 16 waves.  Wave w sums segments w, w + 16, ...: lane l adds that segment's chunk
// partials l, l + 64, ... in ascending order, then the xor-shuffle tree.  Every thread then adds
// the G_s in segment order (LDS broadcast reads) and thread t finishes segments t, t + 1024, ...
// table: r_s per segment, then gmul.   stats: sqrt(P_s) [nseg], gs sqrt(G_s) [nseg], gs sqrt(G), c.
__global__ __launch_bounds__(1024) void lars_finalize_kernel(const double* __restrict__ partials, long nblocks,
                                                             const long* __restrict__ segs, int nseg,
                                                             float* __restrict__ table, double* __restrict__ stats,
                                                             double gs, double max_norm, double trust, double wd,
                                                             double eps) {
  __shared__ double sP[OPT_MAX_SEGMENTS], sG[OPT_MAX_SEGMENTS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double2* part2 = reinterpret_cast<const double2*>(partials);
  for (int s = wave; s < nseg; s += 16) {
    const long first = segs[3 * s], cnt = segs[3 * s + 1];
    double sp = 0.0, sg = 0.0;
    if (first >= 0 && cnt >= 0 && first <= nblocks - cnt) {
      for (long k = lane; k < cnt; k += 64) {
        const double2 v = part2[first + k];
        sp += v.x;
        sg += v.y;
      }
    }
    sp = wave_sum_f64(sp);
    sg = wave_sum_f64(sg);
    if (lane == 0) {
      sP[s] = sp;
      sG[s] = sg;
    }
  }
  __syncthreads();
  double G = 0.0;
  for (int s = 0; s < nseg; ++s) G += sG[s];
  const double gnorm = gs * sqrt(G);
  const double c = max_norm > 0.0 ? fmin(1.0, max_norm / (gnorm + 1e-6)) : 1.0;
  const double gmul = gs * c;
  for (int s = threadIdx.x; s < nseg; s += 1024) {
    const double rootG = sqrt(sG[s]);
    const double pn = sqrt(sP[s]), gn = gmul * rootG;
    double r = 1.0;
    if (segs[3 * s + 2] != 0 && pn > 0.0 && gn > 0.0) r = trust * pn / (gn + wd * pn + eps);
    table[s] = (float)r;
    stats[s] = pn;
    stats[nseg + s] = gs * rootG;
  }
  if (threadIdx.x == 0) {
    table[nseg] = (float)gmul;
    stats[2 * nseg] = gnorm;
    stats[2 * nseg + 1] = c;
  }
}

// (c) the update of sgd_flat_kernel<NP, LR> (sgd_update.h) per chunk, with the chunk's segment ratio
template <int NP, class LR>
__global__ __launch_bounds__(256) void sgd_segmented_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                            float* __restrict__ buf, const long* __restrict__ bmap,
                                                            long n, int nseg, const float* __restrict__ table,
                                                            LR lrs, float momentum, float wd, int first,
                                                            u16* __restrict__ planes, long ps) {
  const long b = blockIdx.x;
  const long seg = bmap[3 * b], start = bmap[3 * b + 1], len = bmap[3 * b + 2];
  if (!chunk_ok(seg, start, len, n, nseg)) return;
  const float lr = lrs.get();
  const float r = table[seg], gmul = table[nseg];
  const long i0 = start >> 2, i1 = (start + len) >> 2;
  for (long i = i0 + threadIdx.x; i < i1; i += 256)
    sgd_update4<NP>(p, g, buf, i, lr, momentum, wd, gmul, r, first, planes, ps);
}

extern "C" int dpa_opt_chunk() { return OPT_CHUNK; }
extern "C" int dpa_opt_max_segments() { return OPT_MAX_SEGMENTS; }

extern "C" int dpa_sqnorm_partials(const float* p, const float* g, const long* bmap, long nblocks, long n, int nseg,
                                   double* partials, hipStream_t s) {
  if (nblocks <= 0) return 0;
  sqnorm_partials_kernel<<<(unsigned)nblocks, 256, 0, s>>>(p, g, bmap, n, nseg, partials);
  return (int)hipGetLastError();
}

extern "C" int dpa_lars_finalize(const double* partials, long nblocks, const long* segs, int nseg, float* table,
                                 double* stats, double gs, double max_norm, double trust, double wd, double eps,
                                 hipStream_t s) {
  if (nseg < 1 || nseg > OPT_MAX_SEGMENTS) return -1;
  lars_finalize_kernel<<<1, 1024, 0, s>>>(partials, nblocks, segs, nseg, table, stats, gs, max_norm, trust, wd, eps);
  return (int)hipGetLastError();
}

extern "C" int dpa_sgd_segmented(float* p, const float* g, float* buf, const long* bmap, long nblocks, long n,
                                 int nseg, const float* table, float lr, const float* lr_dev, float momentum,
                                 float wd, int first, u16* planes, long ps, int np, hipStream_t s) {
  if (nblocks <= 0) return 0;
  const unsigned grid = (unsigned)nblocks;
  with_rate(lr, lr_dev, [&](auto lrs) {
    with_planes(planes, np, [&](auto NP) {
      sgd_segmented_kernel<decltype(NP)::value, decltype(lrs)>
          <<<grid, 256, 0, s>>>(p, g, buf, bmap, n, nseg, table, lrs, momentum, wd, first, planes, ps);
    });
  });
  return (int)hipGetLastError();
}

DPA_H2_OVF_ACCESSOR(dpa_h2_ovf_lars)
