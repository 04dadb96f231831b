// K7/K8 — classifier head: Linear(Cin -> J) + softmax cross-entropy (mean reduction), forward
// and backward fused.  Replaces addmm / _log_softmax / nll_loss and their backwards
// (model.py:40,45 and main.py:34,99).
//
// fc_ce_rows: one wavefront per sample row: logits (wave reductions over Cin), log-sum-exp,
//   per-row loss, dlogits = (softmax - onehot)/B, and dx = dlogits @ W  — all in registers.
//   The target is a plain class index, a label-smoothed one or a Mixup / CutMix pair (training only;
//   the formulas and the instance each runs are in ce_target.h).  Evaluation (fc_ce_eval) is always
//   the plain cross-entropy.
//   Serves J <= 16, Cin <= 1024, with or without the BnIn prologue (J <= 10, Cin <= 512 on the tight
//   <10, 8> instance); training also needs B * J * 4 <= 48 KB (fc_ce_wgrad's LDS image of dlogits).
// fc_ce_wide_rows: the same outputs for 10 < J <= 1024, Cin <= 1024, any B, wherever the kernel above
//   does not serve, with or without BnIn: 16 rows per block on the fp32-input matrix cores, the
//   logits in the accumulators.  Its weight gradient is dpa_gemm_f32 (gemm_f32.hip), db and the batch
//   loss are fc_ce_wide_db_loss.  Cin % 4 == 0 everywhere; anything else is refused (-2) before a launch.
// fc_ce_wgrad: dW[j][c] = sum_b dlogits[b][j] * x[b][c], db[j] = sum_b dlogits[b][j], and the
//   batch-mean loss (fixed summation order -> bitwise reproducible).
#include "api.h"
#include "ce_target.h"
#include "common.h"

#include <type_traits>

namespace {
// Compile-time bounds: MAXJ classes, MAXCL = Cin / 64 values per lane kept in registers.  The VGG
// head (J = 10, Cin = 512) runs the <10, 8> instance, anything else up to J = 16, Cin = 1024 the
// generic one (every loop over MAXJ / MAXCL is fully unrolled, so tight bounds mean no dead lanes).
constexpr int GEN_J = 16, GEN_CL = 16;

// W [J][Cin] is staged once per block into LDS (one round of independent 16-B loads), the row
// (Cin/64 values per lane) is held in registers, and the J wave reductions are interleaved: the
// kernel pays ~two global-memory latencies instead of a chain of dependent L2 round trips.
//
// Bn: the last conv layer's BatchNorm + ReLU + 2x2 max-pool folded into the row load (VGG on 32x32:
// the pool leaves one pixel, so a feature row is the max over the 4 pixels of z [B][4][Cin] of
// relu(z*scale + shift), the same operations in the same order as bn_apply).  The features are
// also stored to x (the weight-gradient kernel reads them), and the separate bn_apply launch goes.
struct BnIn {
  const float* z;
  const float* scale;
  const float* shift;
};

template <bool TRAIN, int MAXJ, int MAXCL, bool BNIN, CeMode MODE>
__global__ __launch_bounds__(256) void fc_ce_rows_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias,
                                                         const long long* __restrict__ target,
                                                         float* __restrict__ loss_row, float* __restrict__ dlogits,
                                                         float* __restrict__ dx, int* __restrict__ correct_row,
                                                         float* __restrict__ logits_out, int B, int Cin, int J,
                                                         BnIn bn, CeArgs<MODE> ce) {
  using Row = CeRow<MODE, int>;
  static_assert(MODE == CeMode::PLAIN || TRAIN, "SMOOTH and MIX: training instances only");
  extern __shared__ float w_s[];  // [J][Cin]
  // All of the block's W loads are issued together, then the row's loads, and only then is the LDS
  // image written: one memory latency for both instead of one per 4 KB of W plus one for the row
  // (the rolled copy loop cost ~5 dependent round trips on the VGG step's critical path).
  constexpr int WIT = (MAXJ * 64 * MAXCL + 1023) / 1024;  // float4 per thread (256 threads)
  float4 wt[WIT];
#pragma unroll
  for (int u = 0; u < WIT; ++u) {
    const int i = threadIdx.x * 4 + u * 1024;
    wt[u] = i < J * Cin ? *reinterpret_cast<const float4*>(w + i) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const int lane = threadIdx.x & 63;
  const int row = min(blockIdx.x * 4 + (threadIdx.x >> 6), B - 1);  // tail waves load a valid row
  const bool rv = blockIdx.x * 4 + (threadIdx.x >> 6) < B;
  const float* xr = x + (long)row * Cin;
  float xv[MAXCL];
  if constexpr (BNIN) {
    const float* zr = bn.z + (long)row * 4 * Cin;
    float* xo = const_cast<float*>(xr);
#pragma unroll
    for (int k = 0; k < MAXCL; ++k) {
      const int c = lane + 64 * k;
      float v = 0.f;
      if (c < Cin) {
        const float sc = bn.scale[c], sh = bn.shift[c];
        const float v00 = fmaxf(fmaf(zr[c], sc, sh), 0.f), v01 = fmaxf(fmaf(zr[Cin + c], sc, sh), 0.f);
        const float v10 = fmaxf(fmaf(zr[2 * Cin + c], sc, sh), 0.f), v11 = fmaxf(fmaf(zr[3 * Cin + c], sc, sh), 0.f);
        v = fmaxf(fmaxf(v00, v01), fmaxf(v10, v11));
        if (rv) xo[c] = v;
      }
      xv[k] = v;
    }
  } else {
#pragma unroll
    for (int k = 0; k < MAXCL; ++k) {
      const int c = lane + 64 * k;
      xv[k] = c < Cin ? xr[c] : 0.f;
    }
  }
#pragma unroll
  for (int u = 0; u < WIT; ++u) {
    const int i = threadIdx.x * 4 + u * 1024;
    if (i < J * Cin) *reinterpret_cast<float4*>(w_s + i) = wt[u];
  }
  __syncthreads();
  if (!rv) return;
  float logit[MAXJ];
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) {
    float s = 0.f;
    if (j < J) {
#pragma unroll
      for (int k = 0; k < MAXCL; ++k) {
        const int c = lane + 64 * k;
        if (c < Cin) s = fmaf(xv[k], w_s[j * Cin + c], s);
      }
    }
    logit[j] = s;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) logit[j] += __shfl_xor(logit[j], o, 64);
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) logit[j] = j < J ? logit[j] + bias[j] : -INFINITY;
  float mx = logit[0];
  int arg = 0;
#pragma unroll
  for (int j = 1; j < MAXJ; ++j)
    if (j < J && logit[j] > mx) {
      mx = logit[j];
      arg = j;
    }
  float se = 0.f;
#pragma unroll
  for (int j = 0; j < MAXJ; ++j)
    if (j < J) se += expf(logit[j] - mx);
  const float lse = mx + logf(se);
  const Row tr(ce, target, row);
  float lt = 0.f, lt2 = 0.f, sz = 0.f;  // the wave holds all J logits: sz in ascending j (fixed order)
#pragma unroll
  for (int j = 0; j < MAXJ; ++j)
    if (j == tr.t) lt = logit[j];
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) {
    if constexpr (Row::SECOND)
      if (j == tr.t2) lt2 = logit[j];
    if constexpr (Row::SUM_Z)
      if (j < J) sz += logit[j];
  }
  // Once, for the loss and every dlogit.  Keep the conversion here, outside the lane-0 branch: where
  // it stands decides how the compiler contracts the loss into FMAs, and moving it changes the bits.
  const float Jf = (float)J;
  if (lane == 0) {
    loss_row[row] = tr.loss(lse, lt, lt2, sz, Jf);
    if (correct_row) correct_row[row] = (arg == tr.t) ? 1 : 0;
  }
  if (logits_out && lane < J) {
#pragma unroll
    for (int j = 0; j < MAXJ; ++j)
      if (j == lane) logits_out[(long)row * J + j] = logit[j];
  }
  if (TRAIN) {
    const float invB = 1.f / (float)B;
    float dl[MAXJ];
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) dl[j] = j < J ? tr.dlogit(expf(logit[j] - lse), j, Jf, invB) : 0.f;
    if (lane < J) {
#pragma unroll
      for (int j = 0; j < MAXJ; ++j)
        if (j == lane) dlogits[(long)row * J + j] = dl[j];
    }
#pragma unroll
    for (int k = 0; k < MAXCL; ++k) {
      const int c = lane + 64 * k;
      if (c < Cin) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < MAXJ; ++j)
          if (j < J) s = fmaf(dl[j], w_s[j * Cin + c], s);
        dx[(long)row * Cin + c] = s;
      }
    }
  }
}

// grid: cdiv(Cin,8) + 1 blocks of 256 threads = 8 columns x 32 row-groups.  dlogits [B][J] is
// staged in LDS; each thread issues its rows' x loads together, the row-groups are combined
// through LDS in a fixed order (deterministic).  The last block reduces db and the batch-mean loss.
template <int MAXJ>
__global__ __launch_bounds__(256) void fc_ce_wgrad_kernel(const float* __restrict__ x,
                                                          const float* __restrict__ dlogits,
                                                          const float* __restrict__ loss_row, float* __restrict__ dw,
                                                          float* __restrict__ db, float* __restrict__ loss_out,
                                                          float* __restrict__ loss_accum, int B, int Cin, int J) {
  const int ncb = (Cin + 7) / 8;
  const int t = threadIdx.x;
  if ((int)blockIdx.x < ncb) {
    extern __shared__ float dl_s[];  // [B][J]
    __shared__ float red[32][8][MAXJ + 1];
    for (int i = t; i < B * J; i += 256) dl_s[i] = dlogits[i];
    __syncthreads();
    const int cl = t & 7, rg = t >> 3;
    const int c = blockIdx.x * 8 + cl;
    float acc[MAXJ];
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) acc[j] = 0.f;
    if (c < Cin) {
      int b = rg;
      for (; b + 96 < B; b += 128) {
        float xv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) xv[u] = x[(long)(b + 32 * u) * Cin + c];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int j = 0; j < MAXJ; ++j)
            if (j < J) acc[j] = fmaf(dl_s[(b + 32 * u) * J + j], xv[u], acc[j]);
      }
      for (; b < B; b += 32) {
        const float xv = x[(long)b * Cin + c];
#pragma unroll
        for (int j = 0; j < MAXJ; ++j)
          if (j < J) acc[j] = fmaf(dl_s[b * J + j], xv, acc[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) red[rg][cl][j] = acc[j];
    __syncthreads();
    if (t < 8 * J) {
      const int j = t / 8, cc = t % 8;
      float s = 0.f;
      for (int k = 0; k < 32; ++k) s += red[k][cc][j];
      const int col = blockIdx.x * 8 + cc;
      if (col < Cin) dw[(long)j * Cin + col] = s;
    }
  } else {
    __shared__ float sh[256];
    __shared__ float sj[16][17];  // 16 row groups x 16 class lanes (+1 pad), independent of MAXJ
    // db: thread (j = t % 16, g = t / 16) sums rows g, g+16, ...
    const int jj = t % 16, g = t / 16;
    float s = 0.f;
    if (jj < J)
      for (int b = g; b < B; b += 16) s += dlogits[(long)b * J + jj];
    sj[g][jj] = s;
    float l = 0.f;
    for (int b = t; b < B; b += 256) l += loss_row[b];
    sh[t] = l;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (t < o) sh[t] += sh[t + o];
      __syncthreads();
    }
    if (t < J) {
      float d = 0.f;
      for (int k = 0; k < 16; ++k) d += sj[k][t];
      db[t] = d;
    }
    if (t == 0) {
      const float lm = sh[0] / (float)B;
      loss_out[0] = lm;
      if (loss_accum) loss_accum[0] += lm;
    }
  }
}

// ---- wide rows: 10 < J <= 1024 classes on the fp32-input matrix cores ----
// v_mfma_f32_16x16x4_f32 (exact fp32 products, as gemm_f32.hip): lane l supplies A[m = l % 16][k = l / 16]
// and B[k = l / 16][n = l % 16]; accumulator register r of lane l is D[m = 4 * (l / 16) + r][n = l % 16].
//
// One 256-thread block owns 16 batch rows and all J classes (grid = cdiv(B, 16); rows past B are
// clamped on load and never stored).
//   1 logits   the 4 waves split the 16-class tiles (wave w: WT contiguous tiles, at most 16), the
//              logits stay in the accumulators (<= 16 x f32x4).  A: the 16 x Cin x tile, staged through
//              LDS in k-chunks of WK floats by the whole block (with BNIN the chunk is computed from z
//              once, not once per wave); B: W rows from global / L2, one float4 along k per lane and
//              tile, a tile set's loads issued together.  A k-step is 16 deep: lane group g = l / 16
//              holds k = 4g .. 4g+3 of it, MFMA u takes component u of both operands.
//   2 softmax  row max, sum of exp, z_t, z_t2 and sum_j z_j: over the lane's tiles, then over the 16
//              lanes of a row group (__shfl_xor 1, 2, 4, 8), then over the 4 waves through LDS, always in
//              that order.  lse, the loss and every dlogit come from CeRow (ce_target.h).
//   3 dx       dx[16][Cin] = dl[16][J] @ W: the waves split the Cin column tiles (<= 16 each); dl
//              reaches all waves through the LDS buffer in rounds of one wave's class share (<= 256
//              classes); B is W[j][c .. c+15], n-contiguous.
// LDS: one [16][WK + 4] buffer (x chunk, then dl round) and the cross-wave words: under 18 KB.
constexpr int WK = 256, WLD = WK + 4;

template <bool TRAIN, bool BNIN, CeMode MODE>
__global__ __launch_bounds__(256) void fc_ce_wide_rows_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
    const long long* __restrict__ target, float* __restrict__ loss_row, float* __restrict__ dlogits,
    float* __restrict__ dx, int* __restrict__ correct_row, float* __restrict__ logits_out, int B, int Cin, int J,
    BnIn bn, CeArgs<MODE> ce) {
  using Row = CeRow<MODE, int>;
  static_assert(MODE == CeMode::PLAIN || TRAIN, "SMOOTH and MIX: training instances only");
  __shared__ __attribute__((aligned(16))) float s[16][WLD];
  __shared__ float red_mx[4][16];
  __shared__ int red_arg[4][16];
  __shared__ float red_s[4][4][16];  // [se, z_t, z_t2, sum_z][wave][row]
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int ln = lane & 15, lg = lane >> 4;
  const int r0 = blockIdx.x * 16;
  // the wave's class tiles [jt0, jt0 + ntw)
  const int NT = cdiv(J, 16), WT = cdiv(NT, 4);
  const int jt0 = wv * WT, ntw = max(0, min(WT, NT - jt0));

  f32x4 acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- phase 1 ----
  for (int k0 = 0; k0 < Cin; k0 += WK) {
    if (k0) __syncthreads();
    // thread -> (row, float4 column) of the chunk, 4 rounds of 4 rows
    float4 xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int rl = wv + 4 * u, c = k0 + lane * 4;
      const int row = min(r0 + rl, B - 1);
      xv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < Cin) {
        if constexpr (BNIN) {
          const float* zr = bn.z + (long)row * 4 * Cin + c;
          const float4 sc = *reinterpret_cast<const float4*>(bn.scale + c);
          const float4 sh = *reinterpret_cast<const float4*>(bn.shift + c);
          const float4 z0 = *reinterpret_cast<const float4*>(zr), z1 = *reinterpret_cast<const float4*>(zr + Cin);
          const float4 z2 = *reinterpret_cast<const float4*>(zr + 2 * Cin),
                       z3 = *reinterpret_cast<const float4*>(zr + 3 * Cin);
          auto feat = [](float a, float b, float c_, float d, float sc_, float sh_) {
            const float v00 = fmaxf(fmaf(a, sc_, sh_), 0.f), v01 = fmaxf(fmaf(b, sc_, sh_), 0.f);
            const float v10 = fmaxf(fmaf(c_, sc_, sh_), 0.f), v11 = fmaxf(fmaf(d, sc_, sh_), 0.f);
            return fmaxf(fmaxf(v00, v01), fmaxf(v10, v11));
          };
          xv[u] = make_float4(feat(z0.x, z1.x, z2.x, z3.x, sc.x, sh.x), feat(z0.y, z1.y, z2.y, z3.y, sc.y, sh.y),
                              feat(z0.z, z1.z, z2.z, z3.z, sc.z, sh.z), feat(z0.w, z1.w, z2.w, z3.w, sc.w, sh.w));
          if (r0 + rl < B) *reinterpret_cast<float4*>(const_cast<float*>(x) + (long)row * Cin + c) = xv[u];
        } else {
          xv[u] = *reinterpret_cast<const float4*>(x + (long)row * Cin + c);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) *reinterpret_cast<float4*>(&s[wv + 4 * u][lane * 4]) = xv[u];
    __syncthreads();
    const int kend = min(WK, Cin - k0);
    // 16 W loads (one float4 each) are issued together: TW tiles x 16 / TW k-steps, so a wave with
    // few tiles (J = 100: 2) keeps as many loads in flight as one with 16.  A tile's k stay ascending.
    auto steps = [&](auto tw) {
      constexpr int TW = decltype(tw)::value, KS = 16 / TW;
      for (int kk = 0; kk < kend; kk += 16 * KS) {  // kk + 16 * KS <= WK: the LDS reads stay inside
        float4 bv[16], av[KS];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int i = u % TW, kl = kk + 16 * (u / TW) + 4 * lg;  // the lane group's 4 k of the step
          if (i < ntw) {
            const int j = min((jt0 + i) * 16 + ln, J - 1);
            bv[u] = k0 + kl < Cin ? *reinterpret_cast<const float4*>(w + (long)j * Cin + k0 + kl)
                                  : make_float4(0.f, 0.f, 0.f, 0.f);
          }
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)  // (zeros in LDS past Cin)
          av[ks] = *reinterpret_cast<const float4*>(&s[ln][kk + 16 * ks + 4 * lg]);
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int i = u % TW, ks = u / TW;
          if (i < ntw) {
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ks].x, bv[u].x, acc[i], 0, 0, 0);
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ks].y, bv[u].y, acc[i], 0, 0, 0);
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ks].z, bv[u].z, acc[i], 0, 0, 0);
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ks].w, bv[u].w, acc[i], 0, 0, 0);
          }
        }
      }
    };
    if (WT <= 2)
      steps(std::integral_constant<int, 2>{});
    else if (WT <= 4)
      steps(std::integral_constant<int, 4>{});
    else
      steps(std::integral_constant<int, 16>{});
  }

  // ---- phase 2: the lane's rows are r0 + 4 * lg + r, its columns (jt0 + i) * 16 + ln ----
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int j = (jt0 + i) * 16 + ln;
    const bool in = i < ntw && j < J;
    const float bj = in ? bias[j] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[i][r] = in ? acc[i][r] + bj : -INFINITY;
  }
  float mx[4];
  int arg[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    mx[r] = -INFINITY;
    arg[r] = J;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (acc[i][r] > mx[r]) {  // ascending j within the lane: the lowest index of a tie stays
        mx[r] = acc[i][r];
        arg[r] = (jt0 + i) * 16 + ln;
      }
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      const float om = __shfl_xor(mx[r], o, 64);
      if constexpr (!TRAIN) {
        const int oa = __shfl_xor(arg[r], o, 64);
        if (om > mx[r] || (om == mx[r] && oa < arg[r])) arg[r] = oa;
      }
      mx[r] = fmaxf(mx[r], om);
    }
    if (ln == 0) {
      red_mx[wv][4 * lg + r] = mx[r];
      if constexpr (!TRAIN) red_arg[wv][4 * lg + r] = arg[r];
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    mx[r] = red_mx[0][4 * lg + r];
    if constexpr (!TRAIN) arg[r] = red_arg[0][4 * lg + r];
#pragma unroll
    for (int q = 1; q < 4; ++q) {
      const float om = red_mx[q][4 * lg + r];
      if constexpr (!TRAIN) {  // later waves hold higher classes: only a larger value wins
        if (om > mx[r]) arg[r] = red_arg[q][4 * lg + r];
      }
      mx[r] = fmaxf(mx[r], om);
    }
  }
  // the row's target (rows past B: a copy of row B - 1, computed and not stored)
  const Row tr[4] = {Row(ce, target, min(r0 + 4 * lg + 0, B - 1)), Row(ce, target, min(r0 + 4 * lg + 1, B - 1)),
                     Row(ce, target, min(r0 + 4 * lg + 2, B - 1)), Row(ce, target, min(r0 + 4 * lg + 3, B - 1))};
  float se[4], zt[4], zt2[4], sz[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    se[r] = zt[r] = zt2[r] = sz[r] = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int j = (jt0 + i) * 16 + ln;
      if (i < ntw && j < J) {
        const float z = acc[i][r];
        se[r] += expf(z - mx[r]);
        if (j == tr[r].t) zt[r] = z;
        if constexpr (Row::SECOND)
          if (j == tr[r].t2) zt2[r] = z;
        if constexpr (Row::SUM_Z) sz[r] += z;
      }
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      se[r] += __shfl_xor(se[r], o, 64);
      zt[r] += __shfl_xor(zt[r], o, 64);  // one lane of the block holds z_t, the others 0
      if constexpr (Row::SECOND) zt2[r] += __shfl_xor(zt2[r], o, 64);
      if constexpr (Row::SUM_Z) sz[r] += __shfl_xor(sz[r], o, 64);
    }
    if (ln == 0) {
      red_s[0][wv][4 * lg + r] = se[r];
      red_s[1][wv][4 * lg + r] = zt[r];
      if constexpr (Row::SECOND) red_s[2][wv][4 * lg + r] = zt2[r];
      if constexpr (Row::SUM_Z) red_s[3][wv][4 * lg + r] = sz[r];
    }
  }
  __syncthreads();
  const float Jf = (float)J;
  float lse[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int rl = 4 * lg + r;
    se[r] = red_s[0][0][rl] + red_s[0][1][rl] + red_s[0][2][rl] + red_s[0][3][rl];
    zt[r] = red_s[1][0][rl] + red_s[1][1][rl] + red_s[1][2][rl] + red_s[1][3][rl];
    if constexpr (Row::SECOND) zt2[r] = red_s[2][0][rl] + red_s[2][1][rl] + red_s[2][2][rl] + red_s[2][3][rl];
    if constexpr (Row::SUM_Z) sz[r] = red_s[3][0][rl] + red_s[3][1][rl] + red_s[3][2][rl] + red_s[3][3][rl];
    lse[r] = mx[r] + logf(se[r]);
    const int row = r0 + rl;
    if (wv == 0 && ln == 0 && row < B) {
      loss_row[row] = tr[r].loss(lse[r], zt[r], zt2[r], sz[r], Jf);
      if constexpr (!TRAIN)
        if (correct_row) correct_row[row] = (arg[r] == tr[r].t) ? 1 : 0;
    }
  }
  if constexpr (!TRAIN) {
    if (logits_out) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int j = (jt0 + i) * 16 + ln;
        if (i < ntw && j < J) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = r0 + 4 * lg + r;
            if (row < B) logits_out[(long)row * J + j] = acc[i][r];
          }
        }
      }
    }
  } else {
    // dlogits: in place in the accumulators (0 for the classes past J), and to global for the weight gradient
    const float invB = 1.f / (float)B;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int j = (jt0 + i) * 16 + ln;
      const bool in = i < ntw && j < J;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float d = in ? tr[r].dlogit(expf(acc[i][r] - lse[r]), j, Jf, invB) : 0.f;
        acc[i][r] = d;
        const int row = r0 + 4 * lg + r;
        if (in && row < B) dlogits[(long)row * J + j] = d;
      }
    }
    // ---- phase 3: the wave's Cin column tiles [ct0, ct0 + ncw) ----
    const int NC = cdiv(Cin, 16), WC = cdiv(NC, 4);
    const int ct0 = wv * WC, ncw = max(0, min(WC, NC - ct0));
    f32x4 dacc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) dacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < 4 && q * WT < NT; ++q) {
      const int nq = min(WT, NT - q * WT);  // wave q's tiles: classes [q * WT * 16, +nq * 16)
      __syncthreads();
      if (wv == q) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          if (i < nq) {
#pragma unroll
            for (int r = 0; r < 4; ++r) s[4 * lg + r][i * 16 + ln] = acc[i][r];
          }
        }
      }
      __syncthreads();
      const int jq = q * WT * 16;
#pragma unroll 2
      for (int jj = 0; jj < nq * 16; jj += 16) {
        const int jl = jj + 4 * lg;
        const float4 av = *reinterpret_cast<const float4*>(&s[ln][jl]);
        // W rows of this lane group's 4 classes (past J: dl is 0 there, any valid row serves)
        const float* w0 = w + (long)min(jq + jl + 0, J - 1) * Cin;
        const float* w1 = w + (long)min(jq + jl + 1, J - 1) * Cin;
        const float* w2 = w + (long)min(jq + jl + 2, J - 1) * Cin;
        const float* w3 = w + (long)min(jq + jl + 3, J - 1) * Cin;
        float bw[16][4];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          if (i < ncw) {
            const int c = min((ct0 + i) * 16 + ln, Cin - 1);
            bw[i][0] = w0[c];
            bw[i][1] = w1[c];
            bw[i][2] = w2[c];
            bw[i][3] = w3[c];
          }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          if (i < ncw) {
            dacc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bw[i][0], dacc[i], 0, 0, 0);
            dacc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bw[i][1], dacc[i], 0, 0, 0);
            dacc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bw[i][2], dacc[i], 0, 0, 0);
            dacc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bw[i][3], dacc[i], 0, 0, 0);
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = (ct0 + i) * 16 + ln;
      if (i < ncw && c < Cin) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = r0 + 4 * lg + r;
          if (row < B) dx[(long)row * Cin + c] = dacc[i][r];
        }
      }
    }
  }
}

// db[j] = sum_b dlogits[b][j] and the batch-mean loss of the wide path, any B: blocks 0 .. cdiv(J,64)-1
// take 64 classes each (4 row groups of 64 lanes, rows g, g+4, ... in order, combined through LDS in
// group order); the last block reduces loss_row as fc_ce_wgrad_kernel's does.
__global__ __launch_bounds__(256) void fc_ce_wide_db_loss_kernel(const float* __restrict__ dlogits,
                                                                 const float* __restrict__ loss_row,
                                                                 float* __restrict__ db, float* __restrict__ loss_out,
                                                                 float* __restrict__ loss_accum, int B, int J) {
  __shared__ float sh[256];
  const int t = threadIdx.x;
  if ((int)blockIdx.x < cdiv(J, 64)) {
    const int j = blockIdx.x * 64 + (t & 63), g = t >> 6;
    float s = 0.f;
    if (j < J)
      for (int b = g; b < B; b += 4) s += dlogits[(long)b * J + j];
    sh[t] = s;
    __syncthreads();
    if (t < 64 && j < J) db[j] = ((sh[t] + sh[t + 64]) + sh[t + 128]) + sh[t + 192];
  } else {
    float l = 0.f;
    for (int b = t; b < B; b += 256) l += loss_row[b];
    sh[t] = l;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (t < o) sh[t] += sh[t + o];
      __syncthreads();
    }
    if (t == 0) {
      const float lm = sh[0] / (float)B;
      loss_out[0] = lm;
      if (loss_accum) loss_accum[0] += lm;
    }
  }
}

// Eval accumulation: acc[0] += mean loss of this batch, acc[1] += #correct (as float, exact < 2^24)
__global__ __launch_bounds__(256) void eval_accum_kernel(const float* __restrict__ loss_row,
                                                         const int* __restrict__ correct_row, float* __restrict__ acc,
                                                         int B) {
  __shared__ float sl[256];
  __shared__ int sc[256];
  float l = 0.f;
  int c = 0;
  for (int b = threadIdx.x; b < B; b += 256) {
    l += loss_row[b];
    c += correct_row[b];
  }
  sl[threadIdx.x] = l;
  sc[threadIdx.x] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sl[threadIdx.x] += sl[threadIdx.x + o];
      sc[threadIdx.x] += sc[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    acc[0] += sl[0] / (float)B;
    acc[1] += (float)sc[0];
  }
}

// The row kernel's geometry: the BN-in VGG instance, the VGG head's <10, 8>, or the generic one.
template <bool TRAIN, CeMode MODE>
void launch_rows(const float* x, const float* w, const float* b, const long long* target, float* loss_row,
                 float* dlogits, float* dx, int* correct_row, float* logits, int B, int Cin, int J, BnIn bn,
                 CeArgs<MODE> ce, hipStream_t st) {
  const int grid = cdiv(B, 4), lds = J * Cin * 4;
  auto rows = [&](auto mj, auto mcl, auto bnin) {
    fc_ce_rows_kernel<TRAIN, decltype(mj)::value, decltype(mcl)::value, decltype(bnin)::value, MODE>
        <<<grid, 256, lds, st>>>(x, w, b, target, loss_row, dlogits, dx, correct_row, logits, B, Cin, J, bn, ce);
  };
  using J10 = std::integral_constant<int, 10>;
  using CL8 = std::integral_constant<int, 8>;
  if constexpr (TRAIN) {
    if (bn.z) {  // the prologue never changes which geometry runs: the same sums as without it
      if (J <= 10 && Cin <= 512)
        rows(J10{}, CL8{}, std::true_type{});
      else
        rows(std::integral_constant<int, GEN_J>{}, std::integral_constant<int, GEN_CL>{}, std::true_type{});
      return;
    }
  }
  if (J <= 10 && Cin <= 512) {
    rows(J10{}, CL8{}, std::false_type{});
  } else {
    rows(std::integral_constant<int, GEN_J>{}, std::integral_constant<int, GEN_CL>{}, std::false_type{});
  }
}

template <bool TRAIN, CeMode MODE>
void launch_wide_rows(const float* x, const float* w, const float* b, const long long* target, float* loss_row,
                      float* dlogits, float* dx, int* correct_row, float* logits, int B, int Cin, int J, BnIn bn,
                      CeArgs<MODE> ce, hipStream_t st) {
  const int grid = cdiv(B, 16);
  if constexpr (TRAIN) {
    if (bn.z) {
      fc_ce_wide_rows_kernel<true, true, MODE>
          <<<grid, 256, 0, st>>>(x, w, b, target, loss_row, dlogits, dx, correct_row, logits, B, Cin, J, bn, ce);
      return;
    }
  }
  fc_ce_wide_rows_kernel<TRAIN, false, MODE>
      <<<grid, 256, 0, st>>>(x, w, b, target, loss_row, dlogits, dx, correct_row, logits, B, Cin, J, bn, ce);
}

// The wide path's range (the launchers route to it only what the kernels above do not serve).
bool wide_ok(int B, int Cin, int J) { return B >= 1 && J > 10 && J <= 1024 && Cin >= 4 && Cin <= 1024; }

}  // namespace

extern "C" {

// arguments: api.h
int dpa_fc_ce_train(const float* x, const float* w, const float* b, const long long* target, float* loss_row,
                    float* dlogits, float* dx, float* dw, float* db, float* loss_out, float* loss_accum, int B,
                    int Cin, int J, hipStream_t st, const float* bn_z, const float* bn_scale, const float* bn_shift,
                    int parts, float label_smoothing, const long long* target2, const float* lam) {
  if (Cin % 4 || (bn_z && (!bn_scale || !bn_shift))) return -2;
  const bool rows = parts & 1, wg = parts & 2;
  const bool lds_ok = (long)B * J * 4 <= 48 * 1024;
  // bn_z does not enter the choice: a call with the prologue and the same call fed its features run the
  // same kernels and agree bit for bit
  const bool narrow = lds_ok && J <= GEN_J && Cin <= 64 * GEN_CL;
  if (!narrow) {
    if (!wide_ok(B, Cin, J)) return -2;
    const int bad = ce_dispatch(label_smoothing, target2, lam, [&](auto ce) {
      if (rows)
        launch_wide_rows<true>(x, w, b, target, loss_row, dlogits, dx, nullptr, nullptr, B, Cin, J,
                               BnIn{bn_z, bn_scale, bn_shift}, ce, st);
    });
    if (bad) return bad;
    if (wg) {
      // dW [J][Cin] = dlogits^T @ x: A = dlogits m-contiguous, B = x n-contiguous, K = B, one split
      const int rc = dpa_gemm_f32(dlogits, J, 0, x, Cin, 0, dw, J, Cin, B, nullptr, nullptr, 1, st);
      if (rc) return rc;
      fc_ce_wide_db_loss_kernel<<<cdiv(J, 64) + 1, 256, 0, st>>>(dlogits, loss_row, db, loss_out, loss_accum, B, J);
    }
    return (int)hipGetLastError();
  }
  const int bad = ce_dispatch(label_smoothing, target2, lam, [&](auto ce) {
    if (rows)
      launch_rows<true>(x, w, b, target, loss_row, dlogits, dx, nullptr, nullptr, B, Cin, J,
                        BnIn{bn_z, bn_scale, bn_shift}, ce, st);
  });
  if (bad) return bad;
  if (wg) {
    if (J <= 10)
      fc_ce_wgrad_kernel<10><<<cdiv(Cin, 8) + 1, 256, B * J * 4, st>>>(x, dlogits, loss_row, dw, db, loss_out,
                                                                       loss_accum, B, Cin, J);
    else
      fc_ce_wgrad_kernel<GEN_J><<<cdiv(Cin, 8) + 1, 256, B * J * 4, st>>>(x, dlogits, loss_row, dw, db, loss_out,
                                                                          loss_accum, B, Cin, J);
  }
  return (int)hipGetLastError();
}

int dpa_fc_ce_eval(const float* x, const float* w, const float* b, const long long* target, float* loss_row,
                   int* correct_row, float* logits, float* acc, int B, int Cin, int J, hipStream_t st) {
  if (Cin % 4) return -2;
  if (J <= GEN_J && Cin <= 64 * GEN_CL)
    launch_rows<false>(x, w, b, target, loss_row, nullptr, nullptr, correct_row, logits, B, Cin, J,
                       BnIn{nullptr, nullptr, nullptr}, CeArgs<CeMode::PLAIN>{}, st);
  else if (wide_ok(B, Cin, J))
    launch_wide_rows<false>(x, w, b, target, loss_row, nullptr, nullptr, correct_row, logits, B, Cin, J,
                            BnIn{nullptr, nullptr, nullptr}, CeArgs<CeMode::PLAIN>{}, st);
  else
    return -2;
  if (acc) eval_accum_kernel<<<1, 256, 0, st>>>(loss_row, correct_row, acc, B);
  return (int)hipGetLastError();
}

}  // extern "C"
