// The target of the softmax cross-entropy row kernels (fc_ce.hip, head.hip), once: what a row's loss
// and its dlogits are for a plain class index, a label-smoothed one, and a Mixup / CutMix pair.
// The kernels keep the softmax itself (max, sum of exp, lse: expf in fc_ce.hip, __expf in head.hip)
// and how sum_j z_j is gathered; everything that depends on the target kind is here.
//
//   PLAIN   loss_row  = lse(z) - z_t
//           dlogits_j = (softmax_j - [j == t]) / B
//   SMOOTH  label smoothing eps (0 <= eps < 1; torch's F.cross_entropy(label_smoothing=eps) with mean
//           reduction and class-index targets):
//           loss_row  = lse(z) - (1 - eps) * z_t - (eps / J) * sum_j z_j
//           dlogits_j = (softmax_j - (1 - eps) * [j == t] - eps / J) / B
//   MIX     pair targets: a second class index t2 and a per-row lam, the one-hot target becomes
//           q = lam * onehot(t) + (1 - lam) * onehot(t2); eps rides along and may be 0.  lam is read
//           per row from device memory: a captured graph never bakes it in.
//           loss_row  = lse(z) - (1 - eps) * (lam * z_t + (1 - lam) * z_t2) - (eps / J) * sum_j z_j
//           dlogits_j = (softmax_j - (1 - eps) * (lam * [j == t] + (1 - lam) * [j == t2]) - eps / J) / B
#pragma once
#include <hip/hip_runtime.h>

enum class CeMode { PLAIN, SMOOTH, MIX };

// The mode's kernel arguments, the row kernels' last parameter (PLAIN: empty, the kernel sees no eps).
template <CeMode M>
struct CeArgs;
template <>
struct CeArgs<CeMode::PLAIN> {
  static constexpr CeMode MODE = CeMode::PLAIN;
};
template <>
struct CeArgs<CeMode::SMOOTH> {
  static constexpr CeMode MODE = CeMode::SMOOTH;
  float eps;
};
template <>
struct CeArgs<CeMode::MIX> {
  static constexpr CeMode MODE = CeMode::MIX;
  const long long* target2;
  const float* lam;
  float eps;
};

// One row's target.  SUM_Z: loss() reads sum_z = sum_j z_j (else the kernel need not gather it);
// SECOND: there is a t2, and loss() reads z_t2.  I: the kernel's class-index type.  J: the class
// count as float (the kernel converts it once, for the loss and every dlogit).
//   loss(lse, z_t, z_t2, sum_z, J)    the row's loss (sum_z by reference: head.hip passes the LDS word,
//                                     read where the expression uses it and not at all by PLAIN)
//   dlogit(p, j, J, inv_batch)        dloss / dz_j of the batch-mean loss, p = softmax_j
template <CeMode M, typename I>
struct CeRow;

template <typename I>
struct CeRow<CeMode::PLAIN, I> {
  static constexpr bool SUM_Z = false, SECOND = false;
  I t;
  __device__ __forceinline__ CeRow(CeArgs<CeMode::PLAIN>, const long long* target, int row) : t((I)target[row]) {}
  __device__ __forceinline__ float loss(float lse, float z_t, float, const float&, float) const { return lse - z_t; }
  __device__ __forceinline__ float dlogit(float p, int j, float, float inv) const {
    return (p - (j == t ? 1.f : 0.f)) * inv;
  }
};

template <typename I>
struct CeRow<CeMode::SMOOTH, I> {
  static constexpr bool SUM_Z = true, SECOND = false;
  I t;
  float eps;
  __device__ __forceinline__ CeRow(CeArgs<CeMode::SMOOTH> a, const long long* target, int row)
      : t((I)target[row]), eps(a.eps) {}
  __device__ __forceinline__ float loss(float lse, float z_t, float, const float& sum_z, float J) const {
    return lse - (1.f - eps) * z_t - eps / J * sum_z;
  }
  __device__ __forceinline__ float dlogit(float p, int j, float J, float inv) const {
    return (p - (j == t ? 1.f - eps : 0.f) - eps / J) * inv;
  }
};

template <typename I>
struct CeRow<CeMode::MIX, I> {
  static constexpr bool SUM_Z = true, SECOND = true;
  I t, t2;
  float lam, eps;
  __device__ __forceinline__ CeRow(CeArgs<CeMode::MIX> a, const long long* target, int row)
      : t((I)target[row]), t2((I)a.target2[row]), lam(a.lam[row]), eps(a.eps) {}
  __device__ __forceinline__ float loss(float lse, float z_t, float z_t2, const float& sum_z, float J) const {
    return lse - (1.f - eps) * (lam * z_t + (1.f - lam) * z_t2) - eps / J * sum_z;
  }
  __device__ __forceinline__ float dlogit(float p, int j, float J, float inv) const {
    const float q = (j == t ? lam : 0.f) + (j == t2 ? 1.f - lam : 0.f);
    return (p - (1.f - eps) * q - eps / J) * inv;
  }
};

// Which instance runs for (eps, target2, lam), for both loss entry points: target2 present: MIX (eps
// possibly 0); otherwise eps != 0: SMOOTH; otherwise PLAIN.  Calls run(CeArgs<mode>) and returns 0, or
// -2 without calling it when only one of target2 / lam is given.
template <typename F>
inline int ce_dispatch(float eps, const long long* target2, const float* lam, F&& run) {
  if (!target2 != !lam) return -2;
  if (target2)
    run(CeArgs<CeMode::MIX>{target2, lam, eps});
  else if (eps != 0.f)
    run(CeArgs<CeMode::SMOOTH>{eps});
  else
    run(CeArgs<CeMode::PLAIN>{});
  return 0;
}
