// The optimizer's entry points (sgd.hip, lars.hip, lr_sched.hip, grad_fold.hip), declared once: the kernel files
// that define them and the bindings that call them include this header, so the compiler checks
// every definition against its use.
#pragma once
#include <hip/hip_runtime_api.h>

extern "C" {
// lr_dev != nullptr: the rate is read from that float32 word on the device and lr is ignored
// planes: np operand planes of the same arena slice (plane stride ps), or nullptr / np = 0
int dpa_sgd_flat(float* p, const float* g, float* buf, long n, float lr, const float* lr_dev, float momentum,
                 float wd, float gscale, int first, unsigned short* planes, long ps, int np, hipStream_t s);
int dpa_sgd_segmented(float* p, const float* g, float* buf, const long* bmap, long nblocks, long n, int nseg,
                      const float* table, float lr, const float* lr_dev, float momentum, float wd, int first,
                      unsigned short* planes, long ps, int np, hipStream_t s);
int dpa_sqnorm_partials(const float* p, const float* g, const long* bmap, long nblocks, long n, int nseg,
                        double* partials, hipStream_t s);
int dpa_lars_finalize(const double* partials, long nblocks, const long* segs, int nseg, float* table, double* stats,
                      double gs, double max_norm, double trust, double wd, double eps, hipStream_t s);
int dpa_lr_advance(const float* table, long T, long* step, float* lr, long host_pos, int from_device, hipStream_t s);
// gradient accumulation (grad_fold.hip) over n elements (n % 4 == 0, else -1):
// mode 0 store: acc = g   1 add: acc = acc + g   2 merge: g = acc + g
int dpa_grad_fold(float* acc, float* g, long n, int mode, hipStream_t s);
int dpa_opt_chunk();
int dpa_opt_max_segments();
}
