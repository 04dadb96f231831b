// Every extern "C" entry point of csrc/kernels/*.hip, declared once, grouped by the file that defines
// it.  The kernel files and the bindings that call them all include this header, so the compiler
// checks every definition and every call against one declaration (C linkage cannot be overloaded: a
// definition that drifts from its declaration here does not compile).  Host-compiler clean: only the
// HIP runtime API types.  The peer-collective launcher and its argument struct are in ipc_coll.h.
//
// Unless its own comment says otherwise, a launcher returns 0, a HIP error code (> 0) or a negative
// argument error; `st` / `s` is the stream.  The size, split and address queries among them launch
// nothing and return what their comment names.
#pragma once
#include <hip/hip_runtime_api.h>

extern "C" {
// ---- augment.hip ----
int dpa_augment(const unsigned char* img, const long long* idx, const long long* labels, float* out,
                long long* target, int B, int Hs, int Ws, int pad, int train, unsigned long long seed,
                unsigned long long salt, const float* mean, const float* std, hipStream_t st);
// mode 0 = Mixup (the box is ignored), 1 = CutMix (box [y0,y1) x [x0,x1) inside the image; lam is only
// stored).  Training augmentation only.  -2: a mode, lambda or box out of range.
int dpa_augment_mix(const unsigned char* img, const long long* idx, const long long* labels, float* out,
                    long long* target, long long* target2, float* lam_out, int mode, float lam, int y0, int y1,
                    int x0, int x1, int B, int Hs, int Ws, int pad, unsigned long long seed, unsigned long long salt,
                    const float* mean, const float* std, hipStream_t st);
// ---- bn.hip ----
// floats of partial workspace needed by fwd stats (2 per (block, channel)) / bwd (5 per ...)
// (backward: rows of the fp32 or the bf16 geometry, whichever has more; the bf16 wide reduce of
// bn_wide.hip uses the bf16 geometry's rows per block)
long dpa_bn_part_floats(int M, int C, int bwd);
// z [M][C] (or nsplit fp32 slabs of it in src; then z is written) -> partials -> finalize.
// zbf: z/src are bf16 (nsplit must be 1).
int dpa_bn_fwd_stats(const void* src, int nsplit, void* z, float* part, int M, int C, const float* gamma,
                     const float* beta, const float* bias, float* rmean, float* rvar, long long* nbt, float* mean,
                     float* invstd, float* scale, float* shift, float momentum, float eps, int zbf, hipStream_t st);
// Finalize from (mean, M2) partials of nblk row blocks of rpb rows each (the producer is not
// bn_stats_kernel, e.g. the first-layer conv's epilogue, first_layer.hip).
int dpa_bn_finalize(const float* part, int nblk, int rpb, int M, int C, const float* gamma, const float* beta,
                    const float* bias, float* rmean, float* rvar, long long* nbt, float* mean, float* invstd,
                    float* scale, float* shift, float momentum, float eps, hipStream_t st);
// Finalize from channel-major partials part[c][k] (conv epilogue statistics).
int dpa_bn_finalize_cm(const float* part, int nblk, int rpb, int M, int C, const float* gamma, const float* beta,
                       const float* bias, float* rmean, float* rvar, long long* nbt, float* mean, float* invstd,
                       float* scale, float* shift, float momentum, float eps, hipStream_t st);
int dpa_bn_eval_params(const float* gamma, const float* beta, const float* bias, const float* rmean,
                       const float* rvar, float* scale, float* shift, int C, float eps, hipStream_t st);
// out: fp32 a (np == 0), bf16 planes a3 [np][...] (np in {1, 3}) or fp16 pairs (np 2, scale H2_SA).
// act: 0 relu (pool allowed), 1 none, 2 relu(. + res).  zbf: z and res are bf16.
int dpa_bn_apply(const void* z, float* a, unsigned short* a3, int np, const float* scale, const float* shift, int N,
                 int H, int W, int C, int pool, int act, const void* res, int zbf, hipStream_t st,
                 unsigned char* mask);
// gsrc: grad of the layer output (pooled shape if pool), or nsplit fp32 slabs of it (then the sum is
// written to g).  Writes dz [N,H,W,C] (fp32, or bf16 planes dz3) and dgamma/dbeta/dbias; act 2 also
// the residual gradient dres.  zbf: gsrc/g/z/res/dres are bf16 (nsplit must be 1).  g2 (optional,
// same type and shape as g, nsplit 1): the gradient is gsrc + g2, summed on load.
int dpa_bn_bwd(const void* gsrc, int nsplit, void* g, const void* z, const float* scale, const float* shift,
               const float* mean, const float* invstd, const float* gamma, float* part, float* coef, float* dgamma,
               float* dbeta, float* dbias, float* dz, unsigned short* dz3, int np, int N, int H, int W, int C,
               int pool, int act, const void* res, void* dres, int zbf, hipStream_t st, int* sig, int sig_val,
               const void* g2, const unsigned char* mask, unsigned* bound);
// Layer-0 backward (see bn_bwd_wgrad0_kernel): BN statistics, then the fused apply + weight gradient.
// g [N,16,16,64] (or nsplit slabs of it in gsrc), z [N,32,32,64], x [N,32,32,4] fp32, dw [64,3,3,CP].
long dpa_wgrad0_part_floats(int N);
int dpa_bn_bwd_wgrad0(const float* gsrc, int nsplit, float* g, const float* z, const float* scale,
                      const float* shift, const float* mean, const float* invstd, const float* gamma, float* part,
                      float* coef, float* dgamma, float* dbeta, float* dbias, const float* x, float* wpart,
                      float* dw, int CP, int N, hipStream_t st, int* sig, int sig_val);
// ---- bn_fused.hip ----
// Geometry query: 0 when the one-launch BN runs this layer (Mo row units of C channels) with at most
// rmax row blocks per channel slice; writes the workspace floats and counter words it needs.
int dpa_bn_fused_geo(int Mo, int C, int pool, int bwd, int rmax, long* part_floats, long* cnt_words, int* blocks);
// Forward: src = z [N,H,W,C] fp32 or nsplit slabs of it (z is then written to zw); writes mean,
// invstd, scale, shift, the running statistics and nbt, and (apply != 0) relu(BN(z)) [2x2 pooled]
// as fp32 out or bf16 planes out3 [np][...] (plane stride ps).
int dpa_bn_fused_fwd(const float* src, int nsplit, float* zw, int N, int H, int W, int C, int pool, int rmax,
                     float* part, unsigned* cnt, const float* gamma, const float* beta, const float* bias,
                     float* rmean, float* rvar, long long* nbt, float* mean, float* invstd, float* scale,
                     float* shift, int apply, float* out, unsigned short* out3, int np, long ps, float momentum,
                     float eps, int* tmo, long long timeout_us, hipStream_t st);
// Backward: gsrc = dL/d(layer output) [N,Ho,Wo,C] fp32 or nsplit slabs of it; z, scale, shift, mean,
// invstd from the forward; writes dgamma, dbeta, dbias and dz (fp32 out or bf16 planes out3).
int dpa_bn_fused_bwd(const float* gsrc, int nsplit, const float* z, int N, int H, int W, int C, int pool, int rmax,
                     float* part, unsigned* cnt, const float* scale, const float* shift, const float* mean,
                     const float* invstd, const float* gamma, float* dgamma, float* dbeta, float* dbias, float* out,
                     unsigned short* out3, int np, long ps, int* tmo, long long timeout_us, hipStream_t st, int* sig,
                     int sig_val);
// ---- bn_wide.hip: bf16 passes with 16-byte lanes, tried first by bn.hip's bf16 paths ----
// Backward reduce for bf16, unpooled, unsplit tensors in bn.hip's 1024-thread geometry: rpb is
// bn.hip's rows per block (rounded up here to whole iterations, so the grid never exceeds its and
// the partial workspace fits).  Returns the number of blocks launched (the finalize's partial
// rows), 0 when not applicable (the caller runs bn.hip's kernel), or -(HIP error).
int dpa_bn_bwd_reduce_wide(const unsigned short* g, const unsigned short* g2, const unsigned short* z,
                           const unsigned short* res, const unsigned char* mask, unsigned short* dyout,
                           const float* scale, const float* shift, const float* mean, const float* invstd,
                           float* part, int Mo, int C, int act, int rpb, int* sig, int sig_val, hipStream_t st);
// bf16 [M][C] -> bf16 [M][C] (+ mask [M*C/4] bytes for act 2); returns 1 when not applicable (the
// caller runs bn.hip's kernel), else a HIP error code.  rscale / rshift (act 2 only): the residual is a
// BatchNorm input, added as bf16(fma(res, rscale, rshift)) (bn_apply_wide_kernel RBN).
int dpa_bn_apply_wide(const unsigned short* z, const unsigned short* res, unsigned short* out, unsigned char* mask,
                      const float* scale, const float* shift, long M, int C, int act, hipStream_t st,
                      const float* rscale, const float* rshift);
// backward apply, bf16: g (+ g2) and z [M][C] -> dz [M][C]; act 0 (ReLU) or 1 (identity); returns 1
// when not applicable
int dpa_bn_bwd_apply_wide(const unsigned short* g, const unsigned short* g2, const unsigned short* z,
                          unsigned short* dz, const float* scale, const float* shift, const float* coef, long M, int C,
                          int act, hipStream_t st);
// ---- conv_gemm.hip ----
// effective split count the launcher will use for a reduction of `ntiles_k` BK-tiles
int dpa_conv_splits(int Kred, int splits);
// Forward conv (and, with dgrad=1, the stride-1 "same" data-gradient conv reading the ORIGINAL
// weights with flipped taps).  x: NHWC [N,H,W,C]; w: fprop [Kout][R][S][C], dgrad [C][R][S][Kout]
// (the original conv's weights, whose input channels Kout are this GEMM's outputs); out
// [N,P,Q,Kout].  splits > 1: partial sums go to slab[splits][N,P,Q,Kout]; reduce=1 sums them into
// out here, reduce=0 leaves them for a consumer that sums on the fly (bn_fwd_stats / bn_bwd).
// tile: 0 -> 128x128 (4 waves, 64x64 each), 1 -> 64x64 (4 waves, 32x32 each)
// posmajor: position-major row order + tap skipping (any value is correct; 1 is faster on small maps)
int dpa_conv_fprop(const float* x, const float* w, float* out, float* slab, int N, int H, int W, int C, int Kout,
                   int R, int S, int stride, int pad, int splits, int tile, int dgrad, int reduce, int posmajor,
                   hipStream_t st);
// dW[Kout][R*S*C] = sum_m dZ[m][kout] * Xcol[m][rsc]
int dpa_conv_wgrad(const float* x, const float* dz, float* dw, float* slab, int N, int H, int W, int C, int Kout,
                   int R, int S, int stride, int pad, int splits, int tile, int posmajor, hipStream_t st);
int dpa_wflip(const float* w, float* wd, int K, int R, int S, int C, hipStream_t st);
// ---- conv_x3.hip ----
int dpa_x3_splits(int Kred, int splits);
// rows per row tile of fprop tile `tile` (the stats partial row block), 0 if it cannot emit stats
int dpa_conv_stats_rows(int tile);
// x planes [NP][N,H,W,C] (plane stride xps), w planes [NP][Kout][R][S][C] (stride wps; for a data
// gradient pass the flipped/transposed Wd planes), out fp32 [N,P,Q,Kout] (or slabs, see
// dpa_conv_fprop).  np: 1 (bf16), 3 (fp32 via bf16x6) or 2 (fp32 via fp16 pairs; outputs times
// h2_out_scale(oscale, obound)).  tile: 0 = 128x128, 1 = 64x64.
// posmajor: bit 0 = position-major GEMM rows, bit 1 = column-tile-outer block order (Args.nmajor;
// implicit-GEMM tiles only, the halo kernels ignore it).
// stats (optional, one split, implicit-GEMM or halo tiles): float2 [Kout][row tiles of conv_stats_rows]
// BN (mean, M2) partials of the output, channel-major (epi_col_stats), for dpa_bn_finalize_cm.
int dpa_conv_x3_fprop(const unsigned short* x, long xps, const unsigned short* w, long wps, void* out, float* slab,
                      int N, int H, int W, int C, int Kout, int R, int S, int stride, int pad, int splits, int tile,
                      int reduce, int posmajor, int np, int obf, hipStream_t st, float* stats, float oscale,
                      const unsigned* obound);
// Data gradient of conv(x [N,H,W,C], w [K,R,S,C], stride, pad) -> dZ [N,Hd,Wd,K]:
// dx [N,H,W,C] fp32 (or slabs) from dz planes [NP][N,Hd,Wd,K] and the forward weight planes.
// stride must be a power of two.
// add (optional, dx's type): dx = dgrad + add -- a second gradient contribution to the same tensor.
// With split-K it is folded into the reduction (no extra pass); with one split an in-place add
// follows (an epilogue read of the addend made the bf16 dgrad kernels ~1.7x slower: the loads sit
// in front of the stores).
int dpa_conv_x3_dgrad(const unsigned short* dz, long dzps, const unsigned short* w, long wps, void* dx, float* slab,
                      int N, int Hd, int Wd, int K, int C, int R, int S, int stride, int pad, int H, int W, int splits,
                      int tile, int reduce, int posmajor, int np, int obf, hipStream_t st, const void* add, int* sig,
                      int sig_val, float oscale, const unsigned* obound);
// dW[Kout][R*S*C] = sum_m dZ[m][kout] Xcol[m][rsc]; x planes [NP][N,H,W,C], dz planes [NP][N,P,Q,Kout]
int dpa_conv_x3_wgrad(const unsigned short* x, long xps, const unsigned short* dz, long dzps, float* dw, float* slab,
                      int N, int H, int W, int C, int Kout, int R, int S, int stride, int pad, int splits, int tile,
                      int posmajor, int np, hipStream_t st, float oscale, const unsigned* obound);
// np 2: the fp16 pairs of x * scale (scale a power of two; conv outputs divide it out)
int dpa_split_planes(const float* x, unsigned short* out, long n, long ps, int np, float scale, hipStream_t st);
// np 2: activation planes (scale H2_SA)
int dpa_pad_split8(const float* x, unsigned short* out, long npix, int cin, long ps, int np, hipStream_t st);
// ---- diag.hip ----
int dpa_spin(long long usec, int* done, hipStream_t s);
// ---- fc_ce.hip ----
// bn_z / bn_scale / bn_shift (optional, VGG head): x is then OUTPUT -- the features are computed from
// the last conv layer's z [B][2][2][Cin] (BN + ReLU + 2x2 max-pool, see BnIn) and stored there.
// parts: bit 0 = the row kernel (loss rows, dlogits, dx), bit 1 = the weight-gradient kernel (dW, db,
// batch loss).  The VGG engine issues the row kernel on the critical path and the weight gradient on
// its weight-gradient stream (nothing on the critical path reads dW, db or the loss).
// label_smoothing (0 <= eps < 1, checked by the caller) and target2 [B] / lam [B] (Mixup / CutMix pair
// targets, both or neither, else -2) pick the row kernel's target mode (ce_target.h: pair, smoothed or
// plain); only the row kernel sees them (the weight gradient reads dlogits and loss_row).
int dpa_fc_ce_train(const float* x, const float* w, const float* b, const long long* target, float* loss_row,
                    float* dlogits, float* dx, float* dw, float* db, float* loss_out, float* loss_accum, int B,
                    int Cin, int J, hipStream_t st, const float* bn_z, const float* bn_scale,
                    const float* bn_shift, int parts, float label_smoothing, const long long* target2,
                    const float* lam);
int dpa_fc_ce_eval(const float* x, const float* w, const float* b, const long long* target, float* loss_row,
                   int* correct_row, float* logits, float* acc, int B, int Cin, int J, hipStream_t st);
// ---- first_layer.hip ----
long dpa_conv0_part_floats(int N);
// Training (part != nullptr): conv + per-block statistics, then the BN finalize (batch statistics,
// running-stat update, scale/shift).  Eval (part == nullptr): conv only.
int dpa_conv0_fwd(const float* x, const float* w, int CP, float* z, float* part, int N, const float* gamma,
                  const float* beta, const float* bias, float* rmean, float* rvar, long long* nbt, float* mean,
                  float* invstd, float* scale, float* shift, float momentum, float eps, hipStream_t st);
// ---- gemm_f32.hip ----
// C = opA @ opB (+ bias): ak / bk as in gemm_f32.hip's header; splits > 1 needs slab >= splits * M * N
// floats and M * N % 4 == 0.
int dpa_gemm_f32(const float* A, int lda, int ak, const float* B, int ldb, int bk, float* C, int M, int N, int K,
                 const float* bias, float* slab, int splits, hipStream_t st);
// ---- grad_fold.hip ----
// gradient accumulation over n elements (n % 4 == 0, else -1):
// mode 0 store: acc = g   1 add: acc = acc + g   2 merge: g = acc + g
int dpa_grad_fold(float* acc, float* g, long n, int mode, hipStream_t s);
// ---- head.hip ----
int dpa_gap(const void* x, float* feat, int N, int HW, int C, int xbf, hipStream_t st);
// label_smoothing (0 <= eps < 1, checked by the caller), target2 [N] / lam [N] (both or neither, else
// -2): the row kernel's target mode, as dpa_fc_ce_train.
int dpa_ce(const float* logits, const long long* target, float* loss_row, float* dlogits, int* correct_row,
           float* loss, float* acc, int N, int J, hipStream_t st, float label_smoothing, const long long* target2,
           const float* lam);
int dpa_head_bwd_prep(const float* dlogits, const float* gout, float* dl, float* db, int N, int J, hipStream_t st);
int dpa_gap_bwd(const float* dfeat, void* dx, int N, int HW, int C, int xbf, hipStream_t st);
// ---- lars.hip, lr_sched.hip, sgd.hip: the optimizer ----
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
int dpa_opt_chunk();
int dpa_opt_max_segments();
// sgd.hip, besides the optimizer: the mean over W stacked copies, and out += add over n elements
// (n % 4 == 0, else -1; bf: bf16, else fp32)
int dpa_mean_of_w(const float* in, float* out, long n, int W, hipStream_t s);
int dpa_add_inplace(void* out, const void* add, long n, int bf, hipStream_t s);
// ---- pool.hip ----
// x [N,H,W,C] (C % 8 == 0) fp32 (bf=0) or bf16 (bf=1) -> y [N,P,Q,C], arg uint8 [N,P,Q,C].
// scale / shift (both or neither, [C] fp32): x is a BatchNorm input, pooled as relu(x*scale + shift).
int dpa_maxpool_fwd(const void* x, void* y, unsigned char* arg, int N, int H, int W, int C, int k, int s, int p,
                    int bf, hipStream_t st, const float* scale, const float* shift);
// dy [N,P,Q,C], arg from the forward -> dx [N,H,W,C] (every element written)
int dpa_maxpool_bwd(const void* dy, const unsigned char* arg, void* dx, int N, int H, int W, int C, int k, int s,
                    int p, int bf, hipStream_t st);
// ---- signal.hip ----
int dpa_wait_signal(const int* sig, int val, long long timeout_us, int* tmo, hipStream_t st);
int dpa_set_signal(int* sig, int val, hipStream_t st);
// w: device array of n (<= 63) word pointers; out: 64 ints of host-pinned (device-mapped) memory
int dpa_health_copy(const int* const* w, int n, int* out, int tag, hipStream_t st);
// ---- DPA_H2_OVF_ACCESSOR (common.h): a translation unit's fp16-pair overflow word, read and
// optionally cleared from the host, and its device address ----
int dpa_h2_ovf_bn(int clear);  // bn.hip
int* dpa_h2_ovf_bn_addr();
int dpa_h2_ovf_conv(int clear);  // conv_x3.hip
int* dpa_h2_ovf_conv_addr();
int dpa_h2_ovf_fused(int clear);  // bn_fused.hip
int* dpa_h2_ovf_fused_addr();
int dpa_h2_ovf_lars(int clear);  // lars.hip
int* dpa_h2_ovf_lars_addr();
int dpa_h2_ovf_sgd(int clear);  // sgd.hip
int* dpa_h2_ovf_sgd_addr();
}
