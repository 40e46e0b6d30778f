/*
 * adnm_hip.h — C-ABI of libadnm_hip.so, the MI355X (gfx950) kernels behind the ADNM-UNet
 * training hot path.
 *
 * The reference (kanyu369/ADNM-UNet) has no FFI of its own: its hot ops are torch / mamba_ssm
 * calls inside nn.Module.forward().  Each entry point below names the reference call site it
 * replaces (file:line under the reference tree).  The Python modules in
 * adnm-unet_amd/models/ keep the reference's nn.Module surface and call these through
 * ctypes (adnm-unet_amd/adnm_hip/lib.py); INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (torch allocator); no compute entry point
 *    allocates, frees, synchronises or touches the host copy of anything (the two setup-time helpers
 *    adnm_uncached_alloc / adnm_uncached_free exist so that the CALLER can own the uncached workspace
 *    of split GEMM launches: see adnm_skgemm);
 *  - kernels are enqueued on `stream` (torch.cuda.current_stream().cuda_stream) and are
 *    hipGraph-capturable; workspace is passed in, its size comes from the *_ws_bytes helper;
 *  - token tensors are channels-last ("BLD" = (B, H*W, C) = NHWC), the layout the reference
 *    keeps between stages (ADNMUNet.py:119, model_untils.py:21-27);
 *  - `dtype` selects the storage type of activations: ADNM_F32 (0) or ADNM_BF16 (1);
 *    parameters, statistics, reductions and workspaces are always fp32;
 *  - a row operand is (pointer, row stride in elements): a column slice of a wider buffer is passed as it lies.  The row
 *    kernels (rownorm, ssd_reduce, gate, catmix, lincomb, mixnorm, dwconv) move 4 elements per access, so they ask for a row
 *    stride >= the width and a multiple of 4, and a base pointer aligned to 4 elements (16 bytes of fp32, 8 of bf16; dwconv:
 *    16 bytes for both); operands read element by element (dt_raw, everything of ssd_scan) only need rows and head strides
 *    that hold what they address.  A row operand that breaks this is rejected (parameter vectors, also read 16 bytes at a
 *    time, are taken as the allocator hands them out and are not checked);
 *  - return value 0 = launched; negative = rejected (nothing launched), text via
 *    adnm_last_error() (thread-local).  The compute entry points keep no global mutable state: they are re-entrant
 *    per thread / stream / device (the reference's nn.DataParallel calls them from one thread per device).  The only
 *    process-wide state is the opt-in profiler's record list (adnm_prof_*, mutex-guarded), per-device "dynamic LDS
 *    limit raised" flags (atomics; setting one twice is harmless) and the thread-local error string and fold- / leaf-queue
 *    bindings.  There are no library-owned device buffers.
 */
#ifndef ADNM_HIP_H
#define ADNM_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* adnm_stream_t; /* hipStream_t */

enum { ADNM_F32 = 0, ADNM_BF16 = 1 };
enum { ADNM_ACT_NONE = 0, ADNM_ACT_SILU = 1, ADNM_ACT_GELU = 2 };
enum { ADNM_OK = 0, ADNM_EINVAL = -1, ADNM_ELAUNCH = -2, ADNM_EWORKSPACE = -3 };
/* `prec` of the GEMM-shaped entry points (tsgemm, skgemm, conv3) — the precision ladder, storage stays fp32:
 *   ADNM_MFMA_F32   exact fp32 MFMA (v_mfma_f32_16x16x4_f32: the parity path);
 *   ADNM_MFMA_BF16  operands rounded to bf16 on the way into v_mfma_f32_16x16x32_bf16, fp32 accumulation (BASELINE configs 2-4);
 *   ADNM_MFMA_FP8   BASELINE config 5: per-tensor scaled OCP fp8 operands into v_mfma_f32_16x16x32_fp8_fp8, fp32 accumulation:
 *                   first operand (the activation rows) e4m3, second (the weight) e4m3;
 *   ADNM_MFMA_FP8_GRAD  the same with the first operand in e5m2 (a gradient: output gradients into the input-gradient GEMMs).
 * The fp8 modes need a quantisation record `q` (device memory, 8 floats): {scale_a, scale_b, amax_a, amax_b, fmax_a, fmax_b, record, -}.
 * An operand value v enters the MFMA as fp8(clamp(v * scale)), the accumulator is multiplied by 1 / (scale_a * scale_b) before bias /
 * activation.  With q != NULL and record != 0 (any prec) the launch also collects amax_a / amax_b = max |v| of the operands it read
 * (atomic max, order-independent); adnm_quant_update turns them into the next scales (delayed per-tensor scaling: a tensor's scale
 * comes from an earlier step's amax, so quantisation costs no extra pass over the activations).  q == NULL: scales 1, nothing recorded. */
enum { ADNM_MFMA_F32 = 0, ADNM_MFMA_BF16 = 1, ADNM_MFMA_FP8 = 2, ADNM_MFMA_FP8_GRAD = 3 };
/* storage of a GEMM's weight operand (b_dtype of adnm_skgemm): fp32 master values or the narrow shadow kept beside them */
enum { ADNM_B_F32 = 0, ADNM_B_BF16 = 1, ADNM_B_FP8 = 2 };

/* One pass over a table of `n` quantisation records (n * 8 floats), once per training step:
 *   state = {step counter, period}: the counter advances; records collect amax (record = 1) during the steps where counter % period == 0;
 *   after such a step: scale_x = fmax_x / (amax_x * headroom) for every operand with amax_x > 0 (else unchanged), amax_x = 0.
 * fmax_a / fmax_b are set by the caller when a record is created (448 for e4m3 operands, 57344 for e5m2).  headroom >= 1 leaves room
 * for the tensor to grow between calibrations (2 = one binade). */
int adnm_quant_update(float* table, int64_t n, float* state, float headroom, adnm_stream_t stream);
/* The same pass behind adnm_step_guard (below: the monitored training step), reading the skip flag of the statistics block `stats` from
 * device memory.  Flag set: amax_a = amax_b = 0 in every record of a GEMM call site (fmax_a > 0): what the skipped step collected is
 * discarded; a weight record (fmax_a == 0) keeps its amax_b, which the optimiser pass of the step BEFORE gathered over finite weights.
 * NOTHING else is written: scales, record flags and the step counter stay, so a skipped calibration step is repeated by the next one
 * and ends in the scales the skipped one would have made.  Flag clear: bit-identical to adnm_quant_update. */
int adnm_quant_update_guarded(float* table, int64_t n, float* state, float headroom, const void* stats, adnm_stream_t stream);

const char* adnm_last_error(void);
int adnm_abi_version(void);

/* Opt-in measurement aid (off by default): when enabled every kernel launch of the library is bracketed by
 * hipEventRecord on its own stream.  adnm_prof_collect synchronises those events and writes one line per kernel
 * name "name\tlaunches\ttotal_ms\talgorithmic_bytes\n" into buf (returns the full length).  bench.py uses it
 * for the roofline figures; nothing else calls it. */
int adnm_prof_enable(int on);
int64_t adnm_prof_collect(char* buf, int64_t buflen);

/* Deferred second-stage folds.  Every cross-workgroup reduction of the library is "fp32 partials + a deterministic fold launch".
 * For parameter gradients (nothing reads them before clip_grad_norm_ / the optimiser, train.py:140-144) the caller may batch
 * those fold launches: create a queue, bind it on the calling thread around *_bwd entry points (their folds are then QUEUED, the
 * partial workspaces and destinations must stay alive), and flush it — one launch per 16 queued folds — before anything reads
 * the results.  Unbound (the default) every fold is launched at once.  The queue is a caller-owned host object; the binding is
 * thread-local (like adnm_last_error), so concurrent threads / devices do not see each other's queues.  Results are bitwise
 * the same either way. */
void* adnm_foldq_create(void);
int adnm_foldq_destroy(void* q);
int adnm_foldq_bind(void* q); /* NULL unbinds */
int64_t adnm_foldq_pending(void* q);
int adnm_foldq_flush(void* q, adnm_stream_t stream);
int adnm_foldq_clear(void* q); /* drop the queued folds without launching them (error path of the caller) */
/* The NEXT fold queued on this thread adds to its destination segment q (instead of overwriting it) for every bit q of mask: a parameter
 * used by two autograd nodes (Block's beta1 / beta2 feed both residual mixes, ADNMUNet.py:152,158) gets the second node's contribution
 * added by the fold itself — flushes launch the overwriting folds first — instead of by a separate autograd add per node.  Only
 * meaningful while a queue is bound (ignored otherwise: an immediate fold always overwrites). */
int adnm_foldq_accumulate_next(int mask);

/* Deferred leaf launches.  The weight-gradient GEMMs of a backward pass (ADNM_SKGEMM_TN) are leaves — nothing reads dW before
 * clip_grad_norm_ / the optimiser (train.py:140-144) — and individually small (70 launches of ~10 us at config 2).  While the calling
 * thread has bound BOTH a leaf queue and a fold queue, adnm_skgemm(TN) stores its prepared launch instead of making it (operands,
 * workspace and destination must stay alive); adnm_leafq_flush launches the stored problems grouped, 16 per launch, and must be called
 * BEFORE adnm_foldq_flush (the folds of split problems read the partials those launches write).  Results are bitwise the same either way.
 * The same holds for adnm_tsgemm_tn, the weight gradients of adnm_dwconv_bwd / adnm_dwconv_wgrad (fp32 tokens), adnm_conv3_wgrad and the
 * two-stage path of adnm_colsum; the last three kinds — the 3x3 column walker of maps of 128 x 128 pixels and more, conv3, colsum — keep
 * the plan of their single launch, so their results do not depend on the queue at all.  ADNM_LEAF_INLINE (environment, a bit mask over
 * the kinds of csrc/adnm_common.h, read at every push) sends kinds back inline: a measurement aid. */
void* adnm_leafq_create(void);
int adnm_leafq_destroy(void* q);
int adnm_leafq_bind(void* q); /* NULL unbinds */
int64_t adnm_leafq_pending(void* q);
int adnm_leafq_flush(void* q, adnm_stream_t stream);
int adnm_leafq_clear(void* q);

/* Launch group: the same step of several INDEPENDENT, structurally identical chains as one launch (EncoderToDecoder's three skip
 * chains: each of their kernels fills a small part of the chip, and the runtime does not overlap independent launches).
 * Contract: the calls the thread makes between adnm_group_begin and adnm_group_launch are mutually independent problems, each of which
 * depends only on work enqueued before adnm_group_begin.  An entry point that knows about groups — adnm_skgemm with ops NT and NN (both of
 * its kernels), adnm_dwconv_fwd, adnm_dwconv_bwd (dpre and the input gradient: two positions; with a weight-gradient destination it is
 * refused inside a group, adnm_dwconv_wgrad is a call of its own behind the launch), adnm_gate_fwd / _bwd, adnm_instnorm_fwd / _bwd (two
 * positions each; without a bound fold queue the fold of the scalar gradients is recorded behind them), adnm_igate_res_fwd / _bwd (likewise),
 * adnm_skipgate_fwd (pools, then branches: two positions) / _bwd (pointwise gate, grouped conv, pools: three positions; its folds likewise)
 * — then stores its fully prepared launch instead of making it (operands, outputs and workspaces must stay alive, and two
 * split problems need DISJOINT counter / slab ranges); every other entry point launches at once, which the contract allows.
 * adnm_group_launch issues the stored launches on `stream`: those of one kernel instantiation merged into one multi-problem launch (up to 8
 * problems; descriptors in the kernel-argument segment), a record without a partner alone.  Every problem keeps the plan, the grid and
 * the workgroup arithmetic it has alone: results are bitwise those of separate launches.  A merged launch is one profiler event under the
 * entry point's own scope name with the summed bytes.
 * Groups are per thread and do not nest (a second begin: EINVAL); adnm_foldq_flush / adnm_leafq_flush are refused while one is open;
 * a launch with nothing recorded is ADNM_OK; adnm_group_clear closes the group and forgets what it recorded (the error path). */
int adnm_group_begin(void);
int adnm_group_launch(adnm_stream_t stream);
int adnm_group_clear(void);
int64_t adnm_group_pending(void);

/* ---------------------------------------------------------------- row norms (K2, K7)
 * y = scale * ( xhat * w + b ) + shift,  xhat = (x - mu) * rstd
 *   RMSNorm   (mamba_ssm RMSNorm bound at ADNMUNet.py:278, used ADNMUNet.py:149,155): subtract_mean=0, b=NULL
 *   LayerNorm (ADNssd.py:456, Vssd.py:280):                                           subtract_mean=1
 *   BiasFree_LayerNorm (model_untils.py:43-48):                                       subtract_mean=1, b=NULL
 * scale/shift are the scalar learnable affine of Block.forward (ADNMUNet.py:149,155) as
 * 1-element device tensors, or NULL (= 1 / 0).  x:(M,d) with row stride ldx, y row stride ldy
 * (elements).  mu,rstd: (M) fp32 statistics saved for backward (mu unused for RMS). d % 4 == 0. */
int adnm_rownorm_fwd(const void* x, int64_t ldx, const float* w, const float* b, const float* scale,
                     const float* shift, void* y, int64_t ldy, float* mu, float* rstd, int64_t M, int64_t d,
                     float eps, int subtract_mean, int dtype, adnm_stream_t stream);
/* dx:(M,d) stride lddx; dw,db:(d); dscale,dshift:(1) — any of db/dscale/dshift may be NULL.
 * dres (optional, (M,d) stride lddres): the gradient reaching x through the residual path of a pre-norm block
 * (ADNMUNet.py:152,158: x' = beta1*x + beta2*f(norm(x))) — added into dx in the same pass, so autograd's separate add disappears.
 * ws: fp32 workspace of adnm_rownorm_bwd_ws_bytes(M,d) bytes. Parameter grads are OVERWRITTEN. */
int64_t adnm_rownorm_bwd_ws_bytes(int64_t M, int64_t d);
int adnm_rownorm_bwd(const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* w, const float* b,
                     const float* scale, const float* mu, const float* rstd, void* dx, int64_t lddx, float* dw,
                     float* db, float* dscale, float* dshift, const void* dres, int64_t lddres, void* ws, int64_t ws_bytes,
                     int64_t M, int64_t d, int subtract_mean, int dtype, adnm_stream_t stream);

/* ---------------------------------------------------------------- SSD reduction form (K1)
 * non_casual_linear_attn (ADNssd.py:252-299, Vssd.py:161-208):
 *   dt = softplus(dt_raw + dt_bias)                      (ADNssd.py:318 fused here)
 *   KV[b,h,n,p] = sum_l Bm[b,l,g(h),n] * x[b,l,h,p] * dt[b,l,h] * exp(A_log[h])
 *   y[b,l,h,p]  = sum_n Cm[b,l,g(h),n] * KV[b,h,n,p] + D[h] * x[b,l,h,p],     g(h) = h % G
 * x:(B,L,H,P) row(token) stride ldx; Bm,Cm:(B,L,G*N) strides ldb,ldc; dt_raw:(B,L,H) stride lddt with
 * per-head element stride dt_hstride (2 for the even/odd head split of ADNssd.py:375-378);
 * dt_bias,A_log,D indexed [h*p_hstride] likewise.  y stride ldy.  kv:(B,H,N,P) fp32 (saved for backward).
 * (P,N) in {(4,8),(4,16),(8,8)}, G in {1,2,4}.  The three contractions run on v_mfma_f32_16x16x4_f32 (exact fp32).
 * Optional fused epilogue (yn != NULL; needs H*P == 64, i.e. the token row is one head block — the refiner mixers): the mixer's
 * LayerNorm(d_inner) of ADNssd.py:456, yn = (y - mean) * rstd * ln_w + ln_b over the H*P columns of the row, written with row
 * stride ldyn next to y itself; ln_mu, ln_rstd:(B*L) fp32 statistics saved for adnm_rownorm_bwd.  yn == NULL: the ln_* arguments
 * are ignored. */
int64_t adnm_ssd_ws_bytes(int64_t B, int64_t L, int64_t H, int64_t P, int64_t N, int64_t G);
int adnm_ssd_reduce_fwd(const void* x, int64_t ldx, const void* Bm, int64_t ldb, const void* Cm, int64_t ldc,
                        const void* dt_raw, int64_t lddt, int64_t dt_hstride, const float* dt_bias,
                        const float* A_log, const float* D, int64_t p_hstride, void* y, int64_t ldy, float* kv,
                        const float* ln_w, const float* ln_b, void* yn, int64_t ldyn, float* ln_mu, float* ln_rstd,
                        float ln_eps, void* ws, int64_t ws_bytes, int64_t B, int64_t L, int64_t H, int64_t P, int64_t N,
                        int64_t G, int dtype, adnm_stream_t stream);
/* gradients: dx,dBm,dCm,ddt_raw share the strides of their primals (they may alias slices of one
 * wide gradient buffer); ddt_bias,dA_log,dD:(H) contiguous fp32, OVERWRITTEN. */
int adnm_ssd_reduce_bwd(const void* dy, int64_t lddy, const void* x, int64_t ldx, const void* Bm, int64_t ldb,
                        const void* Cm, int64_t ldc, const void* dt_raw, int64_t lddt, int64_t dt_hstride,
                        const float* dt_bias, const float* A_log, const float* D, int64_t p_hstride,
                        const float* kv, void* dx, int64_t lddx, void* dBm, int64_t lddb, void* dCm, int64_t lddc,
                        void* ddt_raw, int64_t ldddt, float* ddt_bias, float* dA_log, float* dD, void* ws,
                        int64_t ws_bytes, int64_t B, int64_t L, int64_t H, int64_t P, int64_t N, int64_t G,
                        int dtype, adnm_stream_t stream);

/* ---------------------------------------------------------------- SSD chunked scan (K1b) — PARITY UNPINNED
 * The `linear_attn_duality=False` branch (ADNssd.py:413-454, Vssd.py:245-275): mamba_ssm's
 * mamba_chunk_scan_combined(x, dt, A, B, C, chunk_size, D, z=None) — un-vendored Triton in the reference:
 *   d_t = exp(dt_t*A_h), S_t = d_t S_{t-1} + dt_t B_t (x) x_t, y_t = C_t.S_t + D_h x_t,  dt = softplus(dt_raw+dt_bias),
 *   A_h = -exp(A_log[h]); head h reads K/Q group h / (H/G).  reverse=1 scans the sequence backwards (the reference
 * flips the odd half, ADNssd.py:425-435).  x/y/dx: element (row, h, p) at ptr[row*ld + h*hstride + p];
 * dt_raw (row, h) at ptr[row*lddt + h*dt_hstride]; dt_bias/A_log/D at [h*p_hstride].  S_in: (B,H,ceil(L/chunk),P,N)
 * fp32 entering states, written by fwd and read by bwd.  P = 4, N in {8,16}, fp32 only. */
int64_t adnm_ssd_scan_ws_bytes(int64_t B, int64_t L, int64_t H, int64_t N, int64_t chunk, int backward);
int adnm_ssd_scan_fwd(const void* x, int64_t ldx, int64_t x_hstride, const void* Bm, int64_t ldb, const void* Cm,
                      int64_t ldc, const void* dt_raw, int64_t lddt, int64_t dt_hstride, const float* dt_bias,
                      const float* A_log, const float* D, int64_t p_hstride, void* y, int64_t ldy, int64_t y_hstride,
                      float* S_in, void* ws, int64_t ws_bytes, int64_t B, int64_t L, int64_t H, int64_t P, int64_t N,
                      int64_t G, int64_t chunk, int reverse, int dtype, adnm_stream_t stream);
int adnm_ssd_scan_bwd(const void* dy, int64_t lddy, int64_t dy_hstride, const void* x, int64_t ldx, int64_t x_hstride,
                      const void* Bm, int64_t ldb, const void* Cm, int64_t ldc, const void* dt_raw, int64_t lddt,
                      int64_t dt_hstride, const float* dt_bias, const float* A_log, const float* D, int64_t p_hstride,
                      const float* S_in, void* dx, int64_t lddx, int64_t dx_hstride, void* dBm, int64_t lddb, void* dCm,
                      int64_t lddc, void* ddt_raw, int64_t ldddt, int64_t ddt_hstride, float* ddt_bias, float* dA_log,
                      float* dD, void* ws, int64_t ws_bytes, int64_t B, int64_t L, int64_t H, int64_t P, int64_t N,
                      int64_t G, int64_t chunk, int reverse, int dtype, adnm_stream_t stream);

/* ---------------------------------------------------------------- depthwise conv, NHWC (K4, part of K3)
 * y[b,h,w,c] = act( sum_{i,j} wgt[c,i,j] * x[b,h+i-KH/2,w+j-KW/2,c] + bias[c] ) (+ addend[b,h,w,c])
 * replaces the depthwise nn.Conv2d calls at ADNssd.py:334,343-346,389, Vssd.py:233,
 * model_untils.py:180-188 (FeedForward.dwconv), :203-211 (ConvFFD.dw_conv), WTConv2d.py:81,86 —
 * applied directly on the token layout, so the reference's BLD<->BCHW permute().contiguous()
 * copies disappear.  x pixel stride ldx, y pixel stride ldy, addend pixel stride ldadd (elements);
 * wgt, fp32: wlayout 0 = TAP-MAJOR (KH,KW,C) (one float4 per tap and channel quad: what the parameter-prep kernels
 * emit), wlayout 1 = nn.Conv2d's own (C,1,KH,KW) (no transposes around the call); KH == KW in {3,5}; C % 4 == 0
 * (the 5-channel input stage is zero-padded to 8 channels by the caller). */
int adnm_dwconv_fwd(const void* x, int64_t ldx, const float* wgt, const float* bias, const void* addend,
                    int64_t ldadd, void* y, int64_t ldy, int64_t B, int64_t H, int64_t W, int64_t C, int KH,
                    int KW, int act, int wlayout, int dtype, adnm_stream_t stream);
/* dpre:(B,H,W,C) contiguous scratch in activation dtype (ignored when act==NONE).
 * dwgt: same layout as wgt (wlayout), dbias:(C) or NULL: OVERWRITTEN.  dwgt == NULL skips the weight-gradient pass
 * (constant taps, e.g. the average pools of EncoderToDecoder expressed as a depthwise conv). */
int64_t adnm_dwconv_bwd_ws_bytes(int64_t B, int64_t H, int64_t W, int64_t C, int KH, int KW);
int adnm_dwconv_bwd(const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* wgt,
                    const float* bias, void* dpre, void* dx, int64_t lddx, float* dwgt, float* dbias, void* ws,
                    int64_t ws_bytes, int64_t B, int64_t H, int64_t W, int64_t C, int KH, int KW, int act,
                    int wlayout, int dtype, adnm_stream_t stream);
/* the weight / bias gradient of adnm_dwconv_bwd alone (g = its dpre, or dy when no activation is fused), e.g. on another stream than the
 * input-gradient chain; adnm_dwconv_bwd with dwgt = NULL then skips it.  Workspace: adnm_dwconv_bwd_ws_bytes. */
int adnm_dwconv_wgrad(const void* g, int64_t ldg, const void* x, int64_t ldx, float* dwgt, float* dbias, void* ws, int64_t ws_bytes,
                      int64_t B, int64_t H, int64_t W, int64_t C, int KH, int KW, int wlayout, int dtype, adnm_stream_t stream);

/* ---------------------------------------------------------------- Haar butterflies, NHWC (K3)
 * wavelet_transform / inverse_wavelet_transform with db1 (WTConv2d.py:31-51): per 2x2 block
 * [[a,b],[c,d]]: LL=(a+b+c+d)/2, k1=(a+b-c-d)/2, k2=(a-b+c-d)/2, k3=(a-b-c+d)/2; output channel c*4+k.
 * dwt: x:(B,H,W,C) with pixel stride ldx and channel stride cx (4 when x is the LL band of a previous
 * level) -> y:(B,ceil(H/2),ceil(W/2),4C) contiguous; odd H/W are zero-padded (WTConv2d.py:114-116).
 * idwt: s:(B,h,w,4C) contiguous, optional ll_add:(B,h,w,C) contiguous added to the LL band
 * (WTConv2d.py:136) -> y:(B,H,W,C) contiguous with H in {2h-1,2h}, W in {2w-1,2w} (crop, :141).
 * The butterfly is its own transpose, so dwt's backward is idwt and vice versa. */
int adnm_haar_dwt(const void* x, int64_t ldx, int64_t cx, void* y, int64_t B, int64_t H, int64_t W, int64_t C,
                  int dtype, adnm_stream_t stream);
/* One ANALYSIS LEVEL of WTConv2d fused (WTConv2d.py:111-124): sub = DWT(x) and tag = depthwise KxK 'same' conv of sub (taps tap-major
 * (K*K, 4C) fp32, wavelet_scale folded in) in ONE launch (csrc/wtlevel.hip: the sub-band tile + halo lives in LDS).  x: (B,H,W) pixel rows
 * of stride ldx, channel c at column c*cx (cx = 4: the LL band of the previous level's sub-band tensor); sub, tag: (B,ceil(H/2),ceil(W/2),4C)
 * contiguous fp32, OVERWRITTEN.  flip != 0: flipped taps — one level of the backward pass (dm = DWT(d r), d sub = conv^T(dm)).  K in {3, 5}. */
int adnm_wt_level(const float* x, int64_t ldx, int64_t cx, const float* taps, float* sub, float* tag, int64_t B, int64_t H, int64_t W,
                  int64_t C, int K, int flip, adnm_stream_t stream);
/* Level 0 of a WTConv2d module (cx = 1) together with the module's base depthwise KxK conv of the same input, in one launch: sub and tag as
 * adnm_wt_level; ybase (B,H,W,C) contiguous fp32, OVERWRITTEN, = conv(x, base_taps) + base_bias (base_taps (K*K, C) tap-major fp32, base_bias
 * (C) or NULL) — or, flip != 0, the correlation with the flipped base taps and no bias (the base conv's input gradient).  Bit for bit what
 * adnm_dwconv_fwd (no activation, no addend) / the input-gradient launch of adnm_dwconv_bwd write for the same operands. */
int adnm_wt_level_base(const float* x, int64_t ldx, const float* taps, const float* base_taps, const float* base_bias, float* sub, float* tag,
                       float* ybase, int64_t B, int64_t H, int64_t W, int64_t C, int K, int flip, adnm_stream_t stream);
/* y_add1 / y_add2 (optional, (B,H,W,C) like y): added to the result in the same pass — WTConv2d's backward sums its input-gradient
 * paths (pyramid + base conv + the input's other consumer) there instead of in separate adds.
 * up1 / up2 (optional): the sub-band tensors of the next one / two COARSER levels ((B, ceil(h/2), ceil(w/2), 4C) with h, w the sub-band
 * size of the level below): the synthesis cascade (WTConv2d.py:128-141) in ONE launch — the LL addend of `s` is derived from them instead of
 * being read; ll_add then belongs to the coarsest level given.  Bitwise equal to the chain of single-level calls. */
int adnm_haar_idwt(const void* s, const void* up1, const void* up2, const void* ll_add, const void* y_add1, const void* y_add2, void* y,
                   int64_t B, int64_t H, int64_t W, int64_t C, int dtype, adnm_stream_t stream);

/* ---------------------------------------------------------------- max pooling, NHWC (K11)
 * nn.MaxPool2d on tokens: stride == kernel in [2,4] (DownSample, model_untils.py:472-487; floor mode) or stride 1 with
 * kernel 1x3 / 3x1 / 3x3 and -inf 'same' padding (EncoderToDecoder, model_untils.py:690-719).  x:(B,H,W,C),
 * y:(B,Ho,Wo,C) contiguous.  bwd recomputes the first arg-max of every window (ATen's tie rule): no index tensor; dx_add (optional, like
 * x): the gradient of x's other consumer, added in the same pass (an encoder stage's output is pooled AND kept as a skip tensor). */
int adnm_maxpool_fwd(const void* x, void* y, int64_t B, int64_t H, int64_t W, int64_t C, int kh, int kw, int stride,
                     int dtype, adnm_stream_t stream);
int adnm_maxpool_bwd(const void* dy, const void* x, const void* dx_add, void* dx, int64_t B, int64_t H, int64_t W, int64_t C, int kh,
                     int kw, int stride, int dtype, adnm_stream_t stream);

/* ---------------------------------------------------------------- InstanceNorm2d, NHWC (K8)
 * y = act( scale * (x - mean_{hw}) * rsqrt(var_{hw} + eps) + shift ), per (b,c) plane, no affine,
 * external scalar scale/shift (model_untils.py:90,113,155; nn.InstanceNorm2d at :284,371,741,814).
 * x,y:(B,HW,C) contiguous; mu,rstd:(B,C) fp32 saved for backward. act in {NONE, GELU}. */
int64_t adnm_instnorm_ws_bytes(int64_t B, int64_t HW, int64_t C);
int adnm_instnorm_fwd(const void* x, const float* scale, const float* shift, void* y, float* mu, float* rstd,
                      void* ws, int64_t ws_bytes, int64_t B, int64_t HW, int64_t C, float eps, int act, int dtype,
                      adnm_stream_t stream);
int adnm_instnorm_bwd(const void* dy, const void* x, const float* scale, const float* shift, const float* mu,
                      const float* rstd, void* dx, float* dscale, float* dshift, void* ws, int64_t ws_bytes,
                      int64_t B, int64_t HW, int64_t C, int act, int dtype, adnm_stream_t stream);

/* ---------------------------------------------------------------- GroupNorm, NHWC
 * y = act( scale * (gamma_c * (x - mean_{b,g}) * rsqrt(var_{b,g} + eps) + beta_c) + shift ): nn.GroupNorm(G, C), the norm the
 * reference builds instead of nn.InstanceNorm2d when InstanceNorm=False (model_untils.py:284,371,741,814; the long-interval recipe of
 * ADNMUNet.py:906-940), with the same external scalar scale/shift (model_untils.py:90,113,155) and activation fused.  Group g = channels
 * [g*C/G, (g+1)*C/G); mean and (biased) variance over HW x C/G elements.  gamma, beta: (C) fp32 = GroupNorm.weight / .bias, NULL = 1 / 0;
 * scale, shift: NULL = 1 / 0.  x,y:(B,HW,C) contiguous; mu,rstd:(B,G) fp32 saved for backward.  act in {NONE, GELU}.
 * Supported: C % 4 == 0, C % G == 0 and (C/G) % 4 == 0 (a lane's 16-byte channel quad lies inside one group); anything else is EINVAL.
 * bwd: dx, and the parameter gradients dgamma, dbeta (C each), dscale, dshift (NULL = not wanted) through per-workgroup fp32 partials
 * and the shared deterministic fold (deferred while a fold queue is bound: ws must then stay untouched until adnm_foldq_flush). */
int64_t adnm_groupnorm_ws_bytes(int64_t B, int64_t HW, int64_t C, int64_t G);
int adnm_groupnorm_fwd(const void* x, const float* gamma, const float* beta, const float* scale, const float* shift, void* y,
                       float* mu, float* rstd, void* ws, int64_t ws_bytes, int64_t B, int64_t HW, int64_t C, int64_t G, float eps,
                       int act, int dtype, adnm_stream_t stream);
int adnm_groupnorm_bwd(const void* dy, const void* x, const float* gamma, const float* beta, const float* scale, const float* shift,
                       const float* mu, const float* rstd, void* dx, float* dgamma, float* dbeta, float* dscale, float* dshift,
                       void* ws, int64_t ws_bytes, int64_t B, int64_t HW, int64_t C, int64_t G, int act, int dtype,
                       adnm_stream_t stream);

/* ---------------------------------------------------------------- gated FFN activation (part of K6's epilogue)
 * FeedForward.forward (model_untils.py:194-195): h:(M,2F) -> y[m,f] = gelu(h[m,f]) * sigmoid(h[m,F+f]).
 * bwd: dh:(M,2F) from dy:(M,F).  F % 4 == 0; row strides in elements. */
int adnm_gate_fwd(const void* h, int64_t ldh, void* y, int64_t ldy, int64_t M, int64_t F, int dtype,
                  adnm_stream_t stream);
int adnm_gate_bwd(const void* dy, int64_t lddy, const void* h, int64_t ldh, void* dh, int64_t lddh, int64_t M,
                  int64_t F, int dtype, adnm_stream_t stream);

/* ---------------------------------------------------------------- IntensityGate (K11)
 * y = silu(enhance * (x - threshold)) with both scalars learnable (model_untils.py:523-532; 4 per EncoderToDecoder
 * + the bridge's gates).  n contiguous elements, n % 4 == 0.  bwd also gives d enhance, d threshold (OVERWRITTEN). */
int adnm_igate_fwd(const void* x, const float* enhance, const float* threshold, void* y, int64_t n, int dtype,
                   adnm_stream_t stream);
int64_t adnm_igate_bwd_ws_bytes(int64_t n);
int adnm_igate_bwd(const void* dy, const void* x, const float* enhance, const float* threshold, void* dx, float* denhance,
                   float* dthreshold, void* ws, int64_t ws_bytes, int64_t n, int dtype, adnm_stream_t stream);
/* EncoderToDecoder's entry, fused (model_untils.py:761-763: x = self.act(x + self.gama * res), act = IntensityGate):
 *   y[b,l,c] = silu(enhance * (x[b,l,c] + gama * res[b,c] - threshold)),   x, y:(B,L,C) fp32 contiguous, res:(B,C) — the
 * channel-attention gate of Channel_Att_Bridge, one value per (sample, channel), which the reference expands over the tokens
 * (model_untils.py:604-613); per_token != 0: res is the expanded (B,L,C) tensor itself (the reference's own call form).
 * gama / enhance / threshold: 1-element fp32.  C % 4 == 0.
 * Backward: dx:(B,L,C), dres: the shape of res (complete when the launch ends), dgama/denhance/dthreshold:(1) through per-workgroup partials
 * + one fold (deferrable: parameter gradients).  All OVERWRITTEN. */
int adnm_igate_res_fwd(const float* x, const float* res, int per_token, const float* gama, const float* enhance,
                       const float* threshold, float* y, int64_t B, int64_t L, int64_t C, adnm_stream_t stream);
int64_t adnm_igate_res_bwd_ws_bytes(int64_t B, int64_t L, int64_t C);
int adnm_igate_res_bwd(const float* dy, const float* x, const float* res, int per_token, const float* gama, const float* enhance,
                       const float* threshold, float* dx, float* dres, float* dgama, float* denhance, float* dthreshold, void* ws,
                       int64_t ws_bytes, int64_t B, int64_t L, int64_t C, adnm_stream_t stream);


/* ---------------------------------------------------------------- EncoderToDecoder's pooled gating core (K12)
 * model_untils.py:767-787 of the reference, x = the block's normalised tokens (B, H, W, C) fp32 contiguous, C % 4 == 0:
 *   p_k = MaxPool_k(x) + AvgPool_k(x)      k = 0: (3,1) window, 1: (1,3), 2: (3,3); stride 1, count_include_pad
 *   c_k = conv_k(p_k)                      conv13pool (1,3) / conv31pool (3,1) / conv33pool (3,3), groups = C/4, with bias
 *   y_k = IntensityGate_k(ffd_k(x * GELU(c_k)))    ffd13 + act_func13 for k = 0 AND 1 (as the reference), ffd33 + act_func33 for k = 2
 *   out = gamma * (alpha1 y_0 + alpha2 y_1 + alpha3 y_2)
 * params: HOST array of 18 device pointers
 *   [0..5]  conv13pool.weight (C,4,1,3), .bias, conv31pool.weight (C,4,3,1), .bias, conv33pool.weight (C,4,3,3), .bias
 *   [6..9]  ffd13.weight (C), ffd13.bias, ffd33.weight, ffd33.bias          (1x1 depthwise = per-channel affine)
 *   [10..13] act_func13.enhance, .threshold, act_func33.enhance, .threshold  (scalars)
 *   [14..17] alpha1, alpha2, alpha3 (scalars), gamma (C)
 * pooled, conv: (3, B, H, W, C) each, written by fwd and handed back to bwd.
 * dparams (OVERWRITTEN), adnm_skipgate_grad_floats(C) floats:
 *   [d w0 12C | d w1 12C | d w2 36C | d gamma | d ffd13.w | d ffd13.b | d ffd33.w | d ffd33.b | d b0 | d b1 | d b2 (C each) |
 *    d alpha1..3, d enh13, d thr13, d enh33, d thr33, pad]
 * Inside a launch group (adnm_group_*) both calls record their launches, fwd at positions 0 (pools) and 1 (branches), bwd at 0 (pointwise
 * gate), 1 (grouped conv, both gradients) and 2 (pools); the device pointers behind params are read at the call, everything they point to
 * (and pooled, conv, out, dx, dparams, ws) must stay alive until adnm_group_launch.  bwd's folds wait in a bound fold queue; without one an
 * open group records them behind every position. */
int adnm_skipgate_fwd(const float* x, const float* const* params, float* pooled, float* conv, float* out, int64_t B, int64_t H, int64_t W,
                      int64_t C, adnm_stream_t stream);
int64_t adnm_skipgate_grad_floats(int64_t C);
int64_t adnm_skipgate_bwd_ws_bytes(int64_t B, int64_t H, int64_t W, int64_t C);
int adnm_skipgate_bwd(const float* dout, const float* x, const float* const* params, const float* pooled, const float* conv, float* dx,
                      float* dparams, void* ws, int64_t ws_bytes, int64_t B, int64_t H, int64_t W, int64_t C, adnm_stream_t stream);

/* ---------------------------------------------------------------- soft-max attention with 4-wide heads (K16)
 * StandardAttention.forward (models/ADNssd.py:38-46 of the reference) between to_qkv and to_out:
 *   out[b,l,h*4+d] = sum_j softmax_j(scale * q[b,h,l,:] . k[b,h,j,:]) v[b,h,j,d],   heads = inner/4, L <= 2048
 * qkv: (B, L, 3*inner) fp32 contiguous = to_qkv's output as it is ([q | k | v], head h at columns h*4..h*4+3 of each third);
 * out: (B, L, inner); lse: (B, heads, L) log-sum-exp of the scaled scores, saved for backward.  No (L, L) tensor is
 * materialised.  bwd: dqkv (B, L, 3*inner) OVERWRITTEN. */
int adnm_attn4_fwd(const float* qkv, float* out, float* lse, int64_t B, int64_t L, int64_t heads, float scale, adnm_stream_t stream);
int adnm_attn4_bwd(const float* dout, const float* qkv, const float* out, const float* lse, float* dqkv, int64_t B, int64_t L, int64_t heads,
                   float scale, adnm_stream_t stream);

/* ---------------------------------------------------------------- Channel_Att_Bridge's Conv1d (K15; the pooling itself: adnm_bridge_pool_*)
 * model_untils.py:592 of the reference.  conv1d3: nn.Conv1d(1,1,3,padding=1) over the concatenated channel axis
 * of (B,n) (get_all_att); bwd writes dx and dwb = [dw0, dw1, dw2, dbias] (OVERWRITTEN). */
/* Elementwise product y = a * b of two (M, C) fp32 token matrices with row strides lda / ldb (y, da, db contiguous): VSSD's output gate
 * LayerNorm(y) * z (Vssd.py:280-281).  4 | C. */
int adnm_emul_fwd(const float* a, int64_t lda, const float* b, int64_t ldb, float* y, int64_t M, int64_t C, adnm_stream_t stream);
int adnm_emul_bwd(const float* dy, const float* a, int64_t lda, const float* b, int64_t ldb, float* da, float* db, int64_t M, int64_t C,
                  adnm_stream_t stream);
/* Channel pad / crop of a token matrix (row stride ldx): y[m, c] = x[m, c] for c < min(Cin, Cout), 0 for Cin <= c < Cout; y:(M, Cout)
 * contiguous.  The 5-frame input stage (PatchEmbed.conv1: WTConv2d on 5 channels, model_untils.py:259) runs on 8 channels; pad and crop
 * are each other's backward. */
int adnm_chancopy(const float* x, int64_t ldx, int64_t Cin, float* y, int64_t Cout, int64_t M, adnm_stream_t stream);
int adnm_conv1d3_fwd(const float* x, const float* w, const float* bias, float* y, int64_t B, int64_t n, adnm_stream_t stream);
int adnm_conv1d3_bwd(const float* dy, const float* x, const float* w, float* dx, float* dwb, int64_t B, int64_t n, adnm_stream_t stream);
/* The heads of Channel_Att_Bridge, grouped (model_untils.py:744-750 the seven nn.Linear(sum C, C_i), :594-613 sigmoid1 = IntensityGate):
 *   z_i[b, :] = att[b, :] . W_i^T + bias_i,   gate_i = silu(enhance * (z_i - threshold)),   att:(B, S) fp32 contiguous, W_i:(C_i, S).
 * W / bias / z / y / dy / dW / dbias: HOST arrays of nheads device pointers; C: HOST array of the head widths.  1 <= B <= 8, 4 | S <= 3072.
 * One forward launch for all heads (a wave per output feature); backward = one launch (weight-gradient rows written as they are formed,
 * dbias, per-workgroup partials of datt / denhance / dthreshold) + one fold that is never deferred (datt is read next).
 * All outputs OVERWRITTEN; dbias may be NULL (or hold NULL entries). */
int adnm_bridge_heads_fwd(const float* att, const float* const* W, const float* const* bias, const int64_t* C, int nheads,
                          const float* enhance, const float* threshold, float* const* z, float* const* y, int64_t B, int64_t S,
                          adnm_stream_t stream);
int64_t adnm_bridge_heads_bwd_ws_bytes(int64_t total, int64_t B, int64_t S);
int adnm_bridge_heads_bwd(const float* att, const float* const* W, const int64_t* C, int nheads, const float* enhance,
                          const float* threshold, const float* const* z, const float* const* dy, float* datt, float* const* dW,
                          float* const* dbias, float* denhance, float* dthreshold, void* ws, int64_t ws_bytes, int64_t B, int64_t S,
                          adnm_stream_t stream);

/* The bridge's global average pools, grouped (Channel_Att_Bridge.forward, model_untils.py:570-590: AdaptiveAvgPool2d(1) of each skip, then
 * torch.cat along the channels): ONE launch + one fold for all n <= 8 skips.  x[k]: (B, L[k], C[k]) contiguous fp32 tokens, 4 | C[k];
 * att: (B, S = sum C[k]) OVERWRITTEN, skip k at columns [sum_{j<k} C[j], ...).  bwd: dx[k] = dxa[k] (or 0 when NULL) + datt[:, cols of k] / L[k]
 * broadcast over the tokens, one launch for all skips (dx[k] NULL skips skip k). */
int64_t adnm_bridge_pool_ws_bytes(int64_t B, int64_t S);
int adnm_bridge_pool_fwd(int64_t n, const float* const* x, const int64_t* L, const int64_t* C, float* att, void* ws, int64_t ws_bytes, int64_t B,
                         adnm_stream_t stream);
int adnm_bridge_pool_bwd(int64_t n, const float* const* dxa, const float* datt, const int64_t* L, const int64_t* C, float* const* dx, int64_t B,
                         adnm_stream_t stream);

/* out[c] = sum_r x[r*n + c] for a contiguous (rows, n) fp32 matrix — nn.Linear's bias gradient (autograd's sum over the token
 * rows) when the weight gradient is computed elsewhere (the transposed conv's).  Deterministic (fixed tree), OVERWRITES out; matrices
 * of >= 2048 rows are summed in two stages through `ws` (adnm_colsum_ws_bytes), which must stay alive until a bound fold queue is
 * flushed. */
int64_t adnm_colsum_ws_bytes(int64_t rows, int64_t n);
int adnm_colsum(const float* x, float* out, int64_t rows, int64_t n, void* ws, int64_t ws_bytes, adnm_stream_t stream);

/* ---------------------------------------------------------------- short GEMMs of the deep stages (K6b, MFMA)
 * nn.Linear with M <= 2^20 token rows (M x features < 2^31) and up to 16384 features: Mamba2.in_proj/out_proj (ADNssd.py:309,461),
 * FeedForward.project_in/out (model_untils.py:193,196), Mlp (:64,67), ConvFFD (:217,221), Block.out_proj (ADNMUNet.py:163),
 * StandardAttention.to_qkv/to_out (ADNssd.py:33-34), Channel_Att_Bridge.att* (model_untils.py:744-750).  fp32, row-major:
 *   ADNM_SKGEMM_NT: c[M,N] = a[M,K] . b[N,K]^T (+ bias[N])           forward          K % 4 == 0
 *   ADNM_SKGEMM_NN: c[M,K] = a[M,N] . b[N,K]                         input gradient   N % 4 == 0, K % 4 == 0
 *   ADNM_SKGEMM_TN: c[N,K] = a[M,N]^T . b[M,K]; dbias[N] = sum_m a   weight gradient  N % 4 == 0, K % 4 == 0
 * lda / ldb / ldc: row strides in elements (multiples of 4); bias only with NT, dbias only with TN; c / dbias OVERWRITTEN.
 * prec / q: the precision ladder and the call site's quantisation record (see ADNM_MFMA_*); a = the "first operand", b = the weight.
 * TN (the weight gradient) runs on bf16 operands in the fp8 modes.
 * b_dtype (NT / NN): storage of the weight operand b — ADNM_B_F32 (the fp32 master values, rounded / scaled on the way into the MFMA),
 *   ADNM_B_BF16 (its bf16 shadow, prec ADNM_MFMA_BF16 only) or ADNM_B_FP8 (its per-tensor scaled OCP e4m3 shadow, the fp8 modes only;
 *   b_scale = device pointer to the scale the shadow was made with: value = e4m3 / *b_scale; q's scale_b / amax_b are then unused).
 *   The shadows are written by the optimiser pass (adnm_adamw_step) or the parameter-prep kernels; ldb counts ELEMENTS in every case.
 *   A narrow weight halves / quarters the bytes of the weight-streaming shapes and gives bit for bit the result of the fp32 operand
 *   rounded the same way.
 * Workspace (adnm_skgemm_ws_bytes; 16 = the shape is not split): a reduction that would leave CUs idle is split over workgroups.
 *   The query covers the plan of either precision; a launch that keeps its slabs / partials in ws is refused (ADNM_EWORKSPACE) unless
 *   ws_bytes is at least what the query names, whatever its own plan would touch.
 *   TN: ws holds fp32 partials for the shared fold — ordinary device memory.
 *   NT / NN: the slabs are combined INSIDE the launch (arrival counters; the last workgroup of a tile adds the slabs in slice order:
 *     bitwise reproducible).  ws = [arrival counters: one int per output tile, rounded up to 256 B | slabs], 256-byte aligned ordinary
 *     device memory; the counters must be ZERO when the launch starts and are zero again when it ends, so one workspace serves every
 *     launch of a stream (launches on a stream are ordered) but must not be shared by launches that can run concurrently (another
 *     stream, another captured graph replayed beside this one).  slabs_uc (optional, NULL = none): uncached device memory
 *     (adnm_uncached_alloc) of at least the slab part; the slabs then live there — a completed slab store is at the device-wide
 *     coherence point, so the arrival ticket needs no agent-scope release / acquire (= no per-workgroup write-back / invalidate of an
 *     XCD's L2) — and ws only has to hold the counters (adnm_skgemm_counter_bytes).  Same sharing rule.  Both protocols give bitwise
 *     identical results.
 * adnm_uncached_alloc: `bytes` of zero-filled uncached device memory on the current device (hipExtMallocWithFlags +
 * hipDeviceMallocUncached), NULL on failure; a host-side setup call (it synchronises; not under stream capture). */
#define ADNM_SKGEMM_NT 0
#define ADNM_SKGEMM_NN 1
#define ADNM_SKGEMM_TN 2
int adnm_skgemm_supported(int op, int64_t M, int64_t N, int64_t K);
int64_t adnm_skgemm_ws_bytes(int op, int64_t M, int64_t N, int64_t K);   /* counters + slabs (NT / NN), partials (TN) */
int adnm_skgemm(int op, const float* a, int64_t lda, const void* b, int64_t ldb, int b_dtype, const float* b_scale, const float* bias, float* c,
                int64_t ldc, float* dbias, void* ws, int64_t ws_bytes, void* slabs_uc, int64_t slabs_uc_bytes, int64_t M, int64_t N, int64_t K,
                int prec, float* q, adnm_stream_t stream);
int64_t adnm_skgemm_counter_bytes(int op, int64_t M, int64_t N, int64_t K);
/* The plan adnm_skgemm launches with for this op, shape and precision (bf16 != 0: every narrow mode) — a read-only host query for tests
 * and tools, answered by the planner the launch itself calls.  out[10] = {kernel (0 register-streaming, 1 LDS-tiled), tm, tn, kc (wave
 * tile 16 tm x 16 tn, 16 kc reduction steps per chunk), wpt (waves sharing a tile), nbs (reduction slices over workgroups), cpw (chunks
 * per wave), nchunks, combine (1: the slabs are summed inside the launch, 0: by the fold), source (0 a row of the measured table, 1 the
 * rules, 2 a forced plan)}.  The LDS-tiled kernel reports {1, 4, 4, 2, 1, slices after its own clamp, step tiles per slice, step
 * tiles, ...}.  Every chunk has an owner (nbs * wpt * cpw >= nchunks) and no slice is empty ((nbs - 1) * wpt * cpw < nchunks).
 * direct != 0: the output takes no partials — adnm_skgemm plans so for op TN when ldc != K, never for NT / NN.  For op TN the answer
 * depends, as the launch does, on whether the calling thread has a leaf queue (and a fold queue) bound.  ADNM_EINVAL for a shape
 * adnm_skgemm_supported refuses. */
int adnm_skgemm_plan(int op, int64_t M, int64_t N, int64_t K, int bf16, int direct, int* out);
void* adnm_uncached_alloc(int64_t bytes);
int adnm_uncached_free(void* ptr);

/* ---------------------------------------------------------------- enRainfallLoss (K14)
 * models/loss.py:30-57 of the reference (train_untils.py:43 builds it with omega_t 0.57, alpha 0.25, gamma 0):
 * loss (1 float) and grad = d loss / d pred (n floats) in one pass over contiguous fp32 pred / target. */
int64_t adnm_rainloss_ws_bytes(int64_t n);
int adnm_rainloss(const float* pred, const float* target, float* loss, float* grad, void* ws, int64_t ws_bytes, int64_t n, float omega_t,
                  float alpha, float gamma, adnm_stream_t stream);

/* ---------------------------------------------------------------- head merge (K13)
 * y = cat((a1*x, a2*r), -1) [+ cat((a3*f, a4*f), -1)] — Block / Attention merge (ADNMUNet.py:124-131, :214-221) and WTLayer's
 * (model_untils.py:398-400).  x, r, f: (M,d) with row strides; f may be NULL; a_k: device scalars (NULL = 1); y: (M,2d)
 * contiguous.  bwd: dx, dr, df (M,d) contiguous (NULL skips), da[4] OVERWRITTEN (da[2..3] = 0 without f). */
int adnm_catmix_fwd(const void* x, int64_t ldx, const void* r, int64_t ldr, const void* f, int64_t ldf, const float* a1, const float* a2,
                    const float* a3, const float* a4, void* y, int64_t M, int64_t d, int dtype, adnm_stream_t stream);
int64_t adnm_catmix_bwd_ws_bytes(int64_t M, int64_t d);
int adnm_catmix_bwd(const void* dy, int64_t lddy, const void* x, int64_t ldx, const void* r, int64_t ldr, const void* f, int64_t ldf,
                    const float* a1, const float* a2, const float* a3, const float* a4, void* dx, void* dr, void* df, float* da, void* ws,
                    int64_t ws_bytes, int64_t M, int64_t d, int dtype, adnm_stream_t stream);

/* ---------------------------------------------------------------- fused scalar / channel-affine mixes
 * y[m,c] = gamma[c] * ( s0*x0[m,c] + s1*x1[m,c] + s2*x2[m,c] )      x1,x2 optional (NULL), s_k NULL = 1, gamma NULL = 1
 * replaces the broadcast mul/add chains around the learnable scalars of Block.forward (ADNMUNet.py:152,158,161),
 * Attention.forward (:226,232,234), WTLayer / PatchEmbed / OutProj (model_untils.py:306-310,418-421,881-883) and
 * EncoderToDecoder (:785-787).  bwd: dx_k = s_k*gamma*dy (NULL skips), ds_k = sum dy*gamma*x_k, dgamma[c] = sum_m dy*mix;
 * ds_k / dgamma are OVERWRITTEN (NULL skips).  C % 4 == 0, C <= 2048. */
int adnm_lincomb_fwd(const void* x0, int64_t ld0, const void* x1, int64_t ld1, const void* x2, int64_t ld2,
                     const float* s0, const float* s1, const float* s2, const float* gamma, void* y, int64_t ldy,
                     int64_t M, int64_t C, int dtype, adnm_stream_t stream);
int64_t adnm_lincomb_bwd_ws_bytes(int64_t M, int64_t C);
int adnm_lincomb_bwd(const void* dy, int64_t lddy, const void* x0, int64_t ld0, const void* x1, int64_t ld1,
                     const void* x2, int64_t ld2, const float* s0, const float* s1, const float* s2,
                     const float* gamma, void* dx0, int64_t lddx0, void* dx1, int64_t lddx1, void* dx2, int64_t lddx2,
                     float* ds0, float* ds1, float* ds2, float* dgamma, void* ws, int64_t ws_bytes, int64_t M, int64_t C,
                     int dtype, adnm_stream_t stream);

/* ---------------------------------------------------------------- residual mix + the next pre-norm, one pass each way
 * mix = gamma * (s0*x0 + s1*x1)  (adnm_lincomb_fwd, bitwise)   and   xn = scale * ((mix - mu) * rstd * w + b) + shift  (adnm_rownorm_fwd)
 * — Block.forward's `x = beta1*x + beta2*mixer(..); xn = scale2*norm2(x) + shift2` and the pair around the FFN (ADNMUNet.py:149-158), the
 * same pairs in Attention.forward (:226-232).  fp32 rows, d % 4 == 0, d <= 1024.  bwd: dyn = d xn, dres = the gradient arriving on mix through
 * the residual path (NULL: none); writes dx0 / dx1 (NULL skips) and OVERWRITES ds0, ds1, dgamma, dw, db, dscale, dshift (NULL skips); an
 * accumulate mask announced with adnm_foldq_accumulate_next applies to {dgamma, ds0, ds1} as for adnm_lincomb_bwd. */
int adnm_mixnorm_fwd(const float* x0, int64_t ld0, const float* x1, int64_t ld1, const float* s0, const float* s1, const float* gamma,
                     const float* w, const float* b, const float* scale, const float* shift, float* ymix, int64_t ldm, float* yn,
                     int64_t ldn, float* mu, float* rstd, int64_t M, int64_t d, float eps, int subtract_mean, adnm_stream_t stream);
int64_t adnm_mixnorm_bwd_ws_bytes(int64_t M, int64_t d);
int adnm_mixnorm_bwd(const float* dyn, int64_t lddyn, const float* dres, int64_t lddres, const float* x0, int64_t ld0, const float* x1,
                     int64_t ld1, const float* s0, const float* s1, const float* gamma, const float* w, const float* b, const float* scale,
                     const float* mu, const float* rstd, float* dx0, int64_t lddx0, float* dx1, int64_t lddx1, float* ds0, float* ds1,
                     float* dgamma, float* dw, float* db, float* dscale, float* dshift, void* ws, int64_t ws_bytes, int64_t M, int64_t d,
                     int subtract_mean, adnm_stream_t stream);

/* ---------------------------------------------------------------- fused step glue on flat fp32 buffers (§8f rank 1)
 * clip_grad_norm_(max_norm) (train.py:140) + AdamW (train_untils.py:35-42) over n parameters laid out flat:
 *   state[1] = sum g^2;  coef = min(1, max_norm / (sqrt(state[1]) + 1e-6))  (max_norm <= 0: no clipping)
 *   state[0] += 1 (step);  p *= 1 - lr*wd;  m = lerp(m, coef*g, 1-beta1);  v = beta2*v + (1-beta2)(coef*g)^2
 *   p -= lr/(1-beta1^step) * m / (sqrt(v)/sqrt(1-beta2^step) + eps)        — torch.optim.AdamW's exact update order.
 * state: 4 device floats [step, sumsq, bc1, sqrt(bc2)], zero-initialised by the caller; n % 4 == 0.
 * shadow (optional, NULL = none): the narrow copy of the updated parameters the weight-streaming GEMMs read (adnm_skgemm b_dtype), written
 *   in the same pass — the values are in registers anyway, so the step pays 2 (bf16) or 1 (fp8) more bytes per parameter and the two
 *   passes that re-read the 72 M parameters every step (forward, input gradients) read a half / a quarter of the bytes:
 *   shadow_dtype ADNM_B_BF16: shadow[i] = bf16(p[i]), n uint16;
 *   shadow_dtype ADNM_B_FP8:  shadow[i] = e4m3(clamp(p[i] * scale_b(record of i's tensor))), n bytes.  Tensors = the segments of the flat
 *     buffer: seg_end[s] = END of segment s in units of 4 elements (ascending; tensors are 16-byte aligned in the flat layout),
 *     seg_rec[s] = row of its 8-float quantisation record in wtab (the layout of `q`; only scale_b / amax_b / fmax_b / record are used)
 *     or < 0 for a tensor no GEMM reads (its shadow bytes are unspecified).  While a record's `record` flag is set the pass collects
 *     max |p| of the UPDATED values into amax_b; adnm_quant_update (run over wtab BEFORE this pass in a step) turns it into the next
 *     scale_b, with which this pass writes the shadow and the next step's GEMMs read it: shadow and scale never disagree.
 * hyper (optional, NULL = use the arguments): two device floats {lr, max_norm} read by the kernels INSTEAD of the by-value arguments, so that
 *   a launch captured in a hipGraph (the tail graph of a multi-GPU step) follows the host's learning-rate schedule and adaptive clip
 *   threshold (train.py:122-130) — the host rewrites the two floats when they change.
 * adnm_shadow_refresh: the shadow alone from the parameters as they are (after they moved into the flat buffer, after a checkpoint load);
 *   shadow = NULL (fp8) with collect != 0: only collect max |p| (the first calibration). */
int64_t adnm_adamw_ws_bytes(void);
int adnm_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float* state, float lr, float beta1,
                    float beta2, float eps, float weight_decay, float max_norm, void* ws, int64_t ws_bytes, void* shadow, int shadow_dtype,
                    const int* seg_end, const int* seg_rec, int64_t nseg, float* wtab, const float* hyper, adnm_stream_t stream);
int adnm_shadow_refresh(const float* p, int64_t n, void* shadow, int shadow_dtype, const int* seg_end, const int* seg_rec, int64_t nseg,
                        float* wtab, int collect, adnm_stream_t stream);

/* The monitored step: train.py:136-153 reads original_norm.item() and loss.item() after every step (for the adaptive clip threshold of
 * train.py:122-130, the clip rate and the summed loss it prints); here those sums stay on the device and the host reads them once per
 * epoch.  The same block carries the decision every mixed-precision trainer makes: a step whose gradient is not finite is SKIPPED.
 * stats: 72 bytes of device memory, 8-byte aligned, zero-initialised by the caller:
 *   double [0] applied steps   [1] skipped steps   [2] sum of the pre-clip norms of the applied steps   [3] their maximum
 *          [4] norm of the last step, applied or skipped (inf / nan after a skipped one)
 *          [5] applied steps with max_norm > 0 && norm > max_norm (train.py:142's strict comparison, not the + 1e-6 of the coefficient)
 *          [6] sum of the finite losses   [7] number of non-finite losses
 *   int    [16] skip flag of the step in flight (byte offset 64);  float [17] the guard's sum of squares (byte offset 68).
 * adnm_step_guard, after the gradient is final (bf16 wire cast back, adnm_grad_accum_final) and before the fp8 table update:
 *   sum g^2 by adnm_adamw_step's own two launches (bit-identical norm), left in the block; skip = exponent bits of the sum all ones, i.e.
 *   a gradient with an Inf or a NaN — or a FINITE gradient whose fp32 sum of squares overflows, which counts as non-finite as well (its
 *   norm cannot be formed; the clip coefficient would be 0).  An applied step moves the sum to state[1]; a skipped one leaves all four
 *   floats of state as they were (state[1] then still holds the last applied step's sum).  Then the counters above, norm = sqrtf(sum).  max_norm comes
 *   from hyper[1] when hyper != NULL, exactly as the AdamW kernels read it.  ws: adnm_adamw_ws_bytes().
 * adnm_adamw_step_guarded: adnm_adamw_step WITHOUT its norm pass (state[1] is the guard's), every kernel checking the flag with one
 *   uniform load at entry.  Flag set: state[0], state[2], state[3], p, m, v, the shadow and every amax_b stay untouched.  Flag clear:
 *   bit-identical to adnm_adamw_step.
 * adnm_loss_stat (train.py:145): stats[6] += *loss when finite, else stats[7] += 1; one lane. */
int adnm_step_guard(const float* g, int64_t n, float* state, float max_norm, const float* hyper, void* ws, int64_t ws_bytes, void* stats,
                    adnm_stream_t stream);
int adnm_adamw_step_guarded(float* p, const float* g, float* m, float* v, int64_t n, float* state, float lr, float beta1, float beta2,
                            float eps, float weight_decay, float max_norm, void* shadow, int shadow_dtype, const int* seg_end,
                            const int* seg_rec, int64_t nseg, float* wtab, const float* hyper, const void* stats, adnm_stream_t stream);
int adnm_loss_stat(const float* loss, void* stats, adnm_stream_t stream);

/* ---------------------------------------------------------------- dense 3x3 'same' convolution, NHWC, on MFMA (K5)
 * nn.Conv2d(k=3, s=1, p=1) [+ bias] [+ GELU] of the U-Net conv stack: PatchEmbed.conv2 (model_untils.py:259-273), WTLayer.conv
 * (:376-387), OutProj.conv[0] / conv2 (:818-849).  Implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32).
 *   in:(B*H*W, K) pixel rows (row stride ldin), out:(B*H*W, N) (ldo); K = Cin, N = Cout (any sizes; 16-byte paths need % 4).
 *   w element (n, ky, kx, k) at w[n*ws_n + (ky*3+kx)*ws_tap + k*ws_k]: nn.Conv2d's own (Cout,Cin,3,3) layout is
 *   (ws_n, ws_tap, ws_k) = (9K, 1, 9), the channels-last one (Cout,3,3,Cin) is (9K, K, 1) — both are read in place.
 *   act (fwd only): ADNM_ACT_NONE | ADNM_ACT_GELU applied in the epilogue; pre (optional, row stride ldpre) receives conv + bias BEFORE
 *   the activation — the tensor autograd would have saved for the reference's separate GELU.
 *   dgrad / wgrad: dout (row stride lddo) is the gradient with respect to the conv's PRE-activation: the output gradient itself without
 *   an activation, else dpre = dy * act'(pre), which the caller forms once with adnm_act_bwd — the two kernels read a plain operand.
 *   dgrad: din = conv^T(dout);  wgrad: dw[n][tap][k] contiguous (= the channels-last weight layout), dbias optional; both OVERWRITE.
 *   Workspaces: split-K partials of the deep maps (fwd / dgrad: adnm_conv3_ws_bytes with the (K, N) of THAT launch's reduction /
 *   output), per-wave partial rows (wgrad). */
int64_t adnm_conv3_ws_bytes(int64_t B, int64_t H, int64_t W, int64_t K, int64_t N);
int adnm_conv3_fwd(const float* in, int64_t ldin, const float* w, int64_t ws_n, int64_t ws_tap, int64_t ws_k, const float* bias,
                   float* out, int64_t ldo, float* pre, int64_t ldpre, void* ws, int64_t ws_bytes, int64_t B, int64_t H, int64_t W,
                   int64_t K, int64_t N, int act, int prec, float* q, adnm_stream_t stream);
int adnm_conv3_dgrad(const float* dout, int64_t lddo, const float* w, int64_t ws_n, int64_t ws_tap, int64_t ws_k, float* din,
                     int64_t lddin, void* ws, int64_t ws_bytes, int64_t B, int64_t H, int64_t W, int64_t K, int64_t N, int prec,
                     float* q, adnm_stream_t stream);
int64_t adnm_conv3_wgrad_ws_bytes(int64_t B, int64_t H, int64_t W, int64_t K, int64_t N);
int adnm_conv3_wgrad(const float* dout, int64_t lddo, const float* in, int64_t ldin, float* dw, float* dbias, void* ws,
                     int64_t ws_bytes, int64_t B, int64_t H, int64_t W, int64_t K, int64_t N, int prec, adnm_stream_t stream);

/* ---------------------------------------------------------------- stride-2 transposed conv of UpSample (K9)
 * nn.ConvTranspose2d(C, C, k=3, s=2, p=1, output_padding=1) (model_untils.py:120-158,490-520) = one GEMM over the input pixels
 * (cols[B*H*W, 9C] = X . Wf, adnm_skgemm op NN on the weight as it lies) + these two data-movement kernels:
 *   col2im: out[b, oy, ox, :] = bias + the taps of cols whose parity matches (oy, ox) (1, 2, 2 or 4 of them: the 4 phases);
 *   im2col: dcols[(b,iy,ix), tap, :] = dout[b, 2iy-1+ky, 2ix-1+kx, :] (0 outside): then dX = dcols . Wf^T (op NT), dWf = X^T . dcols (op TN).
 * Column (tap, c) of a cols row sits at tap*col_tap_stride + c*col_c_stride: (C, 1) for the (Cin, 3, 3, Cout) weight order,
 * (1, 9) for nn.ConvTranspose2d's own (Cin, Cout, 3, 3).  out / dout: (B*2H*2W, C) pixel rows. */
int adnm_convt_col2im(const float* cols, int64_t ldc, int64_t col_tap_stride, int64_t col_c_stride, const float* bias, float* out,
                      int64_t ldo, int64_t B, int64_t H, int64_t W, int64_t C, adnm_stream_t stream);
int adnm_convt_im2col(const float* dout, int64_t lddo, float* dcols, int64_t ldc, int64_t col_tap_stride, int64_t col_c_stride,
                      int64_t B, int64_t H, int64_t W, int64_t C, adnm_stream_t stream);

/* ---------------------------------------------------------------- the data formats either side of the path
 * adnm_radar_ingest: datasets/Shanghai.py:52-59,121 — uint8 frames (frames, H0, W0), value * mul (1/255), bilinear resize to (S, S)
 *   (align_corners=False, no antialias = torchvision's tensor Resize) -> fp32 (frames, S, S).  src_u8 is a DEVICE pointer (the
 *   caller moves the bytes, e.g. by an async copy from pinned host memory).
 * adnm_eval_counts: datasets/Shanghai_metrics.py:49-152 — per frame [TP, FN, FP, TN] at each threshold on
 *   uint16(clip(x,0,1) * value_scale) fields (truth = "obs", pred = "sim") and sum |d|, sum d^2 of the scaled clipped float fields.
 *   thresholds_host: nthr <= 8 floats in HOST memory (they become kernel arguments).  out: (frames, 4*nthr + 2) fp32, OVERWRITTEN. */
int adnm_radar_ingest(const void* src_u8, float* dst, int64_t frames, int64_t H0, int64_t W0, int64_t S, float mul, adnm_stream_t stream);
/* adnm_batch_fetch: the DataLoader's collate + copy (train.py:44-57,132-134) for a split that lives on the device.  store: (n_samples, T, hw)
 *   fp32 contiguous; order: order_len int32 sample indices, both in DEVICE memory (the kernel reads the indices: none passes through the
 *   host).  For b < B, s = order[pos + b]:  x[b] = store[s, :T_in] as (B, T_in, hw),  tgt[b] = store[s, T_in:] as (B, T - T_in, hw),
 *   both contiguous, a pure copy (bit exact).  One launch, gridDim.y = B.
 *   An index outside [0, n_samples) is NOT dereferenced: that sample's x and tgt rows are filled with quiet NaNs (0x7fc00000) and the
 *   launch succeeds, so a bad order shows as a non-finite loss (which a monitored step skips and counts), never as a stray read.
 *   Refused before any launch (ADNM_EINVAL): a null pointer; B outside [1, 65535] (the grid's second dimension); T_in < 1 or T_in >= T;
 *   hw < 1 (or hw, T >= 2^31); pos < 0 or pos + B > order_len; n_samples or order_len outside [1, 2^31); a pointer that is not 4-byte
 *   aligned.  Alignment beyond that is the entry point's business: with T*hw and T_in*hw multiples of 4 and store, x and tgt 16-byte
 *   aligned the copy moves 16 bytes per access, otherwise (an odd frame side, x or tgt a 4-byte aligned slice of a larger buffer) it
 *   moves floats one by one with the SAME result: such a call is served, not refused. */
int adnm_batch_fetch(const float* store, int64_t n_samples, int64_t T, int64_t hw, const int32_t* order, int64_t order_len, int64_t pos,
                     float* x, float* tgt, int64_t B, int64_t T_in, adnm_stream_t stream);
/* adnm_batch_fetch_aug: adnm_batch_fetch with the label-preserving augmentations of gridded fields done in the copy.  The reference has
 *   none: its only transform is the resize (datasets/Shanghai.py:40-59), so this entry point adds to what train.py can do and a feed
 *   without augmentation keeps launching adnm_batch_fetch.  store: (n_samples, T, Hs, Ws) fp32 contiguous; order, aug: order_len int32
 *   each, DEVICE memory, indexed by the position in the epoch (a word belongs to a position, not to a sample); x: (B, T_in, H, W),
 *   tgt: (B, T - T_in, H, W), contiguous.  The word a = aug[pos + b]:
 *     bit 0 flip left-right | bit 1 flip up-down | bit 2 transpose | bits 3-16 oy | bits 17-30 ox | bit 31 must be 0
 *   With s = order[pos + b], on every frame of the sample and as bit patterns (NaN payloads and -0.0 are copied, never recomputed):
 *     w = store[s, :, oy:oy+H, ox:ox+W];  bit 1: w = w.flip(-2);  bit 0: w = w.flip(-1);  bit 2: w = w.transpose(-1, -2)
 *     x[b], tgt[b] = w[:T_in], w[T_in:]
 *   input and target of a sample are therefore transformed identically.  One launch, gridDim.y = B, no workspace.
 *   NOT served, per sample: an index outside [0, n_samples); a word with bit 31 set; oy + H > Hs or ox + W > Ws; the transpose bit with
 *   H != W.  None of these is turned into an address: the sample's x and tgt rows are filled with quiet NaNs (adnm_batch_fetch's rule).
 *   Refused before any launch (ADNM_EINVAL): a null pointer or one that is not 4-byte aligned; B outside [1, 65535]; T_in outside
 *   [1, T); H, W, Hs or Ws outside [1, 16384); H > Hs or W > Ws; T*Hs*Ws >= 2^31; pos < 0 or pos + B > order_len; n_samples or
 *   order_len outside [1, 2^31).  Access width is the entry point's business and is chosen PER SAMPLE: without the transpose bit rows
 *   move as 16-byte pieces when W and Ws are multiples of 4, store, x and tgt are 16-byte aligned and the sample's ox is a multiple of
 *   4 (a reversed row swaps the components of each piece), else float by float; with it, through a 32 x 33 LDS tile, float by float
 *   and coalesced on both sides.  The result is the same on every path. */
int adnm_batch_fetch_aug(const float* store, int64_t n_samples, int64_t T, int64_t Hs, int64_t Ws, const int32_t* order, const int32_t* aug,
                         int64_t order_len, int64_t pos, float* x, float* tgt, int64_t B, int64_t T_in, int64_t H, int64_t W,
                         adnm_stream_t stream);
int64_t adnm_eval_counts_ws_bytes(int64_t frames, int64_t hw, int64_t nthr);
int adnm_eval_counts(const float* truth, const float* pred, float* out, const float* thresholds_host, int64_t nthr, float value_scale,
                     void* ws, int64_t ws_bytes, int64_t frames, int64_t hw, adnm_stream_t stream);
/* adnm_eval_ssim: SimplifiedEvaluator.cal_ssim (datasets/Shanghai_metrics.py:132-152) — out[frame] = SUM over the valid (H-10) x (W-10)
 * region of the SSIM map (11x11 Gaussian window, sigma 1.5, C1 = (0.01 s)^2, C2 = (0.03 s)^2, float64 arithmetic like the reference) of
 * the [0,1]-clipped fields times value_scale s; the caller divides by the region's area (the reference takes the mean).  truth, pred:
 * (frames, H, W) fp32 contiguous.  The window is the normalised sampled Gaussian cv2.getGaussianKernel(11, 1.5) documents. */
int64_t adnm_eval_ssim_ws_bytes(int64_t frames, int64_t H, int64_t W);
int adnm_eval_ssim(const float* truth, const float* pred, float* out, float value_scale, void* ws, int64_t ws_bytes, int64_t frames,
                   int64_t H, int64_t W, adnm_stream_t stream);

/* The validation half of an epoch (train.py:156-206: a forward-only pass, the loss per batch, the metrics) accumulated ON THE DEVICE:
 * a batch adds into a block the caller keeps for the whole epoch, and the host reads the block once.
 * block: adnm_valid_block_bytes(T, nthr) bytes of device memory, 8-byte aligned, zero-initialised by the caller, all double:
 *   double [0] sum of the finite batch losses (what train.py:163 accumulates)   [1] batches   [2] samples (frames / T per batch)
 *          [3] batches whose loss was not finite (they add nothing to [0]: adnm_loss_stat's rule)
 *   then a table (T, 4*nthr + 3), row t = frame index within a sample (frame f of a batch belongs to row f mod T):
 *          [4*k .. 4*k + 3] TP, FN, FP, TN at threshold k, summed over every sample so far (integers held in doubles: exact over a dataset)
 *          [4*nthr] sum |d|   [4*nthr + 1] sum d^2   of the value_scale'd [0,1]-clipped fields   [4*nthr + 2] sum of the SSIM maps' sums.
 * adnm_valid_accum: ONE pass over contiguous fp32 pred / target of shape (frames, hw), frames = B*T; two launches.  The counts and the two
 *   error sums are adnm_eval_counts' (the same device code: clip, scale, truncate, compare); the loss is enRainfallLoss on the UNCLIPPED
 *   values with adnm_rainloss' per-element expression (the same device function), value only — no gradient is formed or written.  Per
 *   workgroup fp32 partials go to ws; one workgroup folds them in double, in a fixed order (samples ascending), and updates the block:
 *   loss = (float)(sum e / (frames*hw)); finite: [0] += loss, else [3] += 1; [1] += 1; [2] += B; loss_out (optional device float, NULL
 *   skips) receives the fp32 batch loss.  Deterministic: the same calls on the same block give the same bits.  NaN / Inf data are inputs.
 * adnm_valid_ssim_accum: adnm_eval_ssim's kernel, then column 4*nthr + 2 of row f mod T += the frame's map sum.  H > 10 && W > 10.
 * Limits: frames <= 65535, hw < 2^24, 1 <= nthr <= 8 (adnm_eval_counts'), T >= 1, T | frames.  The *_bytes queries return -1 outside them. */
int64_t adnm_valid_block_bytes(int64_t T, int64_t nthr);
int64_t adnm_valid_accum_ws_bytes(int64_t frames, int64_t T, int64_t hw, int64_t nthr);
int adnm_valid_accum(const float* pred, const float* target, void* block, float* loss_out, const float* thresholds_host, int64_t nthr,
                     float value_scale, float omega_t, float alpha, float gamma, void* ws, int64_t ws_bytes, int64_t frames, int64_t T,
                     int64_t hw, adnm_stream_t stream);
int64_t adnm_valid_ssim_accum_ws_bytes(int64_t frames, int64_t T, int64_t H, int64_t W, int64_t nthr);
int adnm_valid_ssim_accum(const float* pred, const float* target, void* block, int64_t nthr, float value_scale, void* ws, int64_t ws_bytes,
                          int64_t frames, int64_t T, int64_t H, int64_t W, adnm_stream_t stream);

/* Neighbourhood ("pooled") contingency counts: TP / FN / FP / TN per WINDOW of a spatial max-pool instead of per pixel.  The reference
 * has no such score; the definitions are this project's and the yardstick is torch's max_pool2d on the quantised fields.
 *   quantisation  q(v) = floorf(fminf(fmaxf(v, 0), 1) * value_scale) in fp32: adnm_eval_counts' (the same device function).
 *   pool (s, d)   window size s, stride d, 1 <= d <= s <= 32; the windows of max_pool2d(kernel_size=s, stride=d, padding=0,
 *                 ceil_mode=False): ((H-s)/d + 1) x ((W-s)/d + 1), anchored top-left; pixels no window covers take no part.
 *   event         a window is an observed event at threshold k iff max q(target) over it >= thr_k, likewise the forecast; (1, 1) is
 *                 the point-wise count of adnm_eval_counts.
 * table: adnm_valid_pool_block_bytes(T, nthr, npool) bytes, 8-byte aligned, zeroed by the caller, all double, shape (T, npool, 4*nthr):
 *   [t][p][4k .. 4k+3] = TP, FN, FP, TN at threshold k of pool p for frame index t (frame f of a batch belongs to row f mod T), summed
 *   over every sample so far.  No header: batches and samples are in adnm_valid_accum's block.
 * adnm_valid_pool_accum ADDS a batch.  target: contiguous (frames, H, W) fp32.  Frame f = b*T + t of the forecast starts at
 *   pred + b*pred_sample_stride + t*pred_frame_stride (in elements; rows contiguous): a contiguous forecast is (T*H*W, H*W), a
 *   persistence forecast is (T_in*H*W, 0) with pred at the last input frame.  thresholds_host (nthr floats) and pools_host (2*npool
 *   int64: size, stride) are read on the host at call time and passed by value: the call can be captured.  With T = frames on a
 *   zeroed table it is the one-shot per-frame form.  Two launches: each frame tile (32 x 32 window origins plus the halo its windows
 *   reach into) is read once and serves every pool and threshold; integer per-workgroup partials go to ws, and one fold adds them in
 *   a fixed order (samples, then tiles, ascending).  No atomics, no floating-point sums: exact and bit-reproducible.  Aligned shapes
 *   (W, both strides multiples of 4, both bases 16-byte aligned) are read 16 bytes per access, all others float by float: same result.
 * Limits, refused before any launch (ADNM_EINVAL): a null pointer; pred / target not 4-byte or table not 8-byte aligned; npool outside
 *   1..4; a pool outside 1 <= d <= s <= 32 or with s > min(H, W); nthr outside 1..8; T < 1 or not dividing frames; frames > 65535;
 *   H or W >= 32768; H*W >= 2^24; pred_frame_stride neither 0 nor >= H*W; pred_sample_stride < 0.  The *_bytes queries return -1. */
int64_t adnm_valid_pool_block_bytes(int64_t T, int64_t nthr, int64_t npool);
int64_t adnm_valid_pool_accum_ws_bytes(int64_t frames, int64_t T, int64_t H, int64_t W, int64_t nthr, const int64_t* pools_host, int64_t npool);
int adnm_valid_pool_accum(const float* pred, int64_t pred_sample_stride, int64_t pred_frame_stride, const float* target, void* table,
                          const float* thresholds_host, int64_t nthr, float value_scale, const int64_t* pools_host, int64_t npool, void* ws,
                          int64_t ws_bytes, int64_t frames, int64_t T, int64_t H, int64_t W, adnm_stream_t stream);

/* Fractions Skill Score (Roberts & Lean 2008) per scale, threshold and frame index, as three INTEGER sums.  The reference has no FSS;
 * the definitions are this project's and the yardstick is conv2d with an all-ones kernel on the threshold bit fields.
 *   quantisation  adnm_valid_pool_accum's (the same device functions): I_o = q(target) >= thr_k, I_f = q(forecast) >= thr_k.
 *   scale n       odd, 1 <= n <= 33.  c_o(y, x) = the number of I_o pixels in the n x n window CENTRED on (y, x), for every pixel of the
 *                 frame; pixels outside the frame count 0 (scipy.ndimage.uniform_filter(size=n, mode="constant", cval=0) times n^2:
 *                 pysteps' convention); c_f likewise.  A window larger than the frame is allowed: the padding defines it.
 *   sums          A = SUM c_o^2, F = SUM c_f^2, C = SUM c_o c_f over the H*W pixels.  FSS = 2C / (A + F) (the 1/n^4 cancel), NaN when
 *                 A + F = 0: the caller's division.  n = 1: A = TP + FN, F = TP + FP, C = TP of the point-wise counts.
 * table: adnm_valid_fss_block_bytes(T, nthr, nscale) bytes, 8-byte aligned, zeroed by the caller, all double, shape (T, nscale, 3*nthr):
 *   [t][i][3k .. 3k+2] = A, F, C at threshold k of scale i for frame index t (frame f of a batch belongs to row f mod T), summed over
 *   every sample so far.  No header.  Integers held in doubles: one 256 x 256 frame adds at most 65536 * 1089^2 = 7.8e10, so a row stays
 *   exact (< 2^53) for more than 10^5 samples of such frames.
 * adnm_valid_fss_accum ADDS a batch.  target, pred and the two strides: adnm_valid_pool_accum's meaning (persistence is (T_in*H*W, 0)).
 *   thresholds_host (nthr floats) and scales_host (nscale int64) are read on the host at call time and passed by value: the call can be
 *   captured.  With T = frames on a zeroed table it is the one-shot per-frame form.  Two launches: each 32 x 32 tile of window centres
 *   plus a halo of max(n)/2 pixels on all four sides is read once, as threshold bits, and serves every scale and threshold (row sums,
 *   then column sums); uint32 per-workgroup partials (a tile's is at most 1024 * 1089^2 < 2^32: why 33 is the limit) go to ws, and one
 *   fold adds them in a fixed order (samples, then tiles, ascending).  No atomics, no floating-point sums: exact and bit-reproducible.
 *   Aligned shapes (W, both strides multiples of 4, both bases 16-byte aligned) are read 16 bytes per access, all others float by float.
 * Limits, refused before any launch (ADNM_EINVAL): a null pointer; pred / target not 4-byte or table not 8-byte aligned; nscale outside
 *   1..4; a scale even or outside 1..33; a scale given twice; nthr outside 1..8; T < 1 or not dividing frames; frames > 65535; H or W
 *   outside [1, 32768); H*W >= 2^24; pred_frame_stride neither 0 nor >= H*W; pred_sample_stride < 0.  The *_bytes queries return -1. */
int64_t adnm_valid_fss_block_bytes(int64_t T, int64_t nthr, int64_t nscale);
int64_t adnm_valid_fss_accum_ws_bytes(int64_t frames, int64_t T, int64_t H, int64_t W, int64_t nthr, const int64_t* scales_host, int64_t nscale);
int adnm_valid_fss_accum(const float* pred, int64_t pred_sample_stride, int64_t pred_frame_stride, const float* target, void* table,
                         const float* thresholds_host, int64_t nthr, float value_scale, const int64_t* scales_host, int64_t nscale, void* ws,
                         int64_t ws_bytes, int64_t frames, int64_t T, int64_t H, int64_t W, adnm_stream_t stream);

/* Neighbourhood exceedance probability (Theis et al. 2005; Schwartz et al. 2010): the fraction of forecast pixels at or above a threshold
 * in the n x n window around a pixel, read as the probability of the event at that pixel, and the one sufficient statistic that verifies
 * it.  The reference has neither; the definitions are this project's and the yardstick is conv2d + np.bincount.
 *   event, scale  adnm_valid_fss_accum's: q(v) >= thr_k on the quantised field; n odd, 1 <= n <= 33, at most four scales, none twice.
 *   c_f(y, x)     FSS's window count of the FORECAST (zeros outside the frame: the denominator is always n^2); p = c_f / n^2.
 *   o(y, x)       the TARGET's event bit at the pixel itself (no neighbourhood on the observation side).
 *   statistic     N[t][k][scale][o][c] = the number of pixels of all frames f with f mod T = t that have o and c_f = c.
 * table: adnm_valid_nprob_block_bytes(T, nthr, scales_host, nscale) = 8 * T * nthr * S bytes, S = SUM over the scales of 2 * (n^2 + 1),
 *   8-byte aligned device memory, zeroed by the caller, all double, shape (T, nthr, S).  In a (t, k) row the scales stand in the order
 *   given; each scale is [o = 0: c = 0 .. n^2][o = 1: c = 0 .. n^2].  Integers held in doubles, each below frames * H*W < 2^53.
 * adnm_valid_nprob_accum ADDS a batch.  The arguments are adnm_valid_fss_accum's.  ONE launch, grid (tiles, frames), 32 x 32 tiles with
 *   FSS's staging (both the 16-byte and the float-by-float path) and running sums; thresholds are taken four at a time into a u32 LDS
 *   histogram (51.8 KB of static LDS with the image and the row counts), the lanes in bin (o = 0, c = 0) counted by ballot; after each
 *   scale the non-zero bins are added to the table as no-return double atomics.  Every addend is an integer: exact and the same bits on
 *   every run.  No workspace: adnm_valid_nprob_accum_ws_bytes is 0 for every accepted shape and ws may be NULL.
 * Limits, refused before any launch (ADNM_EINVAL): adnm_valid_fss_accum's.  The *_bytes queries return -1.
 * adnm_neighbour_prob is the product: field holds `frames` contiguous fp32 frames (4-byte aligned); out, fp32 (nthr, frames, H, W),
 *   out[k][f][y][x] = (float)c_f / (float)(n^2), ONE correctly rounded IEEE division (np.float32(c) / np.float32(n * n), bit for bit), for
 *   ONE scale and 1..8 thresholds.  Every element of out is written: 16 bytes per store where W % 4 == 0 and out is 16-byte aligned,
 *   float by float otherwise; loads likewise by field's alignment.  Limits (ADNM_EINVAL): a null pointer; field / out not 4-byte
 *   aligned; nthr outside 1..8; scale even or outside 1..33; frames outside 1..65535; H or W outside [1, 32768); H*W >= 2^24. */
int64_t adnm_valid_nprob_block_bytes(int64_t T, int64_t nthr, const int64_t* scales_host, int64_t nscale);
int64_t adnm_valid_nprob_accum_ws_bytes(int64_t frames, int64_t T, int64_t H, int64_t W, int64_t nthr, const int64_t* scales_host, int64_t nscale);
int adnm_valid_nprob_accum(const float* pred, int64_t pred_sample_stride, int64_t pred_frame_stride, const float* target, void* table,
                           const float* thresholds_host, int64_t nthr, float value_scale, const int64_t* scales_host, int64_t nscale, void* ws,
                           int64_t ws_bytes, int64_t frames, int64_t T, int64_t H, int64_t W, adnm_stream_t stream);
int adnm_neighbour_prob(const float* field, float* out, const float* thresholds_host, int64_t nthr, float value_scale, int64_t scale,
                        int64_t frames, int64_t H, int64_t W, adnm_stream_t stream);

/* Intensity-scale skill score (Casati, Ross & Stephenson 2004; the energy form of Casati 2010, as MET's wavelet-stat and pysteps'
 * intensity_scale report it): the binary error I_f - I_o of a threshold split into orthogonal 2-D Haar components of scale 1, 2, 4, ...
 * pixels, from ONE integer statistic.  The reference has none; the definitions are this project's and the yardstick is
 * reshape(P/s, s, P/s, s).sum((1, 3)) and, independently, an explicit orthonormal Haar matrix.
 *   event         adnm_valid_fss_accum's: I_o = q(target) >= thr_k, I_f = q(forecast) >= thr_k on the quantised fields.
 *   domain        1 <= H, W <= 1024.  P = the smallest power of two >= max(H, W), L = log2 P.  The frame sits at the origin of a P x P
 *                 domain; pixels outside the frame are no event in either field (FSS's zero padding).
 *   blocks        block (l, i, j), l = 0 .. L: rows i 2^l .. (i + 1) 2^l - 1, columns j 2^l .. (j + 1) 2^l - 1; o, f its numbers of target
 *                 and forecast events.
 *   sums          A_l = SUM o^2, F_l = SUM f^2, C_l = SUM o f over the blocks of level l.  l = 0: A = TP + FN, F = TP + FP, C = TP of the
 *                 point-wise counts; l = L: the squared event counts of the whole frame.  With D_l = A_l + F_l - 2 C_l and N = P^2 per
 *                 frame, the Haar component of scale 2^j of the error has MSE D_j / (4^j N) - D_(j+1) / (4^(j+1) N) (j < L) and
 *                 D_L / (4^L N) (the domain mean): validate.intensity_scale_entries, the caller's arithmetic.
 * table: adnm_valid_iscale_block_bytes(T, nthr, H, W) = 8 * T * (L + 1) * 3 * nthr bytes, 8-byte aligned, zeroed by the caller, all double,
 *   shape (T, L + 1, 3*nthr): the levels stand where the FSS table has its scales, a row is the FSS row: [t][l][3k .. 3k+2] = A, F, C at
 *   threshold k for frame index t (frame f of a batch belongs to row f mod T), summed over every sample so far.  No header.  Integers held
 *   in doubles: a single addend is at most (H*W)^2 <= 2^40, so a row stays exact (< 2^53) for 2^13 frames per frame index at 1024 x 1024
 *   and for 2^25 at 128 x 128.
 * adnm_valid_iscale_accum ADDS a batch.  target, pred and the two strides: adnm_valid_pool_accum's meaning (persistence is (T_in*H*W, 0)).
 *   thresholds_host (nthr floats) is read on the host at call time and passed by value: the call can be captured.  With T = frames on a
 *   zeroed table it is the one-shot per-frame form.  Two launches: each 32 x 32 tile is read once, with no halo, as threshold bits, and
 *   leaves uint32 partials of levels 0 .. min(L, 5) (a tile's A is at most 2^20) and its two counts per threshold in ws; one fold, a
 *   workgroup per (frame index, threshold), adds the partials over samples and tiles and builds levels 6 .. L from the tile counts in
 *   uint64.  No atomics, no floating-point sums, no workgroup waits for another: exact and bit-reproducible.  Aligned shapes (W, both
 *   strides multiples of 4, both bases 16-byte aligned) are read 16 bytes per access, all others float by float: same result.
 * Limits, refused before any launch (ADNM_EINVAL): a null pointer; pred / target not 4-byte, table or ws not 8-byte aligned; nthr outside
 *   1..8; T < 1 or not dividing frames; frames > 65535; H or W outside [1, 1024]; pred_frame_stride neither 0 nor >= H*W;
 *   pred_sample_stride < 0.  A short workspace is ADNM_EWORKSPACE.  The *_bytes queries return -1. */
int64_t adnm_valid_iscale_block_bytes(int64_t T, int64_t nthr, int64_t H, int64_t W);
int64_t adnm_valid_iscale_accum_ws_bytes(int64_t frames, int64_t T, int64_t H, int64_t W, int64_t nthr);
int adnm_valid_iscale_accum(const float* pred, int64_t pred_sample_stride, int64_t pred_frame_stride, const float* target, void* table,
                            const float* thresholds_host, int64_t nthr, float value_scale, void* ws, int64_t ws_bytes, int64_t frames,
                            int64_t T, int64_t H, int64_t W, adnm_stream_t stream);

/* Ensembles of M member forecasts (csrc/ensemble.hip): the members of a test-time-augmentation ensemble over the eight
 * symmetries of the square, the ONE integer statistic that verifies an ensemble, and the ensemble's products.  The reference has none; the
 * definitions are this project's and the yardstick is numpy (tests/ensemble_ref.py).  The score and the product take ANY stack of members.
 * These are not entry points of the scored-pair contract (they have M forecasts); they use its thresholds and its quantisation
 *   q(v) = floorf(fminf(fmaxf(v, 0), 1) * value_scale): NaN, -Inf and negatives give 0, +Inf and values >= 1 give Q = floor(value_scale).
 * adnm_d4_members: codes_host holds M ints in 0..7 with adnm_batch_fetch_aug's bits (bit 0 flip left-right, bit 1 flip up-down, bit 2
 *   transpose; g(w) = w.flip(-2), w.flip(-1), w.transpose(-1, -2) in that order), read on the host at call time.  `planes` = B * F planes of
 *   H x W fp32, contiguous.  inverse = 0: src is (planes, H, W), dst is (M, planes, H, W) and dst[m][p] = g_m(src[p]).  inverse = 1: src is
 *   (M, planes, H, W) too and dst[m][p] = g_m^-1(src[m][p]): transpose first, then the flips; the two quarter turns (codes 5 and 6) are each
 *   other's inverse, every other element is its own.  A copy of bit patterns: NaN payloads and -0.0 survive.  ONE launch, grid
 *   (32 x 32 tiles, planes, M), no workspace, every element of dst written.  Members without the transpose bit move 16 bytes per access
 *   when W % 4 == 0 and src and dst are 16-byte aligned (a mirrored row swaps the components of each piece), float by float otherwise;
 *   transposing members go float by float through a 32 x 33 LDS tile, coalesced on both sides.  The result is the same on every path.
 *   Refused (ADNM_EINVAL): a null pointer or one not 4-byte aligned; M outside 1..16; a code outside 0..7; the transpose bit with H != W;
 *   planes outside 1..65535; H or W outside [1, 32768); H*W >= 2^24.
 * adnm_valid_ens_accum ADDS a batch to table.  Frame f = b*T + t of member m starts at members + m*member_stride + b*sample_stride +
 *   t*frame_stride (in elements; a frame's hw pixels contiguous); target: contiguous (frames, hw).  y = q(target), x_i = q(member i); all
 *   further arithmetic is integer.  table: adnm_valid_ens_block_bytes(T, nthr, M) = 8 * T * C bytes, C = 7 + (M+1)^2 + 2*nthr*(M+1), 8-byte
 *   aligned, zeroed by the caller, all double, row t = f mod T:
 *     [0] N pixels   [1] Z: the DRY pixels, y = 0 and every x_i = 0   [2] S0 = SUM |x_0 - y| (member 0 is the control)
 *     [3] S1 = SUM_px SUM_i |x_i - y|   [4] S2 = SUM_px SUM_{i<j} |x_i - x_j|   [5] V = SUM_px (M SUM x_i^2 - (SUM x_i)^2)
 *     [6] E = SUM_px (SUM x_i - M y)^2
 *     [7 + b*(M+1) + e] rank bins R, b = #{x_i < y}, e = #{x_i = y}, over the pixels NOT counted in Z
 *     then per threshold k  X[k][o][c], o = (y >= thr_k), c = #{x_i >= thr_k}, laid out [o = 0: c = 0..M][o = 1: c = 0..M] as
 *       adnm_valid_nprob_accum's runs are, over the pixels NOT counted in Z.
 *   THE CONVENTION: a dry pixel is counted in Z alone.  Whoever reads the table adds Z to R[(0, M)] and, for a threshold > 0, to X[k][0][0]
 *   (for a threshold <= 0 every pixel is an event: to X[k][1][M]); validate.ensemble_entries does.  That is what lets the dry pixels, nearly
 *   all pixels of a radar field, leave the kernel through one ballot and popcount per wave.
 *   ONE launch, grid (items of 4096 pixels, frames), no workspace (adnm_valid_ens_accum_ws_bytes is 0 for every accepted shape, ws may be
 *   NULL).  Every float is read once, 16 bytes per access when hw and the three strides are multiples of 4 and both bases 16-byte aligned,
 *   float by float otherwise: same result.  Wet pixels keep their M levels as packed bytes, issue LDS atomics for their rank bin and their
 *   nthr exceedance bins only; the seven sums are reduced over the wave by shuffles and over the workgroup in uint64; non-zero entries
 *   reach the table as double atomics of integers: exact and the same bits on every run.  No workgroup waits for another.
 *   A pixel adds at most (M Q)^2 <= 4080^2 < 2^24 to E, the largest column.  Every sum stays below 2^53, and so exact, for 33024 frames per
 *   frame index at 128 x 128 and M = 16, Q = 255 (more than 10^6 at M = 8, Q = 90), and for 32 frames per frame index at hw = 2^24 - 1.
 *   Limits, refused before any launch (ADNM_EINVAL): a null pointer; members / target not 4-byte or table not 8-byte aligned; M outside
 *   2..16; nthr outside 1..8; value_scale not finite or floor(value_scale) outside 1..255; T < 1 or not dividing frames; frames > 65535;
 *   hw outside [1, 2^24); a stride that is neither 0 (held) nor at least the extent below it (frame_stride >= hw, sample_stride >=
 *   (T-1)*frame_stride + hw, member_stride >= (frames/T - 1)*sample_stride + that).  The *_bytes queries are pure host code and return -1.
 * adnm_ensemble_product: members as above.  mean, fp32 (frames, hw): ((x_0 + x_1) + ... + x_(M-1)) / float(M) on the RAW values, every add
 *   and the one division rounded on their own in fp32 (no FMA, no reassociation: a np.float32 loop gives the same bits).  prob, fp32
 *   (K, frames, hw): float(c) / float(M), c = #{q(x_i) >= thr_k}, one IEEE division (adnm_neighbour_prob's rule).  K = 0..8; K = 0 writes
 *   the mean only, prob and thresholds_host may be NULL and value_scale is not looked at.  Every element is written; 16 bytes per access
 *   when hw and the strides are multiples of 4 and members, mean and prob are 16-byte aligned, float by float otherwise.  Limits
 *   (ADNM_EINVAL): adnm_valid_ens_accum's on M, frames, T, hw, the strides and the pointers. */
int adnm_d4_members(const float* src, float* dst, const int* codes_host, int64_t M, int inverse, int64_t planes, int64_t H, int64_t W,
                    adnm_stream_t stream);
int64_t adnm_valid_ens_block_bytes(int64_t T, int64_t nthr, int64_t M);
int64_t adnm_valid_ens_accum_ws_bytes(int64_t frames, int64_t T, int64_t hw, int64_t nthr, int64_t M, float value_scale);
int adnm_valid_ens_accum(const float* members, int64_t member_stride, int64_t sample_stride, int64_t frame_stride, const float* target,
                         void* table, const float* thresholds_host, int64_t nthr, float value_scale, int64_t M, void* ws, int64_t ws_bytes,
                         int64_t frames, int64_t T, int64_t hw, adnm_stream_t stream);
int adnm_ensemble_product(const float* members, int64_t member_stride, int64_t sample_stride, int64_t frame_stride, float* mean, float* prob,
                          const float* thresholds_host, int64_t K, float value_scale, int64_t M, int64_t frames, int64_t T, int64_t hw,
                          adnm_stream_t stream);

/* The Lagrangian-persistence (advection) baseline: block-matched motion between the last two input frames (TREC, Rinehart & Garvey 1978)
 * and the last frame moved along it.  The reference has none; the definitions are this project's.  Integer arithmetic and
 * bit copies only: exact and bit-reproducible.
 *   quantisation  q(v): adnm_eval_counts' device function, the one adnm_valid_pool_accum uses.  value_scale <= 255, so q fits a byte.
 *   frames        prev, last: the last two input frames of a sample (x[:, T_in - 2], x[:, T_in - 1]), contiguous H x W fp32 each, given
 *                 by two base addresses and ONE sample stride in elements (slices of a (B, T_in, H, W) input: stride T_in*H*W).
 *   blocks        block in {8, 16, 32} tiles the frame from the top-left: nby = ceil(H / block), nbx = ceil(W / block); edge blocks are
 *                 clipped to the frame.
 *   cost          radius R in 1..8.  cost_b(dy, dx) = SUM |q(last)(y, x) - q(prev)(y - dy, x - dx)| for (dy, dx) in [-R, R]^2, over the
 *                 pixels (y, x) of block b inside the frame; q(prev) is 0 outside the frame.  uint32, at most 32*32*255.
 *   pick          the vector of a table: the (dy, dx) that minimises (cost, dy^2 + dx^2, dy, dx) lexicographically — an all-zero block and
 *                 every tie fall towards (0, 0) in a fixed order.
 *   global vector g = the pick of SUM_b cost_b (blocks tile the frame: the whole-frame SAD), summed in 64 bits.
 *   valid blocks  a block is valid when at least `block` of its in-frame pixels have q(last) >= echo (1..255).  A valid block takes its
 *                 own pick, an invalid one takes g (an echo could otherwise never be advected into an empty block).
 *   motion        int32 (samples, nby, nbx, 2) holding (vy, vx); last(y, x) ~ prev(y - vy, x - vx): the echo moves by +v per frame interval.
 *   advection     backward, semi-Lagrangian, piecewise constant: out[s, t, y, x] = last[s, y - (t+1) vy, x - (t+1) vx] with v of the block
 *                 (y / block, x / block); +0.0f where the source lies outside the frame; otherwise the fp32 BIT PATTERN of last (NaN and Inf
 *                 included, nothing is rounded).  Frame index t is lead t + 1 at the input's own frame spacing.
 * adnm_trec_motion: two launches.  trec_cost, one workgroup per (block, sample), stages the block and the (block + 2R)^2 window once as
 *   quantised bytes, four to a dword, and forms the (2R+1)^2 sums from packed dwords (v_alignbyte_b32, v_sad_u8); the tables and the echo
 *   counts go to ws (adnm_trec_ws_bytes, every byte written).  trec_pick, one workgroup per sample, sums the tables in block order, picks
 *   g and per block, applies validity and writes motion; cost_out (or NULL): uint32 (samples, nby, nbx, 2R+1, 2R+1), the tables, row dy + R,
 *   column dx + R.  Aligned shapes (W and the stride multiples of 4, both bases 16-byte aligned) are read 16 bytes per access, all others
 *   float by float: same result.
 * adnm_advect: one launch; out contiguous fp32 (samples, T, H, W), stored 16 bytes per access when W % 4 == 0 and out is 16-byte aligned.
 * All arguments are passed by value: the calls can be captured.
 * Limits, refused before any launch (ADNM_EINVAL): a null pointer other than cost_out; prev / last / out / motion / cost_out not 4-byte
 *   aligned; block outside {8, 16, 32}; radius outside 1..8; echo outside 1..255; value_scale not in (0, 255]; samples outside 1..65535;
 *   T < 1; H or W outside [1, 32768); H*W >= 2^24; sample_stride < H*W.  adnm_trec_ws_bytes returns -1. */
int64_t adnm_trec_ws_bytes(int64_t samples, int64_t H, int64_t W, int64_t block, int64_t radius);
int adnm_trec_motion(const float* prev, const float* last, int64_t sample_stride, void* motion_i32, void* cost_out_u32_or_null, float value_scale,
                     int64_t block, int64_t radius, int64_t echo, void* ws, int64_t ws_bytes, int64_t samples, int64_t H, int64_t W,
                     adnm_stream_t stream);
int adnm_advect(const float* last, int64_t sample_stride, const void* motion_i32, float* out, int64_t block, int64_t samples, int64_t T, int64_t H,
                int64_t W, adnm_stream_t stream);

/* The flow advection: the same baseline with sub-pixel vectors, a dense field and semi-Lagrangian transport along it.  It
 * stands beside the block scheme above and changes nothing of it.  The cost tables, the integer pick d = (dy, dx), the global pick g of the
 * 64-bit sum table and the validity of a block (`block` in-frame pixels with q(last) >= echo) are adnm_trec_motion's, unchanged.  All the
 * motion arithmetic is integer (fixed point); the final interpolation is fp32 with every rounding prescribed: exact and bit-reproducible.
 *   1. refinement  -> the block flow u, int32 (samples, nby, nbx, 2) holding (uy, ux) in 1/16 px.  A valid block refines its own pick on
 *                  its own table; an invalid block takes the global pick refined on the sum table (int64 arithmetic).  Each axis is refined
 *                  independently, using the two neighbours along that axis at the picked other coordinate.  With c0 the cost at the pick and
 *                  cm, cp the costs at d - 1, d + 1:  delta = 0 if |d| == radius, or if den = cm - 2 c0 + cp <= 0;  otherwise
 *                  num = 8 (cm - cp) and delta = sgn(num) * floor((2 |num| + den) / (2 den)): round half away from zero; |delta| <= 8
 *                  follows from c0 being minimal.  u = 16 d + delta.
 *   2. dense field V, int32 (samples, H, W, 2) in 1/256 px, bilinear between block centres.  Block centres are at b block + block/2 - 1/2;
 *                  the weights are integers and the vectors are clamped at the outermost centres.  Per axis of length N with nb blocks, at
 *                  pixel y:  p = 2y + 1 - block;  b0 = clamp(floor(p / (2 block)), 0, nb - 1);  b1 = min(b0 + 1, nb - 1);
 *                  w1 = p < 0 ? 0 : clamp(p - 2 block b0, 0, 2 block);  w0 = 2 block - w1.  Then S = SUM wy_i wx_j 16 u[b_i, b_j] over the
 *                  four corners and V = floor((S + 2 block^2) / (4 block^2)): an arithmetic shift, block is a power of two.
 *   3. transport   backward, semi-Lagrangian, along the field.  Per pixel p = (y, x) the displacement D is int32 in 1/256 px, D_0 = 0.  For
 *                  frame index t = 0 .. T - 1, per axis:  r = clamp(floor((256 p - D_t + 128) / 256), 0, N - 1), the pixel nearest the
 *                  departure point;  D_{t+1} = D_t + V[r];  the source is s = 256 p - D_{t+1} with i = floor(s / 256) and
 *                  f = (s - 256 i) / 256, exact in fp32.  The four taps are a = last[iy, ix], b = last[iy, ix+1], c = last[iy+1, ix],
 *                  d = last[iy+1, ix+1].  A tap outside the frame is +0.0f.  A tap whose weight is 0 is not read and contributes nothing:
 *                  fx == 0 gives top = a, fy == 0 gives out = top, so a NaN or Inf beside an integer source position does not leak, and
 *                  zero or whole-pixel motion remains a copy of the value.  Otherwise, in fp32: gx = 1 - fx, top = gx a + fx b,
 *                  bot = gx c + fx d, gy = 1 - fy, out = gy top + fy bot; every product and every sum is rounded to fp32 on its own, there
 *                  is no fused multiply-add.  Frame index t is lead t + 1 at the input's own frame spacing.
 * adnm_trec_flow: two launches.  adnm_trec_motion's trec_cost into ws (adnm_trec_flow_ws_bytes = adnm_trec_ws_bytes, every byte written);
 *   trec_flow, one workgroup per sample, sums the tables in block order in 64 bits (integers, no atomics), picks g and per block, applies
 *   validity, refines and writes flow; motion (or NULL): adnm_trec_motion's int32 (samples, nby, nbx, 2), so that one call serves both
 *   schemes.  prev, last, sample_stride and the 16-byte rule: adnm_trec_motion's.
 * adnm_flow_field: one launch, field = V; for inspection and drawing.  The transport does not need it.
 * adnm_advect_flow: one launch; out contiguous fp32 (samples, T, H, W).  A sample's block vectors are staged in LDS (up to 4096 blocks; beyond
 *   that they are read from memory: same result) and V at any pixel is formed from them by the integer formula; each lane owns four pixels
 *   of a row for all T frames (the chain over t is sequential).  Stored 16 bytes per access when W % 4 == 0 and out is 16-byte aligned, float
 *   by float otherwise: same result.
 * All arguments are passed by value: the calls can be captured.
 * Limits, refused before any launch (ADNM_EINVAL): those of adnm_trec_motion and adnm_advect (flow and field 4-byte aligned and not null),
 *   and T > 4096 (|V| <= 16 * 136, so |D| stays below 2^24 and 256 p - D inside int32).  adnm_trec_flow_ws_bytes returns -1. */
int64_t adnm_trec_flow_ws_bytes(int64_t samples, int64_t H, int64_t W, int64_t block, int64_t radius);
int adnm_trec_flow(const float* prev, const float* last, int64_t sample_stride, void* flow_i32, void* motion_i32_or_null, float value_scale,
                   int64_t block, int64_t radius, int64_t echo, void* ws, int64_t ws_bytes, int64_t samples, int64_t H, int64_t W,
                   adnm_stream_t stream);
int adnm_flow_field(const void* flow_i32, void* field_i32, int64_t block, int64_t samples, int64_t H, int64_t W, adnm_stream_t stream);
int adnm_advect_flow(const float* last, int64_t sample_stride, const void* flow_i32, float* out, int64_t block, int64_t samples, int64_t T, int64_t H,
                     int64_t W, adnm_stream_t stream);

/* Radially averaged power spectra (RAPSD) of observation and forecast and their co-spectrum, per wavenumber and frame index, as SUMS.
 * The reference has no spectrum; the definitions are this project's, follow pysteps' rapsd convention, and the yardstick
 * is numpy.fft.fft2 in float64.
 *   fields        o = clip(target, 0, 1) * value_scale, f = clip(forecast, 0, 1) * value_scale in fp32: the fields whose differences
 *                 adnm_valid_accum sums for RMSE, except that a NaN stays a NaN (numpy's clip) instead of becoming 0.
 *   frame sizes   H and W powers of two, 8 <= H, W <= 512.  L = max(H, W).
 *   transform     O = DFT2(o), F = DFT2(f), unnormalised; signed frequencies ky in [-H/2, H/2), kx in [-W/2, W/2).  Per coefficient
 *                 p_o = |O|^2 / (H W), p_f = |F|^2 / (H W), c = Re(F conj O) / (H W).
 *   radial bin    the wavenumber in cycles per L pixels is (ky L/H, kx L/W), both integers; r = round(sqrt(k2)), k2 = (ky L/H)^2 +
 *                 (kx L/W)^2, formed in integers as the r with r^2 - r < k2 <= r^2 + r (sqrt of an integer is never m + 1/2).  Bins
 *                 r = 0 .. R - 1, R = L/2, are kept; coefficients with r >= R (the corners) are dropped, as in pysteps.  n_r, the number of
 *                 coefficients of bin r, depends on (H, W) only: the host's business (ops.spectrum_bins).
 *   sums          P_o[r] = SUM p_o, P_f[r] = SUM p_f, C[r] = SUM c over the coefficients of bin r.  The device keeps SUMS; the caller
 *                 divides by n_r * samples for pysteps' mean.
 * table: adnm_valid_spectrum_block_bytes(T, H, W) = 8 * T * R * 3 bytes, 8-byte aligned, zeroed by the caller, all double, shape (T, R, 3):
 *   [t][r] = P_o, P_f, C for frame index t (frame f of a batch belongs to row f mod T), summed over every sample so far.  No header.
 * adnm_valid_spectrum_accum ADDS a batch.  target, pred and the two strides: adnm_valid_pool_accum's meaning (a contiguous forecast is
 *   (T*H*W, H*W), a held frame (T_in*H*W, 0)).  With T = frames on a zeroed table it is the one-shot per-frame form.  Every argument is
 *   passed by value, nothing is allocated and no device memory is read on the host: the call can be captured.  Three launches.  Rows: rows
 *   2p and 2p + 1 of ONE field are the real and imaginary part of one complex row, transformed along x in LDS and separated again; the
 *   fields are real, so only kx = 0 .. W/2 is kept and goes, transposed, to ws.  Columns: one workgroup per (kx, frame) transforms o's and
 *   f's column along y, forms p_o, p_f, c with one expression, doubles them for 0 < kx < W/2 (the column stands for -kx as well) and
 *   adds each bin's run of |ky| in ascending order in fp32; fold: per (t, r) the partials are added in DOUBLE, samples ascending, then kx
 *   ascending, and the table is updated.  o and f go through the SAME instructions and are never packed into one transform: pred == target
 *   gives P_f == P_o == C bit for bit, pred == 0 gives P_f = C = 0 exactly.  Each pixel is read from HBM once, 16 bytes per access when
 *   both bases are 16-byte aligned and both strides multiples of 4, float by float otherwise: same result.
 *   precision     radix-2 decimation in time in fp32; twiddles exp(-2 pi i j / N) from sincospi in double, rounded once to fp32.  A bin
 *                 sum has at most 2 + log2(H W) roundings per coefficient in front of it, then a handful of fp32 additions within one
 *                 column, then double.  No atomics: the same calls on the same table give the same bits, whatever ws held.
 *   ws            adnm_valid_spectrum_accum_ws_bytes: frames * (W/2 + 1) * (2 * H * 8 + R * 3 * 4) bytes, the transposed row transforms
 *                 and the per-workgroup partials, every byte written before it is read.
 * Limits, refused before any launch (ADNM_EINVAL): a null pointer; pred / target not 4-byte or table / ws not 8-byte aligned; H or W not a
 *   power of two or outside 8..512; T < 1 or not dividing frames; frames > 65535; pred_frame_stride neither 0 nor >= H*W;
 *   pred_sample_stride < 0; ws_bytes below the query.  The *_bytes queries return -1. */
int64_t adnm_valid_spectrum_block_bytes(int64_t T, int64_t H, int64_t W);
int64_t adnm_valid_spectrum_accum_ws_bytes(int64_t frames, int64_t T, int64_t H, int64_t W);
int adnm_valid_spectrum_accum(const float* pred, int64_t pred_sample_stride, int64_t pred_frame_stride, const float* target, void* table,
                              float value_scale, void* ws, int64_t ws_bytes, int64_t frames, int64_t T, int64_t H, int64_t W,
                              adnm_stream_t stream);

/* The joint histogram of the quantised observation and the quantised forecast per frame index: the sufficient statistic of every
 * contingency table at every integer threshold, of the frequency bias, the conditional bias and a quantile-mapping table.
 * The reference has no histogram; the yardstick is numpy.histogram2d on the quantised fields (tests/joint_ref.py), integer for integer.
 *   levels        L = (int)floorf(value_scale) + 1 (adnm_valid_joint_levels); value_scale finite with 2 <= L <= 128.
 *   q(v)          eval_trunc(eval_scaled(v, value_scale)) = floor(clip(v, 0, 1) * value_scale) in fp32, the level adnm_valid_accum compares
 *                 with its thresholds: a NaN, -Inf and negatives give 0, +Inf and values >= 1 give L - 1.
 * table: adnm_valid_joint_block_bytes(T, value_scale) = 8 * T * L * L bytes, 8-byte aligned device memory, zeroed by the caller, all double,
 *   shape (T, L, L): [t][q(target)][q(forecast)] = the number of pixels, over every sample so far, of the frames f with f mod T = t.  The
 *   target is on the row, the forecast on the column.  No header.  Every entry is an integer held in a double.
 * adnm_valid_joint_accum ADDS a batch.  target, pred and the two strides: adnm_valid_pool_accum's meaning (a contiguous forecast is
 *   (T*hw, hw), a held frame (T_in*hw, 0)); hw = H * W pixels per frame.  With T = frames on a zeroed table it is the one-shot per-frame
 *   form.  Every argument is passed by value, nothing is allocated and no device memory is read on the host: the call can be captured.  One
 *   launch, grid (G, T): a row's frames are cut into items of 4096 pixels, a workgroup counts its items into one u32 histogram of L * L bins
 *   in LDS (dynamic, 4 L^2 <= 64 KB: no function attribute) and adds the NON-ZERO bins to the table at the end.  Each pixel of each field is
 *   read from HBM once, 16 bytes per access when both bases are 16-byte aligned and hw and both strides are multiples of 4, float by float
 *   otherwise: same result.
 *   the hot bin   a radar field is mostly zero.  The lanes of a wave whose bin is (0, 0) are counted with a ballot and a popcount into a
 *                 per-wave scalar that reaches LDS once per workgroup; only the other lanes issue an LDS atomic.
 *   exactness     the counts in LDS are u32 integer atomics, and G is chosen so that a workgroup counts at most 2^31 pixels.  The flush is
 *                 a double atomic add per non-zero bin.  Every addend and every partial sum is an integer below 2^53 (frames * hw < 2^40
 *                 per call), so every addition is exact and the sum does not depend on the order: the table is exact, and the same bits on
 *                 every run, although the order of the atomics is not fixed.
 *   ws            adnm_valid_joint_accum_ws_bytes is 0 for every accepted shape (the partial histograms live in LDS); ws may be NULL.
 * Limits, refused before any launch (ADNM_EINVAL): a null pred, target or table; pred / target not 4-byte or table / ws not 8-byte aligned;
 *   value_scale outside the range above; T < 1 or not dividing frames; frames > 65535; hw < 1 or >= 2^24; pred_frame_stride neither 0 nor
 *   >= hw; pred_sample_stride < 0; ws_bytes below the query.  The queries return -1. */
int64_t adnm_valid_joint_levels(float value_scale);
int64_t adnm_valid_joint_block_bytes(int64_t T, float value_scale);
int64_t adnm_valid_joint_accum_ws_bytes(int64_t frames, int64_t T, int64_t hw, float value_scale);
int adnm_valid_joint_accum(const float* pred, int64_t pred_sample_stride, int64_t pred_frame_stride, const float* target, void* table,
                           float value_scale, void* ws, int64_t ws_bytes, int64_t frames, int64_t T, int64_t hw, adnm_stream_t stream);

/* Object-based scores from connected-component labelling of the event masks: how many rain cells a field has, how large
 * they are, and how many of them the other field touches.  The reference has no object score; the yardstick is scipy.ndimage.label on the
 * CPU (tests/objects_ref.py), integer for integer and pixel for pixel.
 *   field         q(v) = eval_trunc(eval_scaled(v, value_scale)), adnm_valid_joint_accum's: a NaN, -Inf and negatives give 0, +Inf and
 *                 values >= 1 give floor(value_scale).
 *   event         q >= thr, adnm_valid_accum's comparison.
 *   object        an 8-connected component of the event mask of ONE frame of ONE field; frames do not wrap and do not connect.
 *   label         1 + the row-major index of the object's first pixel; the background is 0.
 *   min_area      an object of fewer than min_area (>= 1) pixels is ignored in every column and labelled 0.
 * table: adnm_valid_objects_block_bytes(T, nthr) = 8 * T * 2 * nthr * 23 bytes, 8-byte aligned device memory, zeroed by the caller, all
 *   double, shape (T, 2, nthr, 23): [t][field][k], field 0 = target, 1 = forecast, threshold k, summed over every sample so far of the
 *   frames f with f mod T = t.  No header.  Columns:
 *     [0] objects   [1] SUM area (the frame's event count when min_area = 1)   [2] SUM area^2   [3] SUM over frames of the largest object's
 *     area (a frame without objects adds 0)   [4] matched objects: at least one pixel is an event of the OTHER field at the same threshold
 *     [5] SUM area of the matched objects   [6 + b] objects with floor(log2(area)) = b, b = 0 .. 16.
 *   Every addend is an integer.  A frame has at most 65 536 pixels, so it adds at most 2^32 to SUM area^2 (one object that fills it): the
 *   sums over 2^20 frames per frame index stay below 2^53 and every entry is exact.
 * adnm_valid_objects_accum ADDS a batch.  target, pred and the two strides: adnm_valid_pool_accum's meaning (a contiguous forecast is
 *   (T*H*W, H*W), a held frame (T_in*H*W, 0)).  thresholds_host (nthr floats) is read on the host at call time and passed by value: the call
 *   can be captured.  With T = frames on a zeroed table it is the one-shot per-frame form.  One launch, one workgroup of 1024 lanes per
 *   (frame, threshold), which labels BOTH fields (matching needs both masks).  The event bits of both fields are staged once in LDS, one
 *   ballot per 64 pixels, floats read 4 bytes per lane (any 4-byte aligned address takes the same route).  Labels are resolved by label
 *   equivalence: a pixel starts at the first pixel of its horizontal run, and a union-find with atomicMin links and pointer jumping unites the
 *   runs with the row above in ONE sweep, whatever the shape.  One u32 word per pixel holds the parent, then, for a root, its area in the
 *   low bits and the matched flag in the top bit.  The words live in LDS where the frame fits beside the bits (H * W <= about 38 000; up to
 *   160 KB of dynamic LDS) and in ws otherwise.  The roots' entries are reduced in u64 LDS counters and added to the table as double
 *   atomics: integers below 2^53, so the table is exact and the same bits on every run although the order of the atomics is not fixed.
 *   termination   no workgroup waits for another one.  A parent only decreases, so a find takes at most H * W steps; a union retries at
 *                 most H * W times, and one that gave up repeats the sweep, at most H * W times.
 *   ws            adnm_valid_objects_accum_ws_bytes: 0 where the words are in LDS, else 4 * H * W * min(frames * nthr, 512) bytes; what it
 *                 held does not matter; ws may be NULL when the query is 0.
 * adnm_label_objects writes the int32 label image (frames, H, W) of ONE field at ONE threshold with the same device code (one workgroup per
 *   frame); frame f = b*T + t starts at src + b*sample_stride + t*frame_stride.  adnm_label_objects_ws_bytes likewise, with frames for
 *   frames * nthr.
 * Limits, refused before any launch (ADNM_EINVAL): a null pointer other than ws; pred / target / src / labels not 4-byte or table / ws not
 *   8-byte aligned; nthr outside 1..8; min_area < 1; T < 1 or not dividing frames; frames > 65535; H or W < 1; H * W > 65 536; a frame
 *   stride neither 0 nor >= H*W; a sample stride < 0; ws_bytes below the query.  The queries return -1. */
int64_t adnm_valid_objects_block_bytes(int64_t T, int64_t nthr);
int64_t adnm_valid_objects_accum_ws_bytes(int64_t frames, int64_t T, int64_t H, int64_t W, int64_t nthr);
int adnm_valid_objects_accum(const float* pred, int64_t pred_sample_stride, int64_t pred_frame_stride, const float* target, void* table,
                             const float* thresholds_host, int64_t nthr, float value_scale, int64_t min_area, void* ws, int64_t ws_bytes,
                             int64_t frames, int64_t T, int64_t H, int64_t W, adnm_stream_t stream);
int64_t adnm_label_objects_ws_bytes(int64_t frames, int64_t T, int64_t H, int64_t W);
int adnm_label_objects(const float* src, int64_t sample_stride, int64_t frame_stride, void* labels_i32, float thr, float value_scale,
                       int64_t min_area, void* ws, int64_t ws_bytes, int64_t frames, int64_t T, int64_t H, int64_t W, adnm_stream_t stream);

/* SAL scores (Structure, Amplitude, Location; Wernli et al. 2008) from per-object intensity moments.  The reference has no
 * object score; the yardstick is scipy.ndimage on the CPU (tests/sal_ref.py).  Field, event, object, label and min_area are those of the
 * object scores above.
 *   weight        w = intensity[q], intensity_host a HOST table of floor(value_scale) + 1 entries of uint16_t, read at call time and passed by
 *                 value (the call can be captured); NULL is the identity w = q.  This needs value_scale finite with 1 <= floor(value_scale)
 *                 <= 255: a level fits a byte.
 *   coordinates   x = column, y = row; the domain scale is d = sqrt(H^2 + W^2).
 *   whole field   M = SUM w, Mx = SUM w x, My = SUM w y over the frame (whatever the threshold), the centre c = (Mx / M, My / M).
 *   per object    R = SUM w, Q = max w, X = SUM w x, Y = SUM w y over the pixels of an object of at least min_area pixels; an object with
 *                 R = 0 (only with a zero weight) contributes nothing and does not count as an object.  R < 2^32, X and Y < 2^40: all exact.
 *   per frame pair and threshold, in double, o = target and f = forecast:
 *     A  = (M_f - M_o) / (0.5 (M_f + M_o))                      defined when M_o + M_f > 0
 *     L1 = |c_f - c_o| / d                                      defined when M_o > 0 and M_f > 0
 *     V  = SUM_n R_n (R_n / Q_n) / SUM_n R_n                    per field, with at least one object
 *     r  = SUM_n R_n |(X_n / R_n, Y_n / R_n) - c| / SUM_n R_n   per field, with at least one object
 *     S  = (V_f - V_o) / (0.5 (V_f + V_o)),  L2 = 2 |r_f - r_o| / d,  L = L1 + L2     defined when both fields have an object
 * table: adnm_valid_sal_block_bytes(T, nthr) = 8 * T * nthr * 12 bytes, 8-byte aligned device memory, zeroed by the caller, all double,
 *   shape (T, nthr, 12): [t][k], summed over every sample so far of the frames f with f mod T = t.  No header.  Columns:
 *     [0] frames with A defined   [1] SUM A   [2] SUM |A|   [3] frames with L1 defined   [4] SUM L1   [5] frames with S defined   [6] SUM S
 *     [7] SUM |S|   [8] SUM L2   [9] SUM L over the frames of [5]   [10] frames where only the target has an object   [11] frames where only
 *     the forecast has one.  A and L1 do not depend on the threshold and are repeated in every threshold's row.
 * adnm_valid_sal_accum ADDS a batch; pred, target, the strides and thresholds_host as in adnm_valid_objects_accum.  Two launches.  The first
 *   runs one workgroup of 1024 lanes per (frame, threshold): it stages the event bits of both fields and the level q as one byte per pixel
 *   in LDS (floats are read once), labels one field at a time with the device code of adnm_label_objects, lets the first pixel of every run
 *   add the run's SUM w, max w, SUM w x and SUM w y to its object's record with integer atomics (record (y / 2) * ceil(W / 2) + x / 2 of the
 *   object's first pixel: two first pixels never share an aligned 2 x 2 cell), reduces the objects in double in a fixed order (a lane's
 *   objects ascending, a shuffle tree over the lanes, the waves ascending) and writes the item's 12 entries to ws.  The second adds, per
 *   (t, k, column), the batch's entries, samples ascending from 0.0, and adds that one sum to the table.  No floating-point atomics: the
 *   same bits on every run; a forecast that IS the target gives exact zeros.  Records and words live in LDS where they fit (H * W up to
 *   about 13 000), the records in ws up to about 26 000 pixels, both in ws above.
 *   ws            adnm_valid_sal_accum_ws_bytes = 8 * frames * nthr * 12 for the item rows, plus, per workgroup that needs a slice (at most
 *                 256), 24 bytes per record and 4 per pixel: at most 16 * H * W + 16 bytes.  Never NULL; what it held does not matter.
 * adnm_object_moments writes int64 (frames, 4, H, W) of ONE field at ONE threshold with the same device code (one workgroup per frame): R, Q,
 *   X, Y at the first pixel of every object of at least min_area pixels, 0 everywhere else; every element is written.  Frame f = b*T + t
 *   starts at src + b*sample_stride + t*frame_stride.  adnm_object_moments_ws_bytes: the slices alone (0: ws may be NULL).
 * Limits, refused before any launch (ADNM_EINVAL): a null pointer other than intensity_host (and, for adnm_object_moments, ws when the query
 *   is 0); pred / target / src not 4-byte or table / moments / ws not 8-byte aligned; nthr outside 1..8; min_area < 1; value_scale outside
 *   the range above; T < 1 or not dividing frames; frames > 65535; H or W < 1; H * W > 65 536; a frame stride neither 0 nor >= H*W; a sample
 *   stride < 0; ws_bytes below the query.  The queries return -1. */
int64_t adnm_valid_sal_block_bytes(int64_t T, int64_t nthr);
int64_t adnm_valid_sal_accum_ws_bytes(int64_t frames, int64_t T, int64_t H, int64_t W, int64_t nthr);
int adnm_valid_sal_accum(const float* pred, int64_t pred_sample_stride, int64_t pred_frame_stride, const float* target, void* table,
                         const float* thresholds_host, int64_t nthr, float value_scale, int64_t min_area, const uint16_t* intensity_host,
                         void* ws, int64_t ws_bytes, int64_t frames, int64_t T, int64_t H, int64_t W, adnm_stream_t stream);
int64_t adnm_object_moments_ws_bytes(int64_t frames, int64_t T, int64_t H, int64_t W);
int adnm_object_moments(const float* src, int64_t sample_stride, int64_t frame_stride, void* moments_i64, float thr, float value_scale,
                        int64_t min_area, const uint16_t* intensity_host, void* ws, int64_t ws_bytes, int64_t frames, int64_t T, int64_t H,
                        int64_t W, adnm_stream_t stream);

/* Space-time rain-cell tracks by connected-component labelling of the (t, y, x) event volume: how long cells live, when
 * they are born and die, and how many of the cells of the first lead time survive to each later one.  This is the space-time object of MODE
 * Time Domain (MET).  The reference has no object score; the yardstick is scipy.ndimage.label with the full 3 x 3 x 3 structure on the CPU
 * (tests/tracks_ref.py), integer for integer and voxel for voxel.  Field, quantisation and event are those of the object scores above.
 *   track         a 26-connected component (|dt|, |dy|, |dx| <= 1) of the event voxels of ONE sample's (T, H, W) volume of ONE field.  Samples
 *                 never connect; frames do not wrap.  A cell that moves at most 1 px per frame stays one track however thin it is.
 *   label         1 + (t*H*W + y*W + x) of the track's first voxel, the smallest flat index inside the sample's volume; the background is 0.
 *   per track     t0 the frame of the first voxel, t1 the last frame holding one of its voxels, d = t1 - t0 + 1, v its voxels; matched when
 *                 any of its voxels is an event of the OTHER field at the same threshold.
 *   min_volume    a track of fewer than min_volume (>= 1) voxels is ignored in every column and labelled 0.
 * table: adnm_valid_tracks_block_bytes(T, nthr) = 8 * 2 * nthr * C bytes, C = 7 + 4 T, 8-byte aligned device memory, zeroed by the caller, all
 *   double, shape (2, nthr, C): [field][k], field 0 = target, 1 = forecast, summed over every sample so far.  A track belongs to no single
 *   frame index, so this table has NO leading T axis (the one deviation from the scored pair's "row t = f mod T").  Columns:
 *     [0] tracks N   [1] SUM v   [2] SUM v^2   [3] SUM d   [4] matched tracks   [5] SUM v of the matched tracks   [6] spanning tracks (t0 = 0
 *     and t1 = T - 1)   [7 + t] births: tracks with t0 = t   [7 + T + t] deaths: tracks with t1 = t   [7 + 2T + t] deaths of the initial
 *     tracks: t1 = t among those with t0 = 0   [7 + 3T + d - 1] the duration histogram.
 *   Hence SUM births = SUM deaths = SUM hist = N, SUM deaths0 = births[0], deaths0[T - 1] = spanning, SUM d = SUM (k + 1) hist[k].
 *   Every addend is an integer, and the sums are exact while SUM v^2 < 2^53: a volume has at most 2^22 voxels, so one sample adds at most
 *   2^44; at 20 x 128^2 a sample adds at most 2^36.7 and more than 80 000 all-event samples fit.
 * adnm_valid_tracks_accum ADDS a batch; the arguments are adnm_valid_objects_accum's with min_volume in place of min_area.  A held frame
 *   (pred_frame_stride = 0) is legal and gives only spanning tracks.  Per chunk of thresholds, four launches in stream order, no workgroup
 *   waiting for another one: (1) a workgroup of 1024 lanes per (frame, threshold) labels the frame's 8-connected objects of both fields with
 *   the device code of adnm_valid_objects_accum and writes, per voxel, the parent as an index into the sample's volume, at an object's first
 *   pixel its area and matched flag, the frame index, and the event bits (a plane per frame, padded to whole ballots); (2) a workgroup per
 *   (frame boundary, threshold, field) unites every event voxel with its event neighbours in the 3 x 3 window of the frame before, through
 *   the same lock-free union on the global words with agent-scope atomics; (3) every object's first pixel finds its track's root and adds
 *   its area, flag and frame to the root's words with integer atomics; (4) the roots of at least min_volume voxels add their columns to u64
 *   LDS counters, whose non-zero entries go to the table as double atomics: integers below 2^53, the same bits on every run.
 *   termination   a parent only decreases, so a find takes at most T*H*W steps; after a lost race the larger of a union's two roots is
 *                 strictly smaller than before, so a union ends within T*H*W rounds and none is ever dropped.
 *   ws            adnm_valid_tracks_accum_ws_bytes = c * 2 * frames * 4 * (3 H W + 2 ceil(H W / 64)) with c = the thresholds per chunk: all
 *                 nthr where that stays within 256 MB, else as many as do, at least one.  Never NULL; what it held does not matter.
 * adnm_label_tracks writes the int32 label volume (frames, H, W) of ONE field at ONE threshold with the same device code; every element is
 *   written, 0 for the background and for dropped tracks.  Frame f = b*T + t starts at src + b*sample_stride + t*frame_stride.
 *   adnm_label_tracks_ws_bytes = frames * 4 * (3 H W + 2 ceil(H W / 64)); never NULL.
 * Limits, refused before any launch (ADNM_EINVAL): a null pointer; pred / target / src / labels not 4-byte or table / ws not 8-byte aligned;
 *   nthr outside 1..8; min_volume < 1; T < 1 or not dividing frames; frames > 65535; H or W < 1; H * W > 65 536; T * H * W > 2^22; a frame
 *   stride neither 0 nor >= H*W; a sample stride < 0; ws_bytes below the query.  The queries return -1. */
int64_t adnm_valid_tracks_block_bytes(int64_t T, int64_t nthr);
int64_t adnm_valid_tracks_accum_ws_bytes(int64_t frames, int64_t T, int64_t H, int64_t W, int64_t nthr);
int adnm_valid_tracks_accum(const float* pred, int64_t pred_sample_stride, int64_t pred_frame_stride, const float* target, void* table,
                            const float* thresholds_host, int64_t nthr, float value_scale, int64_t min_volume, void* ws, int64_t ws_bytes,
                            int64_t frames, int64_t T, int64_t H, int64_t W, adnm_stream_t stream);
int64_t adnm_label_tracks_ws_bytes(int64_t frames, int64_t T, int64_t H, int64_t W);
int adnm_label_tracks(const float* src, int64_t sample_stride, int64_t frame_stride, void* labels_i32, float thr, float value_scale,
                      int64_t min_volume, void* ws, int64_t ws_bytes, int64_t frames, int64_t T, int64_t H, int64_t W, adnm_stream_t stream);

/* The output side (pic_results.py:104-184 of the reference): a forecast as the bytes a consumer keeps, in ONE launch.
 * adnm_forecast_render: pred contiguous fp32 (B, T, H, W), 4-byte aligned.  fields: (B, T, H, W) uint8 or NULL.  strip: (B, H, Ws, 4) uint8
 *   (RGBA, 4-byte aligned) or NULL, Ws = n*W + (n-1)*gap, holding the n = ceil((T - frame_start) / frame_step) frames frame_start,
 *   frame_start + frame_step, ... side by side along the width with `gap` pixels 255,255,255,255 between neighbours and none at the ends.
 *   At least one of fields / strip.  bounds_host: nbins + 1 finite, strictly ascending floats; palette_host: nbins x 4 bytes (R, G, B, A);
 *   both in HOST memory, read at call time and passed by value as kernel arguments (nothing to keep alive; the call can be captured).
 * Value rule, per pixel p:
 *   pixel_scale > 0:  b = (uint8) trunc(clamp(p * pixel_scale, 0, 255)), the product formed in fp32 on its own (not contracted into
 *       anything else); NaN gives 0.  fields receives b; the binned value is v = (float) b.  Inside [0, 256) this is numpy's
 *       (seq * pixel_scale).astype(np.uint8); numpy's cast of a float outside the range is undefined, so the clamp is THIS project's
 *       definition there (negative, -Inf, NaN -> 0; above 255, +Inf -> 255).
 *   pixel_scale == 0: the binned value is v = p itself; fields receives the bin index; a NaN pixel renders 0,0,0,0 (matplotlib's "bad"
 *       colour) and its fields byte is 0.
 *   bin index = clamp(#{k : bounds[k] <= v} - 1, 0, nbins - 1) (BoundaryNorm + ListedColormap: below the first edge the first colour, at
 *       or above the last edge the last); strip receives palette[index].  The comparison is made in fp32 AGAINST THE EDGES AS GIVEN:
 *       matplotlib compares the fp32 value with double edges, so a caller holding double edges passes each one rounded UP to the
 *       smallest float >= it (an edge rounded down would admit the value equal to that float, which the double edge rejects).
 * Limits: 1 <= nbins <= 32, B*T*H*W < 2^31, 0 <= frame_start < T, frame_step >= 1, 0 <= gap < 2^24, pixel_scale finite >= 0; with a strip
 *   (not for a fields-only call) Ws < 2^24 and strip 4-byte aligned.
 *   Anything else is refused before any launch. */
int adnm_forecast_render(const float* pred, uint8_t* fields, uint8_t* strip, const float* bounds_host, const uint8_t* palette_host,
                         int64_t nbins, float pixel_scale, int64_t B, int64_t T, int64_t H, int64_t W, int64_t frame_start,
                         int64_t frame_step, int64_t gap, adnm_stream_t stream);

/* ---------------------------------------------------------------- stand-alone activations
 * act_fwd / act_bwd: y = act(x), dpre = dy * act'(pre) over flat fp32 arrays (any n > 0, 16-byte aligned pointers: the last n % 4
 *   elements go by scalar accesses in the same launch), act in {ADNM_ACT_SILU, ADNM_ACT_GELU}: nn.GELU between Mlp.fc1 and fc2
 *   (model_untils.py:52-70) and the backward of the GELUs fused into GEMM / conv epilogues.
 * swish_fwd / bwd: Swish with a learnable slope, y = x * sigmoid(beta * x) (model_untils.py:162-169), beta a 1-element device tensor;
 *   bwd OVERWRITES dx and dbeta (1 element). */
int adnm_act_fwd(const float* x, float* y, int64_t n, int act, adnm_stream_t stream);
int adnm_act_bwd(const float* dy, const float* pre, float* dpre, int64_t n, int act, adnm_stream_t stream);
int adnm_swish_fwd(const float* x, const float* beta, float* y, int64_t n, adnm_stream_t stream);
int64_t adnm_swish_bwd_ws_bytes(int64_t n);
int adnm_swish_bwd(const float* dy, const float* x, const float* beta, float* dx, float* dbeta, void* ws, int64_t ws_bytes, int64_t n,
                   adnm_stream_t stream);

/* Wire format of the data-parallel gradient all-reduce that replaces nn.DataParallel's reduce_add_coalesced (train.py:99-102;
 * SURVEY.md §8e): dst[i] = (bf16)(scale * src[i]) before the collective, dst[i] = scale * (float)src[i] after it (scale = 1/world
 * folds the average in).  n elements, both buffers 16-byte aligned. */
int adnm_cast_f32_bf16(const void* src, void* dst, int64_t n, float scale, adnm_stream_t stream);
int adnm_cast_bf16_f32(const void* src, void* dst, int64_t n, float scale, adnm_stream_t stream);

/* Gradient accumulation over micro-batches: train.py:136-145 with loss.backward() repeated k times before optimizer.step() — there
 * autograd adds into p.grad; here the backward kernels OVERWRITE their flat_g slices every pass, so the sum lives in a second flat
 * fp32 buffer.  Streaming passes over a flat range: acc, g 16-byte aligned, n > 0, n % 4 == 0.
 *   adnm_grad_accum, micro-steps 1 .. k-1:   first != 0: acc[i] = g[i]   (acc is NOT read: no memset is ever needed; 8 B/element)
 *                                            first == 0: acc[i] = acc[i] + g[i]                                  (12 B/element)
 *   adnm_grad_accum_final, micro-step k:     g[i] = (acc[i] + g[i]) * scale   (add, then multiply, each rounded once; scale = 1/k)
 *       wire_bf16 != NULL (8-byte aligned): also wire_bf16[i] = bf16_rne(g[i]), the range's image for the bf16 collective
 *       (adnm_cast_f32_bf16 of the result, without the second pass).  12 (14) B/element.
 * After the final pass g holds the averaged accumulated gradient; adnm_adamw_step runs on it unchanged. */
int adnm_grad_accum(float* acc, const float* g, int64_t n, int first, adnm_stream_t stream);
int adnm_grad_accum_final(const float* acc, float* g, void* wire_bf16, int64_t n, float scale, adnm_stream_t stream);

/* Exponential moving average of the parameters (FlatTrainer(ema_decay=...)): a second flat fp32 buffer laid out like p.  Streaming
 * passes: p, ema 16-byte aligned and disjoint, n > 0, n % 4 == 0; checked on entry.  <= 2048 workgroups of 256 lanes, two 16-byte quads
 * per lane and trip, the rest by grid stride.
 *   adnm_ema_update, behind the optimiser pass of the same step:  t = state[0] (adnm_adamw_step's step counter, after that pass),
 *       d = warmup ? min(decay, (1 + t) / (10 + t)) : decay,  w = 1.0f - d,  ema[i] = fmaf(d, ema[i], w * p[i])   (two roundings;
 *       12 B/element).  d is formed on the device, so a captured launch follows the counter.  decay in [0, 1]: 0 leaves ema == p,
 *       1 leaves ema as it was.  info[0] = the d this call used, info[1] += 1 (updates applied); two device floats, 4-byte aligned.
 *       stats: the statistics block of adnm_step_guard (8-byte aligned) or NULL; with its skip flag set every workgroup returns after
 *       one uniform load and neither ema nor info is written (adnm_adamw_step_guarded's rule).
 *   adnm_ema_swap: p and ema exchange their contents, bit pattern for bit pattern, in one pass without a temporary buffer
 *       (16 B/element); twice is the identity. */
int adnm_ema_update(const float* p, float* ema, int64_t n, const float* state, float decay, int warmup, float* info, const void* stats,
                    adnm_stream_t stream);
int adnm_ema_swap(float* p, float* ema, int64_t n, adnm_stream_t stream);

/* ---------------------------------------------------------------- tall-skinny fp32 GEMMs on MFMA (K6)
 * The Linear / 1x1 projections of the full-resolution stages (ADNssd.py:309,461; model_untils.py:64,67,193,196,831;
 * ADNMUNet.py:634): M = B*H*W tokens, K,N <= 256.  v_mfma_f32_16x16x4_f32: exact fp32 (an fmaf chain).
 *   nt: Y[M,N] = X[M,K] . Wp^T (+bias[N]),  Wp[n][k] = w[n*ws_n + k*ws_k]   (forward: ws_n=K, ws_k=1;
 *       input gradient dX = dY . W: call with X:=dY, N:=K_w, K:=N_w, ws_n=1, ws_k=K_w).  K % 16 == 0.
 *   tn: dW[N,K] = dY[M,N]^T . X[M,K], dbias[N] = column sums of dY (NULL skips); OVERWRITTEN; ws from *_ws_bytes.
 * *_supported() return 1 when the shape fits the kernels (callers use the library GEMM otherwise). */
int adnm_tsgemm_supported(int64_t M, int64_t N, int64_t K);
/* x_dtype / y_dtype (ADNM_F32 | ADNM_BF16): storage type of the token rows read / written; bf16 storage needs prec = ADNM_MFMA_BF16
 * (the wide intermediates of the full-resolution level are kept in bf16 in the bf16 configuration: half the bytes). */
int adnm_tsgemm_nt(const void* x, int64_t ldx, const float* w, int64_t ws_n, int64_t ws_k, const float* bias, void* y,
                   int64_t ldy, int64_t M, int64_t N, int64_t K, int prec, float* q, int x_dtype, int y_dtype, adnm_stream_t stream);
int adnm_tsgemm_tn_supported(int64_t M, int64_t N, int64_t K);
int64_t adnm_tsgemm_tn_ws_bytes(int64_t M, int64_t N, int64_t K);
int adnm_tsgemm_tn(const void* dy, int64_t lddy, const void* x, int64_t ldx, float* dw, float* dbias, void* ws,
                   int64_t ws_bytes, int64_t M, int64_t N, int64_t K, int dy_dtype, int x_dtype, adnm_stream_t stream);

/* ---------------------------------------------------------------- parameter-side preparation (one launch each way)
 * ADN-SSD mixer: reference-layout parameters -> kernel-layout tensors (row-permuted in_proj, effective 3x3 taps of
 * the conv2d / asymmetric 1x3o3x1 chains (ADNssd.py:334,343-346) in tap-major order, permuted LayerNorm weights,
 * alpha1 * column-permuted out_proj (ADNssd.py:459)) and the transpose of that map for the gradients.
 *   params[15]  = {in_proj.weight, conv2d.weight, conv_31_x1, conv_31_bc1, conv_31_x2, conv_31_bc2, conv_13_x1,
 *                  conv_13_bc1, conv_13_x2, conv_13_bc2, conv2d_z.weight, norm.weight, norm.bias, out_proj.weight, alpha1}
 *   prepped[6]  = {w_in (d_in_proj,dm), cw (9,di+2gn), czw (9,di), ln_w (di), ln_b (di), w_out (dm,2di)}
 * All fp32 device pointers; the tables themselves are host arrays.  gn = ngroups*d_state.
 * tap_ld: row stride (floats) of BOTH tap images, 0 = dense (di+2gn resp. di).  With tap_ld = 2di+2gn, czw = T and cw = T + di are
 * the two column ranges of ONE (9, 2di+2gn) image T = [czw | cw]: the taps of a single depthwise launch over [z | xBC]. */
int adnm_adnprep_fwd(float* const* params, float* const* prepped, int64_t d_model, int64_t d_inner, int64_t gn,
                     int64_t headdim, int64_t tap_ld, adnm_stream_t stream);
int64_t adnm_adnprep_bwd_ws_bytes(void);
int adnm_adnprep_bwd(float* const* params, float* const* gprepped, float* const* dparams, int64_t d_model,
                     int64_t d_inner, int64_t gn, int64_t headdim, int64_t tap_ld, void* ws, int64_t ws_bytes,
                     adnm_stream_t stream);
/* WTConv2d: taps[k] (K*K, Cgp) = tap-major( w[k] (Cg,K*K) * s[k] (Cg) ), zero-padded from C to Cp channels
 * (Cg = C for k = 0, the base conv; 4C for the level convs k = 1..levels), bias_t = bias * s[0]
 * (WTConv2d.py:123,146).  bwd: dw, ds, dbias from the tap gradients. */
int adnm_wtprep_fwd(float* const* w, float* const* s, float* bias, float* const* taps, float* bias_t, int64_t C,
                    int64_t Cp, int64_t K, int64_t levels, adnm_stream_t stream);
int adnm_wtprep_bwd(float* const* w, float* const* s, float* bias, float* const* gtaps, float* gbias_t,
                    float* const* dw, float* const* ds, float* dbias, int64_t C, int64_t Cp, int64_t K, int64_t levels,
                    adnm_stream_t stream);
/* Grouped forms: every ADN-SSD mixer / every WTConv2d of a model stage in ONE launch each way (36 per-module launches of a few
 * microseconds each at config 2).  Tables are concatenated per module i: params[15 i ..], prepped / gprepped[6 i ..], dparams[15 i ..],
 * dims[5 i ..] = {d_model, d_inner, gn, headdim, tap_ld};  WTConv2d: w / s / taps / gtaps / dw / ds[5 i ..] (entries 0 .. levels), bias[i],
 * bias_t[i], gbias_t[i], dbias[i] (all NULL or all set per module), dims[4 i ..] = {C, Cp, K, levels}.  More than 8 modules are cut into
 * several launches.  Same results as the per-module entry points, bit for bit.
 * adnm_adnprep_fwd_multi, narrow (optional, NULL = none): narrow[5 i ..] = {w_in_n, w_out_n, s_in, s_out, s_out_eff} — NARROW copies of the
 * two big matrices of mixer i for the weight-streaming GEMMs (adnm_skgemm b_dtype = narrow_dtype) INSTEAD of the fp32 ones (prepped[6 i]
 * resp. prepped[6 i + 5] may then be NULL): ADNM_B_BF16: bf16 values; ADNM_B_FP8: w_in_n = e4m3(w_in * *s_in), w_out_n = e4m3(w_out * e)
 * with e = *s_out / |alpha1| written to *s_out_eff (s_in / s_out: the scale_b of in_proj.weight's / out_proj.weight's quantisation
 * records — a row / column permutation keeps a tensor's maximum, alpha1 scales it). */
int adnm_adnprep_fwd_multi(int64_t n, float* const* params, float* const* prepped, const int64_t* dims, float* const* narrow, int narrow_dtype,
                           adnm_stream_t stream);
int64_t adnm_adnprep_bwd_multi_ws_bytes(int64_t n);
int adnm_adnprep_bwd_multi(int64_t n, float* const* params, float* const* gprepped, float* const* dparams, const int64_t* dims, void* ws,
                           int64_t ws_bytes, adnm_stream_t stream);
int adnm_wtprep_fwd_multi(int64_t n, float* const* w, float* const* s, float* const* bias, float* const* taps, float* const* bias_t,
                          const int64_t* dims, adnm_stream_t stream);
int adnm_wtprep_bwd_multi(int64_t n, float* const* w, float* const* s, float* const* bias, float* const* gtaps, float* const* gbias_t,
                          float* const* dw, float* const* ds, float* const* dbias, const int64_t* dims, adnm_stream_t stream);


#ifdef __cplusplus
}
#endif
#endif /* ADNM_HIP_H */
