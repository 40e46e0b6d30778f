// The data formats on either side of the hot path: data in (radar_ingest, batch_fetch and its augmented
// form), the point-wise evaluator (eval_counts, eval_ssim), the validation epoch's accumulators of a CONTIGUOUS prediction (valid_accum,
// valid_ssim_accum) and data out (forecast_render).  The scores of a strided forecast against a target live in files of their own
// (scored_pair.h names them).
//
//   radar_ingest  — the input pipeline of datasets/Shanghai.py:52-59,121: uint8 radar frames (25, H0, W0) in 0..70 -> float / 255 ->
//                   transforms.Resize((S, S)) (bilinear, align_corners=False, no antialias: what torchvision's tensor Resize hands to
//                   F.interpolate) -> (B, T, 1, S, S) fp32, in ONE pass over bytes that arrive by DMA from pinned host memory, instead of
//                   a float copy 4x the size followed by torch's resize and a pageable, synchronous H2D copy (train.py:134).
//   eval_counts   — SimplifiedEvaluator.evaluate (datasets/Shanghai_metrics.py:49-152) without the round trip to numpy: per frame the
//                   contingency counts TP / FN / FP / TN at every threshold on the uint16-truncated, value_scale'd, [0,1]-clipped fields
//                   (:45-47,103-112) and the sums |d|, d^2 of the scaled float fields (:114-120) from which MAE / MSE / RMSE / PSNR follow.
//   valid_accum   — the validation half of an epoch (train.py:156-206): the same counts and sums plus the enRainfallLoss value of the batch,
//                   ADDED to a block of doubles the caller keeps on the device for the whole epoch (no gradient tensor, no host read).
//   forecast_render — the output side, pic_results.py:104-184: the forecast quantised to a byte per pixel ((seq * pixel_scale).astype(uint8)),
//                   the frame selection seq[1::2], BoundaryNorm + ListedColormap as a table lookup and the frames laid side by side with a
//                   gap of opaque white, as RGBA bytes: what a consumer stores, instead of a float copy and numpy / matplotlib per frame.
#include "scored_pair.h"
#include <math.h>

namespace {
constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void radar_ingest_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int64_t frames, int H0, int W0,
                                                              int S, float scale_y, float scale_x, float mul) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= frames * S * S) return;
  const int x = (int)(i % S), y = (int)((i / S) % S);
  const int64_t f = i / ((int64_t)S * S);
  // torch's area_pixel_compute_source_index(align_corners=False): src = scale * (dst + 0.5) - 0.5, clamped at 0
  float sy = scale_y * (y + 0.5f) - 0.5f, sx = scale_x * (x + 0.5f) - 0.5f;
  sy = sy < 0.f ? 0.f : sy;
  sx = sx < 0.f ? 0.f : sx;
  const int y0 = (int)sy < H0 - 1 ? (int)sy : H0 - 1, x0 = (int)sx < W0 - 1 ? (int)sx : W0 - 1;
  const int y1 = y0 + (y0 < H0 - 1), x1 = x0 + (x0 < W0 - 1);
  const float ly = sy - y0, lx = sx - x0, hy = 1.f - ly, hx = 1.f - lx;
  const uint8_t* p = src + f * (int64_t)H0 * W0;
  const float v00 = p[(int64_t)y0 * W0 + x0], v01 = p[(int64_t)y0 * W0 + x1], v10 = p[(int64_t)y1 * W0 + x0], v11 = p[(int64_t)y1 * W0 + x1];
  // the reference divides by 255 BEFORE resizing; interpolation is linear, so the order only moves the rounding: kept as the reference has it
  dst[i] = hy * (hx * (v00 * mul) + lx * (v01 * mul)) + ly * (hx * (v10 * mul) + lx * (v11 * mul));
}

// The quantisation of a field value q(v): eval_scaled / eval_trunc of adnm_common.h, stated ONCE for every kernel that counts events
// (EvalAcc::add here, pair_bits of scored_pair.h) or matches blocks (advect.hip).  Thr, the thresholds as a kernel argument: scored_pair.h.

// One lane's share of a frame's contingency counts and error sums, and the workgroup's fold of it: the arithmetic of eval_counts, stated
// ONCE for eval_counts_kernel and valid_accum_kernel (the validation epoch's accumulating pass) so that their counts cannot drift apart.
struct EvalAcc {
  float cnt[4 * kMaxThr], sa, sq;
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int k = 0; k < 4 * kMaxThr; ++k) cnt[k] = 0.f;
    sa = sq = 0.f;
  }
  // clip to [0,1], scale, truncate, compare (Shanghai_metrics.py:45-47,103-120)
  __device__ __forceinline__ void add(float tv, float pv, float value_scale, const Thr& thr) {
    const float ts = eval_scaled(tv, value_scale), ps = eval_scaled(pv, value_scale);
    const float d = ps - ts;
    sa += fabsf(d);
    sq = fmaf(d, d, sq);
    const float ti = eval_trunc(ts), pi = eval_trunc(ps);
#pragma unroll
    for (int k = 0; k < kMaxThr; ++k)
      if (k < thr.n) {
        const bool o = ti >= thr.t[k], s = pi >= thr.t[k];
        cnt[4 * k + 0] += (o && s) ? 1.f : 0.f;     // TP
        cnt[4 * k + 1] += (o && !s) ? 1.f : 0.f;    // FN
        cnt[4 * k + 2] += (!o && s) ? 1.f : 0.f;    // FP
        cnt[4 * k + 3] += (!o && !s) ? 1.f : 0.f;   // TN
      }
  }
  // wave sums -> sm[wave][0 .. 4*nthr + 2); EXTRA: a further per-lane sum of the caller's -> sm[wave][4*nthr + 2].  The caller
  // synchronises and adds the four waves as (0 + 1) + (2 + 3).
  template <bool EXTRA, int COLS>
  __device__ __forceinline__ void to_lds(float (*sm)[COLS], int nthr, float extra) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 4 * kMaxThr; ++k) {
      const float v = wave_sum(cnt[k]);
      if (lane == 0 && k < 4 * nthr) sm[wave][k] = v;
    }
    sa = wave_sum(sa);
    sq = wave_sum(sq);
    if (EXTRA) extra = wave_sum(extra);
    if (lane == 0) {
      sm[wave][4 * nthr] = sa;
      sm[wave][4 * nthr + 1] = sq;
      if (EXTRA) sm[wave][4 * nthr + 2] = extra;
    }
  }
};

// part[blk][frame][4*nthr + 2]; blocks along a frame: gridDim.x, frames: gridDim.y
__global__ __launch_bounds__(kBlock) void eval_counts_kernel(const float* __restrict__ truth, const float* __restrict__ pred, float* __restrict__ part,
                                                             int64_t hw, float value_scale, Thr thr) {
  __shared__ float sm[kBlock / 64][4 * kMaxThr + 2];
  const int64_t f = blockIdx.y;
  const float* t = truth + f * hw;
  const float* p = pred + f * hw;
  EvalAcc acc;
  acc.clear();
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < hw; i += (int64_t)gridDim.x * kBlock) acc.add(t[i], p[i], value_scale, thr);
  const int nout = 4 * thr.n + 2;
  acc.to_lds<false>(sm, thr.n, 0.f);
  __syncthreads();
  if ((int)threadIdx.x < nout)
    part[((int64_t)blockIdx.x * gridDim.y + f) * nout + threadIdx.x] = (sm[0][threadIdx.x] + sm[1][threadIdx.x]) + (sm[2][threadIdx.x] + sm[3][threadIdx.x]);
}

// The validation epoch's pass (include/adnm_hip.h: adnm_valid_accum): eval_counts_kernel's grid and arithmetic, and beside it the
// enRainfallLoss terms of the UNCLIPPED values (adnm_rainloss_term, no gradient).  part[blk][frame][4*nthr + 3]: the last column is
// the workgroup's sum of e.  Longest chain of fp32 additions behind a loss partial: the lane's trips (hw / (blocks * 256) <= 16 while
// hw <= 2^18: eval_blocks) + 6 (wave) + 2 (the four waves); the partials are then folded in double.
__global__ __launch_bounds__(kBlock) void valid_accum_kernel(const float* __restrict__ pred, const float* __restrict__ tgt, float* __restrict__ part,
                                                             int64_t hw, float value_scale, Thr thr, float omega, float alpha, float gamma) {
  __shared__ float sm[kBlock / 64][4 * kMaxThr + 3];
  const int64_t f = blockIdx.y;
  const float* t = tgt + f * hw;
  const float* p = pred + f * hw;
  EvalAcc acc;
  acc.clear();
  float e = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < hw; i += (int64_t)gridDim.x * kBlock) {
    const float tv = t[i], pv = p[i];
    acc.add(tv, pv, value_scale, thr);
    e += adnm_rainloss_term<false>(pv, tv, omega, alpha, gamma, nullptr);
  }
  const int nout = 4 * thr.n + 3;
  acc.to_lds<true>(sm, thr.n, e);
  __syncthreads();
  if ((int)threadIdx.x < nout)
    part[((int64_t)blockIdx.x * gridDim.y + f) * nout + threadIdx.x] = (sm[0][threadIdx.x] + sm[1][threadIdx.x]) + (sm[2][threadIdx.x] + sm[3][threadIdx.x]);
}

// The accumulator block of a validation epoch (include/adnm_hip.h: adnm_valid_accum): 4 header doubles, then the (T, 4*nthr + 3) table.
constexpr int kValidHdr = 4;
constexpr int kFoldBlock = 256;

// One workgroup, fixed order, double arithmetic: row t of the table += sum over the samples b (ascending) of frame b*T + t's partials
// (blocks ascending); the batch loss = sum of every loss partial (lane-strided, then an LDS tree) / n, rounded to fp32.
__global__ __launch_bounds__(kFoldBlock) void valid_fold_kernel(const float* __restrict__ part, int nb, int frames, int T, int nthr, double inv_n,
                                                                double* __restrict__ blk, float* __restrict__ loss_out) {
  __shared__ double red[kFoldBlock];
  const int nin = 4 * nthr + 3, ncol = 4 * nthr + 3, B = frames / T;
  for (int i = threadIdx.x; i < T * (nin - 1); i += kFoldBlock) {
    const int t = i / (nin - 1), c = i % (nin - 1);
    double a = 0.0;
    for (int b = 0; b < B; ++b)
      for (int k = 0; k < nb; ++k) a += (double)part[((int64_t)k * frames + (b * T + t)) * nin + c];
    blk[kValidHdr + t * ncol + c] += a;
  }
  double e = 0.0;
  for (int64_t i = threadIdx.x; i < (int64_t)nb * frames; i += kFoldBlock) e += (double)part[i * nin + (nin - 1)];
  red[threadIdx.x] = e;
  __syncthreads();
  for (int o = kFoldBlock / 2; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float loss = (float)(red[0] * inv_n);
    if (adnm_nonfinite_bits(loss)) blk[3] += 1.0;
    else blk[0] += (double)loss;
    blk[1] += 1.0;
    blk[2] += (double)B;
    if (loss_out) *loss_out = loss;
  }
}

// part[tile][frame] (eval_ssim_kernel) -> column 4*nthr + 2 of row t += sum over the samples (ascending) of frame b*T + t's tiles (ascending)
__global__ __launch_bounds__(kFoldBlock) void valid_ssim_fold_kernel(const float* __restrict__ part, int tiles, int frames, int T, int nthr,
                                                                     double* __restrict__ blk) {
  const int ncol = 4 * nthr + 3, B = frames / T;
  for (int t = threadIdx.x; t < T; t += kFoldBlock) {
    double a = 0.0;
    for (int b = 0; b < B; ++b)
      for (int k = 0; k < tiles; ++k) a += (double)part[(int64_t)k * frames + (b * T + t)];
    blk[kValidHdr + t * ncol + 4 * nthr + 2] += a;
  }
}

// SSIM of SimplifiedEvaluator.cal_ssim (datasets/Shanghai_metrics.py:132-152): per frame, the mean over the VALID region of
//   ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)),   mu / s = 11x11 Gaussian (sigma 1.5) windowed moments of the
// value_scale'd clipped fields, computed in float64 as the reference does.  A workgroup = a 16 x 16 tile of output pixels of one frame: the
// 26 x 26 input patch of both fields is staged in LDS, the five moment maps are filtered separably (rows, then columns) through LDS, and the
// tile's sum of the SSIM map goes to part[frame][tile] for the shared fold.
constexpr int kSsimT = 16, kSsimR = 5, kSsimP = kSsimT + 2 * kSsimR;
struct GaussWin {
  double k[2 * kSsimR + 1];
};
__global__ __launch_bounds__(kSsimT * kSsimT) void eval_ssim_kernel(const float* __restrict__ truth, const float* __restrict__ pred, float* __restrict__ part,
                                                                  int H, int W, int tiles_x, int tiles, float value_scale, GaussWin g) {
  __shared__ double sp[kSsimP][kSsimP], st[kSsimP][kSsimP];   // pred, truth patches (scaled, clipped)
  __shared__ double sh[5][kSsimP][kSsimT];                     // row-filtered moments: p, t, p^2, t^2, p t
  __shared__ double red[kSsimT * kSsimT / 64];
  const int f = blockIdx.y, tile = blockIdx.x, ty0 = (tile / tiles_x) * kSsimT, tx0 = (tile % tiles_x) * kSsimT;
  const int Ho = H - 2 * kSsimR, Wo = W - 2 * kSsimR;
  const float* tp = truth + (int64_t)f * H * W;
  const float* pp = pred + (int64_t)f * H * W;
  for (int i = threadIdx.x; i < kSsimP * kSsimP; i += kSsimT * kSsimT) {
    const int r = i / kSsimP, c = i % kSsimP, y = ty0 + r, x = tx0 + c;   // input pixel of valid-output (ty0, tx0) + offset
    double a = 0.0, b = 0.0;
    if (y < H && x < W) {
      a = (double)(fminf(fmaxf(pp[(int64_t)y * W + x], 0.f), 1.f) * value_scale);   // float32 product (as numpy), then float64
      b = (double)(fminf(fmaxf(tp[(int64_t)y * W + x], 0.f), 1.f) * value_scale);
    }
    sp[r][c] = a, st[r][c] = b;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kSsimP * kSsimT; i += kSsimT * kSsimT) {
    const int r = i / kSsimT, c = i % kSsimT;
    double m[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j <= 2 * kSsimR; ++j) {
      const double a = sp[r][c + j], b = st[r][c + j], w = g.k[j];
      m[0] += w * a, m[1] += w * b, m[2] += w * a * a, m[3] += w * b * b, m[4] += w * a * b;
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) sh[q][r][c] = m[q];
  }
  __syncthreads();
  const int r = threadIdx.x / kSsimT, c = threadIdx.x % kSsimT;
  double v = 0.0;
  if (ty0 + r < Ho && tx0 + c < Wo) {
    double m[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j <= 2 * kSsimR; ++j)
#pragma unroll
      for (int q = 0; q < 5; ++q) m[q] += g.k[j] * sh[q][r + j][c];
    const double C1 = (0.01 * value_scale) * (0.01 * value_scale), C2 = (0.03 * value_scale) * (0.03 * value_scale);
    const double mu12 = m[0] * m[1], s1 = m[2] - m[0] * m[0], s2 = m[3] - m[1] * m[1], s12 = m[4] - mu12;
    v = ((2 * mu12 + C1) * (2 * s12 + C2)) / ((m[0] * m[0] + m[1] * m[1] + C1) * (s1 + s2 + C2));
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) part[(int64_t)tile * gridDim.y + f] = (float)((red[0] + red[1]) + (red[2] + red[3]));
}

inline int eval_blocks(int64_t hw) {
  int64_t b = adnm_cdiv(hw, kBlock * 16);
  return (int)(b < 1 ? 1 : (b > 64 ? 64 : b));
}
// the normalised sampled Gaussian cv2.getGaussianKernel(11, 1.5) documents
inline GaussWin gauss_window() {
  GaussWin g;
  double sum = 0.0;
  for (int j = 0; j <= 2 * kSsimR; ++j) sum += (g.k[j] = exp(-(double)((j - kSsimR) * (j - kSsimR)) / (2.0 * 1.5 * 1.5)));
  for (int j = 0; j <= 2 * kSsimR; ++j) g.k[j] /= sum;
  return g;
}
}  // namespace

extern "C" int adnm_radar_ingest(const void* src_u8, float* dst, int64_t frames, int64_t H0, int64_t W0, int64_t S, float mul, adnm_stream_t stream) {
  ADNM_REQUIRE(src_u8 && dst, "radar_ingest: null pointer");
  ADNM_REQUIRE(frames > 0 && H0 > 0 && W0 > 0 && S > 0 && H0 < 32768 && W0 < 32768 && S < 32768, "radar_ingest: bad shape");
  hipStream_t st = (hipStream_t)stream;
  const int64_t total = frames * S * S;
  ADNM_PROF("radar_ingest", st, (double)frames * H0 * W0 + 4.0 * total);
  radar_ingest_kernel<<<(unsigned)adnm_cdiv(total, kBlock), kBlock, 0, st>>>((const uint8_t*)src_u8, dst, frames, (int)H0, (int)W0, (int)S, (float)H0 / (float)S,
                                                                            (float)W0 / (float)S, mul);
  ADNM_CHECK_LAUNCH("radar_ingest");
  return ADNM_OK;
}

// ---- the resident split: one batch out of the store (include/adnm_hip.h: adnm_batch_fetch) ----
namespace {
constexpr int kFetchUnroll = 4;       // pieces a lane keeps in flight per trip
constexpr int kFetchMaxBlocks = 2048; // workgroups of a launch, all samples together (a streaming grid: the rest is grid-strided)
constexpr int64_t kFetchMaxBatch = 65535;

// gridDim.y = the batch: a workgroup stays inside sample b = blockIdx.y, whose index order[pos + b] is one uniform load.  An index
// outside [0, n_samples) is never turned into an address: the sample's rows are filled with quiet NaNs instead (a uniform branch).
// V = float4: `per` (= T*hw) and `split` (= T_in*hw) count 16-byte pieces, so that no piece straddles the x / tgt boundary; V = float:
// they count floats.  A lane's pieces lie `stride` apart; it loads kFetchUnroll of them before it stores the first, then the ragged rest
// one by one.
__device__ __forceinline__ void fetch_nan(float& v) { v = __int_as_float(0x7fc00000); }
__device__ __forceinline__ void fetch_nan(float4& v) { v.x = v.y = v.z = v.w = __int_as_float(0x7fc00000); }

template <typename V>
__global__ __launch_bounds__(kBlock) void batch_fetch_kernel(const V* __restrict__ store, const int32_t* __restrict__ order, int64_t pos, int n_samples,
                                                             int64_t per, int64_t split, V* __restrict__ x, V* __restrict__ tgt) {
  const int64_t b = blockIdx.y;
  const int s = order[pos + b];
  V* dx = x + b * split;
  V* dt = tgt + b * (per - split) - split;   // piece i >= split of the sample -> dt[i]
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (s < 0 || s >= n_samples) {
    V nan;
    fetch_nan(nan);
    for (; i < per; i += stride) (i < split ? dx : dt)[i] = nan;
    return;
  }
  const V* src = store + (int64_t)s * per;
  for (; i + (kFetchUnroll - 1) * stride < per; i += kFetchUnroll * stride) {
    V v[kFetchUnroll];
#pragma unroll
    for (int k = 0; k < kFetchUnroll; ++k) v[k] = src[i + k * stride];
#pragma unroll
    for (int k = 0; k < kFetchUnroll; ++k) (i + k * stride < split ? dx : dt)[i + k * stride] = v[k];
  }
  for (; i < per; i += stride) (i < split ? dx : dt)[i] = src[i];
}
}  // namespace

extern "C" int adnm_batch_fetch(const float* store, int64_t n_samples, int64_t T, int64_t hw, const int32_t* order, int64_t order_len, int64_t pos, float* x,
                                float* tgt, int64_t B, int64_t T_in, adnm_stream_t stream) {
  ADNM_REQUIRE(store && order && x && tgt, "batch_fetch: null pointer");
  ADNM_REQUIRE(((uintptr_t)store | (uintptr_t)order | (uintptr_t)x | (uintptr_t)tgt) % 4 == 0, "batch_fetch: store, order, x and tgt must be 4-byte aligned");
  ADNM_REQUIRE(B >= 1 && B <= kFetchMaxBatch, "batch_fetch: the batch must be in [1, %lld] (one grid row per sample), got %lld", (long long)kFetchMaxBatch, (long long)B);
  ADNM_REQUIRE(hw >= 1 && hw < (1ll << 31) && T < (1ll << 31), "batch_fetch: bad shape (1 <= hw < 2^31, T < 2^31), got T %lld hw %lld", (long long)T, (long long)hw);
  ADNM_REQUIRE(T_in >= 1 && T_in < T, "batch_fetch: T_in must be in [1, T), got T_in %lld of T %lld", (long long)T_in, (long long)T);
  ADNM_REQUIRE(n_samples >= 1 && n_samples < (1ll << 31) && order_len >= 1 && order_len < (1ll << 31),
               "batch_fetch: n_samples and order_len must be in [1, 2^31), got %lld and %lld", (long long)n_samples, (long long)order_len);
  ADNM_REQUIRE(pos >= 0 && pos <= order_len - B, "batch_fetch: %lld positions from %lld on lie outside an order of %lld", (long long)B, (long long)pos,
               (long long)order_len);
  const int64_t per = T * hw, split = T_in * hw;
  // 16-byte accesses need every sample start in the store (stride `per`), both halves' starts in x and tgt (strides `split`, `per - split`)
  // and the three bases aligned; anything else (an odd S, a 4-byte aligned slice of a larger buffer) takes the scalar path: same result
  const bool vec = per % 4 == 0 && split % 4 == 0 && adnm_quad_aligned(ADNM_F32, {store, x, tgt});
  const int64_t units = vec ? per / 4 : per;
  int64_t gx = adnm_cdiv(units, (int64_t)kBlock * kFetchUnroll), cap = kFetchMaxBlocks / B;
  cap = cap < 1 ? 1 : cap;
  gx = gx > cap ? cap : gx;
  hipStream_t st = (hipStream_t)stream;
  {
    ADNM_PROF("batch_fetch", st, 8.0 * B * T * hw);
    if (vec)
      batch_fetch_kernel<float4><<<dim3((unsigned)gx, (unsigned)B), kBlock, 0, st>>>((const float4*)store, order, pos, (int)n_samples, per / 4, split / 4,
                                                                                     (float4*)x, (float4*)tgt);
    else
      batch_fetch_kernel<float><<<dim3((unsigned)gx, (unsigned)B), kBlock, 0, st>>>(store, order, pos, (int)n_samples, per, split, x, tgt);
  }
  ADNM_CHECK_LAUNCH("batch_fetch");
  return ADNM_OK;
}

// ---- the resident split, augmented: a window of the stored frame under one of the square's symmetries (adnm_batch_fetch_aug) ----
namespace {
constexpr int kAugTile = 32;             // the transposing path's LDS tile: kAugTile x (kAugTile + 1) floats
constexpr int64_t kAugMaxSide = 16384;   // oy and ox are 14-bit fields of the word

struct AugGeom {
  int T, T_in, H, W, Hs, Ws;
};

__device__ __forceinline__ float aug_reversed(float v) { return v; }
__device__ __forceinline__ float4 aug_reversed(float4 v) { return make_float4(v.w, v.z, v.y, v.x); }

// Without the transpose bit an output row is a row of the window, possibly read from its far end.  V = float4: W, Ws and the window's
// ox are multiples of 4, so that every row piece is a 16-byte access on both sides (a reversed row takes its pieces from the far end
// and swaps the components inside each).  The output of a sample is contiguous, so piece i goes where batch_fetch_kernel puts it; only
// the source address needs (t, y, c).  win: the window's origin in frame 0 of the sample.  All indices fit 32 bits (the host refuses
// T*Hs*Ws >= 2^31).
template <typename V>
__device__ __forceinline__ void aug_rows(const float* __restrict__ win, float* __restrict__ dx, float* __restrict__ dt, const AugGeom& g, bool flip_lr,
                                         bool flip_ud) {
  constexpr uint32_t E = sizeof(V) / sizeof(float);
  const uint32_t wv = (uint32_t)g.W / E, H = (uint32_t)g.H, units = (uint32_t)g.T * H * wv, split = (uint32_t)g.T_in * H * wv;
  const uint32_t stride = gridDim.x * kBlock, fs = (uint32_t)g.Hs * (uint32_t)g.Ws;
  V* ox_ = (V*)dx;
  V* ot_ = (V*)dt;   // dt is `split` pieces before the sample's target rows: piece i >= split -> ot_[i]
  uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  // (t, y, c) of piece i: two divisions per lane here, none per piece.  A step of `stride` pieces is (dt, dy, dc) with carries, and
  // the step's own split is uniform.  The three always belong to i, and nothing is loaded for an i >= units.
  const uint32_t dr = stride / wv, dc = stride - dr * wv, dt_ = dr / H, dy = dr - dt_ * H;
  uint32_t row = i / wv, c = i - row * wv, t = row / H, y = row - t * H;
  auto load_and_step = [&]() {
    const uint32_t sy = flip_ud ? H - 1 - y : y, sc = flip_lr ? wv - 1 - c : c;
    const V v = *(const V*)(win + (t * fs + sy * (uint32_t)g.Ws + sc * E));
    c += dc;
    const bool cc = c >= wv;      // c < 2 wv
    c -= cc ? wv : 0u;
    y += dy + (cc ? 1u : 0u);
    const bool cy = y >= H;       // y <= (H - 1) + (H - 1) + 1 < 2 H
    y -= cy ? H : 0u;
    t += dt_ + (cy ? 1u : 0u);
    return flip_lr ? aug_reversed(v) : v;
  };
  for (; (uint64_t)i + (uint64_t)(kFetchUnroll - 1) * stride < units; i += kFetchUnroll * stride) {
    V v[kFetchUnroll];
#pragma unroll
    for (int k = 0; k < kFetchUnroll; ++k) v[k] = load_and_step();
#pragma unroll
    for (int k = 0; k < kFetchUnroll; ++k) (i + k * stride < split ? ox_ : ot_)[i + k * stride] = v[k];
  }
  for (; i < units; i += stride) (i < split ? ox_ : ot_)[i] = load_and_step();
}

// With the transpose bit (H == W = n) output rows are source columns:  out[t][r][c] = window[t][fy(c)][fx(r)],  fy / fx the flips.  A
// workgroup takes 32 x 32 output tiles.  Loading, lane lx runs along the SOURCE row (consecutive or, flipped, descending addresses: one
// 128-byte line per 32 lanes) and writes tile[ly][lx]; storing, lane lx runs along the OUTPUT row and reads tile[lx][ly].  Rows are 33
// dwords apart, so both the row writes (banks lx + const) and the column reads (banks 33 lx + const = lx + const mod 32) of a 32-lane
// half touch 32 different banks.  Ragged tiles at the right and bottom edges skip what lies outside.
__device__ __forceinline__ void aug_transposed(const float* __restrict__ win, float* __restrict__ dx, float* __restrict__ dt, const AugGeom& g, bool flip_lr,
                                               bool flip_ud, float (*tile)[kAugTile + 1]) {
  constexpr int kRows = kBlock / kAugTile;   // tile rows a pass of the workgroup covers
  const int n = g.H, side = (n + kAugTile - 1) / kAugTile, tiles = g.T * side * side;
  const int lx = threadIdx.x % kAugTile, ly = threadIdx.x / kAugTile;
  const int64_t fs = (int64_t)g.Hs * g.Ws, split = (int64_t)g.T_in * n * n;
  for (int u = blockIdx.x; u < tiles; u += gridDim.x) {   // the same trips for every lane: the barriers below see the whole workgroup
    const int t = u / (side * side), q = u - t * side * side, r0 = (q / side) * kAugTile, c0 = (q % side) * kAugTile;
    const float* sp = win + t * fs;
    const int sr = r0 + lx;   // the output ROW this lane loads for: its source column is fx(sr)
    float v[kAugTile / kRows];
#pragma unroll
    for (int k = 0; k < kAugTile / kRows; ++k) {
      const int sc = c0 + ly + k * kRows;   // the output COLUMN: its source row is fy(sc)
      v[k] = 0.f;
      if (sr < n && sc < n) v[k] = sp[(int64_t)(flip_ud ? n - 1 - sc : sc) * g.Ws + (flip_lr ? n - 1 - sr : sr)];
    }
#pragma unroll
    for (int k = 0; k < kAugTile / kRows; ++k) tile[ly + k * kRows][lx] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kAugTile / kRows; ++k) {
      const int r = r0 + ly + k * kRows, c = c0 + lx;
      if (r < n && c < n) {
        const int64_t e = ((int64_t)t * n + r) * n + c;
        (e < split ? dx : dt)[e] = tile[lx][ly + k * kRows];
      }
    }
    __syncthreads();   // the next tile rewrites what this one still reads
  }
}

// gridDim.y = the batch, as batch_fetch_kernel: index s = order[pos + b] and word a = aug[pos + b] are two uniform loads, and every
// branch below is taken by a whole workgroup.  A sample that must not be served (see include/adnm_hip.h) is filled with quiet NaNs
// before anything of it is turned into an address.  can_vec: what the 16-byte path needs of the LAUNCH (W and Ws multiples of 4, the
// three bases aligned); the sample adds ox % 4 == 0.
__global__ __launch_bounds__(kBlock) void batch_fetch_aug_kernel(const float* __restrict__ store, const int32_t* __restrict__ order,
                                                                 const int32_t* __restrict__ aug, int64_t pos, int n_samples, AugGeom g, int can_vec,
                                                                 float* __restrict__ x, float* __restrict__ tgt) {
  __shared__ float tile[kAugTile][kAugTile + 1];
  const int64_t b = blockIdx.y;
  const int s = order[pos + b];
  const uint32_t a = (uint32_t)aug[pos + b];
  const bool flip_lr = a & 1u, flip_ud = a & 2u, transpose = a & 4u;
  const int oy = (int)((a >> 3) & 0x3fffu), ox = (int)((a >> 17) & 0x3fffu);
  const int64_t hw = (int64_t)g.H * g.W, per = g.T * hw, split = g.T_in * hw;
  float* dx = x + b * split;
  float* dt = tgt + b * (per - split) - split;   // element i >= split of the sample -> dt[i]
  if (s < 0 || s >= n_samples || (a >> 31) || oy + g.H > g.Hs || ox + g.W > g.Ws || (transpose && g.H != g.W)) {
    float nan;
    fetch_nan(nan);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < per; i += (int64_t)gridDim.x * kBlock) (i < split ? dx : dt)[i] = nan;
    return;
  }
  const float* win = store + (int64_t)s * g.T * g.Hs * g.Ws + (int64_t)oy * g.Ws + ox;
  if (transpose) aug_transposed(win, dx, dt, g, flip_lr, flip_ud, tile);
  else if (can_vec && ox % 4 == 0) aug_rows<float4>(win, dx, dt, g, flip_lr, flip_ud);
  else aug_rows<float>(win, dx, dt, g, flip_lr, flip_ud);
}
}  // namespace

extern "C" int adnm_batch_fetch_aug(const float* store, int64_t n_samples, int64_t T, int64_t Hs, int64_t Ws, const int32_t* order, const int32_t* aug,
                                    int64_t order_len, int64_t pos, float* x, float* tgt, int64_t B, int64_t T_in, int64_t H, int64_t W,
                                    adnm_stream_t stream) {
  ADNM_REQUIRE(store && order && aug && x && tgt, "batch_fetch_aug: null pointer");
  ADNM_REQUIRE(((uintptr_t)store | (uintptr_t)order | (uintptr_t)aug | (uintptr_t)x | (uintptr_t)tgt) % 4 == 0,
               "batch_fetch_aug: store, order, aug, x and tgt must be 4-byte aligned");
  ADNM_REQUIRE(B >= 1 && B <= kFetchMaxBatch, "batch_fetch_aug: the batch must be in [1, %lld] (one grid row per sample), got %lld", (long long)kFetchMaxBatch,
               (long long)B);
  ADNM_REQUIRE(H >= 1 && H < kAugMaxSide && W >= 1 && W < kAugMaxSide && Hs >= 1 && Hs < kAugMaxSide && Ws >= 1 && Ws < kAugMaxSide,
               "batch_fetch_aug: H, W, Hs and Ws must be in [1, 16384) (the word's offsets are 14-bit fields), got %lld x %lld of %lld x %lld", (long long)H,
               (long long)W, (long long)Hs, (long long)Ws);
  ADNM_REQUIRE(H <= Hs && W <= Ws, "batch_fetch_aug: the served frame %lld x %lld is larger than the stored one, %lld x %lld", (long long)H, (long long)W,
               (long long)Hs, (long long)Ws);
  ADNM_REQUIRE(T >= 1 && T < (1ll << 31) && T * Hs * Ws < (1ll << 31),"batch_fetch_aug: a stored sample must hold fewer than 2^31 floats, got T %lld of %lld x %lld",
               (long long)T, (long long)Hs, (long long)Ws);
  ADNM_REQUIRE(T_in >= 1 && T_in < T, "batch_fetch_aug: T_in must be in [1, T), got T_in %lld of T %lld", (long long)T_in, (long long)T);
  ADNM_REQUIRE(n_samples >= 1 && n_samples < (1ll << 31) && order_len >= 1 && order_len < (1ll << 31),
               "batch_fetch_aug: n_samples and order_len must be in [1, 2^31), got %lld and %lld", (long long)n_samples, (long long)order_len);
  ADNM_REQUIRE(pos >= 0 && pos <= order_len - B, "batch_fetch_aug: %lld positions from %lld on lie outside an order of %lld", (long long)B, (long long)pos,
               (long long)order_len);
  const int64_t per = T * H * W;
  // what the 16-byte path needs of the launch: every row start on both sides (W, Ws multiples of 4, hence the frame strides, the sample
  // strides and the x / tgt split as well) and the three bases; a sample adds ox % 4 == 0 in the kernel
  const bool can_vec = W % 4 == 0 && Ws % 4 == 0 && adnm_quad_aligned(ADNM_F32, {store, x, tgt});
  const int64_t units = can_vec ? per / 4 : per;
  int64_t gx = adnm_cdiv(units, (int64_t)kBlock * kFetchUnroll), cap = kFetchMaxBlocks / B;
  cap = cap < 1 ? 1 : cap;
  gx = gx > cap ? cap : gx;
  const AugGeom g = {(int)T, (int)T_in, (int)H, (int)W, (int)Hs, (int)Ws};
  hipStream_t st = (hipStream_t)stream;
  {
    ADNM_PROF("batch_fetch_aug", st, 8.0 * B * per);
    batch_fetch_aug_kernel<<<dim3((unsigned)gx, (unsigned)B), kBlock, 0, st>>>(store, order, aug, pos, (int)n_samples, g, can_vec ? 1 : 0, x, tgt);
  }
  ADNM_CHECK_LAUNCH("batch_fetch_aug");
  return ADNM_OK;
}

extern "C" int64_t adnm_eval_counts_ws_bytes(int64_t frames, int64_t hw, int64_t nthr) {
  if (frames <= 0 || hw <= 0 || nthr <= 0 || nthr > kMaxThr) return 0;
  return (int64_t)eval_blocks(hw) * frames * (4 * nthr + 2) * (int64_t)sizeof(float);
}

// out: (frames, 4*nthr + 2) fp32 = [TP, FN, FP, TN] per threshold, then sum |d|, sum d^2 of the value_scale'd clipped fields.  OVERWRITES out.
extern "C" int adnm_eval_counts(const float* truth, const float* pred, float* out, const float* thresholds_host, int64_t nthr, float value_scale,
                                void* ws, int64_t ws_bytes, int64_t frames, int64_t hw, adnm_stream_t stream) {
  ADNM_REQUIRE(truth && pred && out && thresholds_host, "eval_counts: null pointer");
  ADNM_REQUIRE(frames > 0 && frames <= 65535 && hw > 0 && hw < (1ll << 24) && nthr > 0 && nthr <= kMaxThr,
               "eval_counts: bad shape (frames <= 65535, pixels per frame < 2^24 so that counts are exact in fp32, <= 8 thresholds)");
  if (!ws || ws_bytes < adnm_eval_counts_ws_bytes(frames, hw, nthr)) {
    adnm_set_error("eval_counts: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)adnm_eval_counts_ws_bytes(frames, hw, nthr));
    return ADNM_EWORKSPACE;
  }
  const Thr thr = thr_fill(thresholds_host, nthr);
  hipStream_t st = (hipStream_t)stream;
  const int nb = eval_blocks(hw), nout = 4 * (int)nthr + 2;
  {
    ADNM_PROF("eval_counts", st, 8.0 * frames * hw);
    eval_counts_kernel<<<dim3(nb, (unsigned)frames), kBlock, 0, st>>>(truth, pred, (float*)ws, hw, value_scale, thr);
  }
  ADNM_CHECK_LAUNCH("eval_counts");
  adnm_launch_fold("eval_counts_fold", (const float*)ws, nb, (int)(frames * nout), {out, (int)(frames * nout)}, {nullptr, 0}, {nullptr, 0}, {nullptr, 0}, st);
  ADNM_CHECK_LAUNCH("eval_counts_fold");
  return ADNM_OK;
}


extern "C" int64_t adnm_eval_ssim_ws_bytes(int64_t frames, int64_t H, int64_t W) {
  if (frames <= 0 || H <= 2 * kSsimR || W <= 2 * kSsimR) return 0;
  return adnm_cdiv(H - 2 * kSsimR, kSsimT) * adnm_cdiv(W - 2 * kSsimR, kSsimT) * frames * (int64_t)sizeof(float);
}

// out[frame] = SUM of the SSIM map of frame `frame` over its (H - 10) x (W - 10) valid region (SimplifiedEvaluator.cal_ssim,
// datasets/Shanghai_metrics.py:132-152, takes the mean: the caller divides) on the [0,1]-clipped, value_scale'd fields.  OVERWRITES out.
extern "C" int adnm_eval_ssim(const float* truth, const float* pred, float* out, float value_scale, void* ws, int64_t ws_bytes, int64_t frames, int64_t H,
                              int64_t W, adnm_stream_t stream) {
  ADNM_REQUIRE(truth && pred && out, "eval_ssim: null pointer");
  ADNM_REQUIRE(frames > 0 && frames <= 65535 && H > 2 * kSsimR && W > 2 * kSsimR && H < 32768 && W < 32768,
               "eval_ssim: needs frames of more than 10 x 10 pixels (11 x 11 window, valid region), got %lld x %lld", (long long)H, (long long)W);
  if (!ws || ws_bytes < adnm_eval_ssim_ws_bytes(frames, H, W)) {
    adnm_set_error("eval_ssim: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)adnm_eval_ssim_ws_bytes(frames, H, W));
    return ADNM_EWORKSPACE;
  }
  const GaussWin g = gauss_window();
  const int tx = (int)adnm_cdiv(W - 2 * kSsimR, kSsimT), ty = (int)adnm_cdiv(H - 2 * kSsimR, kSsimT);
  hipStream_t st = (hipStream_t)stream;
  {
    ADNM_PROF("eval_ssim", st, 8.0 * frames * H * W);
    eval_ssim_kernel<<<dim3((unsigned)(tx * ty), (unsigned)frames), kSsimT * kSsimT, 0, st>>>(truth, pred, (float*)ws, (int)H, (int)W, tx, tx * ty, value_scale, g);
  }
  ADNM_CHECK_LAUNCH("eval_ssim");
  adnm_launch_fold("eval_ssim_fold", (const float*)ws, tx * ty, (int)frames, {out, (int)frames}, {nullptr, 0}, {nullptr, 0}, {nullptr, 0}, st);
  ADNM_CHECK_LAUNCH("eval_ssim_fold");
  return ADNM_OK;
}


// ---- the validation epoch: accumulate on the device (include/adnm_hip.h) ----
namespace {
bool valid_shape_ok(int64_t frames, int64_t T, int64_t hw, int64_t nthr) {
  return frames > 0 && frames <= 65535 && T >= 1 && frames % T == 0 && hw > 0 && hw < (1ll << 24) && nthr >= 1 && nthr <= kMaxThr;
}
}  // namespace

extern "C" int64_t adnm_valid_block_bytes(int64_t T, int64_t nthr) {
  if (T < 1 || T > 65535 || nthr < 1 || nthr > kMaxThr) return -1;
  return (int64_t)sizeof(double) * (kValidHdr + T * (4 * nthr + 3));
}

extern "C" int64_t adnm_valid_accum_ws_bytes(int64_t frames, int64_t T, int64_t hw, int64_t nthr) {
  if (!valid_shape_ok(frames, T, hw, nthr)) return -1;
  return (int64_t)eval_blocks(hw) * frames * (4 * nthr + 3) * (int64_t)sizeof(float);
}

extern "C" int adnm_valid_accum(const float* pred, const float* target, void* block, float* loss_out, const float* thresholds_host, int64_t nthr,
                                float value_scale, float omega_t, float alpha, float gamma, void* ws, int64_t ws_bytes, int64_t frames, int64_t T,
                                int64_t hw, adnm_stream_t stream) {
  ADNM_REQUIRE(pred && target && block && thresholds_host, "valid_accum: null pointer");
  ADNM_REQUIRE((uintptr_t)block % 8 == 0, "valid_accum: the accumulator block must be 8-byte aligned");
  ADNM_REQUIRE(valid_shape_ok(frames, T, hw, nthr),
               "valid_accum: bad shape (frames <= 65535, T >= 1 dividing frames, pixels per frame < 2^24, 1..8 thresholds), got frames %lld T %lld hw %lld "
               "nthr %lld", (long long)frames, (long long)T, (long long)hw, (long long)nthr);
  if (!ws || ws_bytes < adnm_valid_accum_ws_bytes(frames, T, hw, nthr)) {
    adnm_set_error("valid_accum: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)adnm_valid_accum_ws_bytes(frames, T, hw, nthr));
    return ADNM_EWORKSPACE;
  }
  const Thr thr = thr_fill(thresholds_host, nthr);
  hipStream_t st = (hipStream_t)stream;
  const int nb = eval_blocks(hw);
  {
    ADNM_PROF("valid_accum", st, 8.0 * frames * hw);
    valid_accum_kernel<<<dim3(nb, (unsigned)frames), kBlock, 0, st>>>(pred, target, (float*)ws, hw, value_scale, thr, omega_t, alpha, gamma);
  }
  ADNM_CHECK_LAUNCH("valid_accum");
  {
    ADNM_PROF("valid_accum_fold", st, 4.0 * nb * frames * (4 * nthr + 3));
    valid_fold_kernel<<<1, kFoldBlock, 0, st>>>((const float*)ws, nb, (int)frames, (int)T, (int)nthr, 1.0 / ((double)frames * (double)hw), (double*)block,
                                                loss_out);
  }
  ADNM_CHECK_LAUNCH("valid_accum_fold");
  return ADNM_OK;
}

extern "C" int64_t adnm_valid_ssim_accum_ws_bytes(int64_t frames, int64_t T, int64_t H, int64_t W, int64_t nthr) {
  if (H <= 2 * kSsimR || W <= 2 * kSsimR || H >= 32768 || W >= 32768 || !valid_shape_ok(frames, T, H * W, nthr)) return -1;
  return adnm_eval_ssim_ws_bytes(frames, H, W);
}

extern "C" int adnm_valid_ssim_accum(const float* pred, const float* target, void* block, int64_t nthr, float value_scale, void* ws, int64_t ws_bytes,
                                     int64_t frames, int64_t T, int64_t H, int64_t W, adnm_stream_t stream) {
  ADNM_REQUIRE(pred && target && block, "valid_ssim_accum: null pointer");
  ADNM_REQUIRE((uintptr_t)block % 8 == 0, "valid_ssim_accum: the accumulator block must be 8-byte aligned");
  ADNM_REQUIRE(H > 2 * kSsimR && W > 2 * kSsimR && H < 32768 && W < 32768,
               "valid_ssim_accum: needs frames of more than 10 x 10 pixels (11 x 11 window, valid region), got %lld x %lld", (long long)H, (long long)W);
  ADNM_REQUIRE(valid_shape_ok(frames, T, H * W, nthr),
               "valid_ssim_accum: bad shape (frames <= 65535, T >= 1 dividing frames, pixels per frame < 2^24, 1..8 thresholds), got frames %lld T %lld "
               "%lld x %lld nthr %lld", (long long)frames, (long long)T, (long long)H, (long long)W, (long long)nthr);
  if (!ws || ws_bytes < adnm_valid_ssim_accum_ws_bytes(frames, T, H, W, nthr)) {
    adnm_set_error("valid_ssim_accum: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)adnm_valid_ssim_accum_ws_bytes(frames, T, H, W, nthr));
    return ADNM_EWORKSPACE;
  }
  const GaussWin g = gauss_window();
  const int tx = (int)adnm_cdiv(W - 2 * kSsimR, kSsimT), ty = (int)adnm_cdiv(H - 2 * kSsimR, kSsimT);
  hipStream_t st = (hipStream_t)stream;
  {
    ADNM_PROF("valid_ssim", st, 8.0 * frames * H * W);
    eval_ssim_kernel<<<dim3((unsigned)(tx * ty), (unsigned)frames), kSsimT * kSsimT, 0, st>>>(target, pred, (float*)ws, (int)H, (int)W, tx, tx * ty, value_scale, g);
  }
  ADNM_CHECK_LAUNCH("valid_ssim_accum");
  {
    ADNM_PROF("valid_ssim_fold", st, 4.0 * tx * ty * frames);
    valid_ssim_fold_kernel<<<1, kFoldBlock, 0, st>>>((const float*)ws, tx * ty, (int)frames, (int)T, (int)nthr, (double*)block);
  }
  ADNM_CHECK_LAUNCH("valid_ssim_fold");
  return ADNM_OK;
}


// ---- the output side: forecast fields and colour strips (include/adnm_hip.h: adnm_forecast_render) ----
namespace {
constexpr int kMaxBins = 32;
// edges and colours travel by value in the kernarg segment: every lane's edge loads are uniform, and nothing on the device has to outlive the call
struct RenderTab {
  float bounds[kMaxBins + 1];
  uint32_t rgba[kMaxBins];   // R | G << 8 | B << 16 | A << 24: the dword whose bytes in memory are R, G, B, A
  int n;
};

// the value rule of one pixel -> the byte for `fields`, the RGBA dword for `strip`
__device__ __forceinline__ void render_pixel(float p, float pixel_scale, const RenderTab& tab, uint32_t& byte, uint32_t& colour) {
  float v = p;
  if (pixel_scale > 0.f) {
    const float prod = __fmul_rn(p, pixel_scale);            // the fp32 product on its own, as numpy forms it (never contracted)
    const float c = fminf(fmaxf(prod, 0.f), 255.f);          // fmaxf(NaN, 0) = 0
    byte = (uint32_t)(int)c;                                 // truncation toward zero
    v = (float)byte;
  }
  int cnt = 0;
#pragma unroll
  for (int k = 0; k <= kMaxBins; ++k) cnt += (k <= tab.n && tab.bounds[k] <= v) ? 1 : 0;   // NaN: no edge is <= it
  int idx = cnt - 1;
  idx = idx < 0 ? 0 : (idx > tab.n - 1 ? tab.n - 1 : idx);
  colour = tab.rgba[idx];
  if (!(pixel_scale > 0.f)) {
    byte = (uint32_t)idx;
    if (v != v) colour = 0u;                                 // matplotlib's "bad" colour
  }
}

// A lane owns up to 4 consecutive pixels of one row of one frame: lane i -> group q = i % Q of row i / Q, Q = ceil(W / 4).
// VEC (W % 4 == 0, pred 16-byte and fields 4-byte aligned): one 16-byte load, one packed dword store to fields.  The strip is written
// pixel by pixel as dwords: a frame's origin in a strip row is 4 * j * (W + gap) bytes, which is 16-byte aligned only when
// (W + gap) % 4 == 0 (W = 128, gap = 10: 552 * j).  The gap behind a selected frame (all but the last) is written by that frame's
// lanes of the same row, lane q taking the gap pixels q, q + Q, ...
template <bool VEC>
__global__ __launch_bounds__(kBlock) void forecast_render_kernel(const float* __restrict__ pred, uint8_t* __restrict__ fields, uint32_t* __restrict__ strip,
                                                                 RenderTab tab, float pixel_scale, int64_t lanes, int T, int H, int W, int Q, int frame_start,
                                                                 int frame_step, int nsel, int gap, int64_t strip_w) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= lanes) return;
  const int q = (int)(i % Q);
  const int64_t row = i / Q;                     // (b * T + t) * H + y
  const int y = (int)(row % H);
  const int64_t ft = row / H;
  const int t = (int)(ft % T);
  const int64_t b = ft / T;
  const int x0 = 4 * q, npx = W - x0 < 4 ? W - x0 : 4;
  const int64_t src = row * W + x0;
  float p[4] = {0.f, 0.f, 0.f, 0.f};
  if (VEC) {
    const float4 v = *reinterpret_cast<const float4*>(pred + src);
    p[0] = v.x, p[1] = v.y, p[2] = v.z, p[3] = v.w;
  } else {
    for (int k = 0; k < npx; ++k) p[k] = pred[src + k];
  }
  uint32_t byte[4] = {0u, 0u, 0u, 0u}, colour[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < npx) render_pixel(p[k], pixel_scale, tab, byte[k], colour[k]);
  if (fields) {
    if (VEC) *reinterpret_cast<uint32_t*>(fields + src) = byte[0] | (byte[1] << 8) | (byte[2] << 16) | (byte[3] << 24);
    else
      for (int k = 0; k < npx; ++k) fields[src + k] = (uint8_t)byte[k];
  }
  if (strip && t >= frame_start && (t - frame_start) % frame_step == 0) {
    const int j = (t - frame_start) / frame_step;
    uint32_t* dst = strip + ((b * H + y) * strip_w + (int64_t)j * (W + gap));
    for (int k = 0; k < npx; ++k) dst[x0 + k] = colour[k];
    if (j < nsel - 1)
      for (int g = q; g < gap; g += Q) dst[W + g] = 0xffffffffu;
  }
}
}  // namespace

extern "C" int adnm_forecast_render(const float* pred, uint8_t* fields, uint8_t* strip, const float* bounds_host, const uint8_t* palette_host, int64_t nbins,
                                    float pixel_scale, int64_t B, int64_t T, int64_t H, int64_t W, int64_t frame_start, int64_t frame_step, int64_t gap,
                                    adnm_stream_t stream) {
  ADNM_REQUIRE(pred && bounds_host && palette_host, "forecast_render: null pointer");
  ADNM_REQUIRE(fields || strip, "forecast_render: no output (fields and strip are both NULL)");
  ADNM_REQUIRE(nbins >= 1 && nbins <= kMaxBins, "forecast_render: 1..32 bins, got %lld", (long long)nbins);
  for (int64_t k = 0; k <= nbins; ++k)
    ADNM_REQUIRE(isfinite(bounds_host[k]) && (k == 0 || bounds_host[k] > bounds_host[k - 1]), "forecast_render: the %lld edges must be finite and ascending (edge %lld)",
                 (long long)(nbins + 1), (long long)k);
  ADNM_REQUIRE(pixel_scale >= 0.f && isfinite(pixel_scale), "forecast_render: pixel_scale must be finite and >= 0 (0: bin the float value itself)");
  ADNM_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0 && B < (1ll << 31) && T < (1ll << 31) && H < (1ll << 31) && W < (1ll << 31) &&
                   (double)B * (double)T * (double)H * (double)W < 2147483648.0,
               "forecast_render: bad shape (B, T, H, W >= 1, B*T*H*W < 2^31), got %lld %lld %lld %lld", (long long)B, (long long)T, (long long)H, (long long)W);
  ADNM_REQUIRE(frame_start >= 0 && frame_start < T, "forecast_render: frame_start %lld outside the %lld frames", (long long)frame_start, (long long)T);
  ADNM_REQUIRE(frame_step >= 1 && frame_step < (1ll << 31), "forecast_render: frame_step must be >= 1, got %lld", (long long)frame_step);
  ADNM_REQUIRE(gap >= 0 && gap < (1ll << 24), "forecast_render: gap must be in [0, 2^24), got %lld", (long long)gap);
  const int64_t nsel = adnm_cdiv(T - frame_start, frame_step);
  const int64_t strip_w = nsel * W + (nsel - 1) * gap;
  ADNM_REQUIRE((uintptr_t)pred % 4 == 0, "forecast_render: pred must be 4-byte aligned");
  if (strip) {   // a fields-only call is not held to the strip's limits
    ADNM_REQUIRE(strip_w < (1ll << 24), "forecast_render: the strip would be %lld pixels wide (limit 2^24)", (long long)strip_w);
    ADNM_REQUIRE((uintptr_t)strip % 4 == 0, "forecast_render: strip must be 4-byte aligned");
  }
  RenderTab tab;
  tab.n = (int)nbins;
  for (int k = 0; k <= kMaxBins; ++k) tab.bounds[k] = k <= nbins ? bounds_host[k] : 0.f;
  for (int k = 0; k < kMaxBins; ++k) {
    const uint8_t* c = palette_host + 4 * (k < nbins ? k : 0);
    tab.rgba[k] = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24);
  }
  const int Q = (int)adnm_cdiv(W, 4);
  const int64_t lanes = B * T * H * Q;
  const bool vec = W % 4 == 0 && (uintptr_t)pred % 16 == 0 && (uintptr_t)fields % 4 == 0;
  hipStream_t st = (hipStream_t)stream;
  {
    ADNM_PROF("forecast_render", st, (double)B * T * H * W * (4.0 + (fields ? 1.0 : 0.0)) + (strip ? 4.0 * B * H * strip_w : 0.0));
    const unsigned blocks = (unsigned)adnm_cdiv(lanes, kBlock);
    if (vec)
      forecast_render_kernel<true><<<blocks, kBlock, 0, st>>>(pred, fields, (uint32_t*)strip, tab, pixel_scale, lanes, (int)T, (int)H, (int)W, Q, (int)frame_start,
                                                              (int)frame_step, (int)nsel, (int)gap, strip_w);
    else
      forecast_render_kernel<false><<<blocks, kBlock, 0, st>>>(pred, fields, (uint32_t*)strip, tab, pixel_scale, lanes, (int)T, (int)H, (int)W, Q, (int)frame_start,
                                                               (int)frame_step, (int)nsel, (int)gap, strip_w);
  }
  ADNM_CHECK_LAUNCH("forecast_render");
  return ADNM_OK;
}
