// Radially averaged power spectra and the co-spectrum of forecast and observation (include/adnm_hip.h: adnm_valid_spectrum_accum;
// DESIGN.md §4k).  The fields are o = clip(target, 0, 1) * value_scale and f = clip(forecast, 0, 1) * value_scale (numpy's clip: a NaN
// stays a NaN); O and F are their unnormalised 2-D DFTs; per coefficient p_o = |O|^2 / (H W), p_f = |F|^2 / (H W),
// c = Re(F conj O) / (H W); the coefficients are summed per radial bin r = round(sqrt((ky L/H)^2 + (kx L/W)^2)), L = max(H, W), r < L/2.
//
//   spec_rows   one workgroup per group of row PAIRS of one frame, both fields.  Rows 2p and 2p + 1 of ONE field are packed as the real
//               and the imaginary part of one complex row (z = row_2p + i row_2p+1), transformed along x in LDS and unpacked:
//               A(kx) = (Z(kx) + conj Z(-kx)) / 2 is row 2p's transform, B(kx) = (Z(kx) - conj Z(-kx)) / 2i row 2p + 1's.  Only
//               kx = 0 .. W/2 is kept (the fields are real: X(-ky, -kx) = conj X(ky, kx)), written TRANSPOSED to ws:
//               cols[frame][kx][field][y] complex, so that the column pass reads contiguous memory.  Each pixel is read from HBM once.
//               o and f are NOT packed into one transform: with the same instructions applied to each field, pred == target gives
//               F == O bit for bit and pred == 0 gives F == 0 exactly, which the packed form o + i f cannot promise.
//   spec_cols   one workgroup per (kx, frame): the two columns (o's, f's) are transformed along y in LDS; p_o, p_f, c of the H
//               coefficients are formed with ONE expression (spec_dot) and weighted 2 for 0 < kx < W/2, where the column stands for
//               its mirror image -kx as well (the same values by the symmetry above).  Along a column the bin grows with |ky|, so bin r
//               owns a run of |ky|: one thread per bin adds its run in ascending |ky| (+ky, then -ky) in fp32 -> part[frame][kx][r][3].
//               Every cell is written, empty bins with 0.
//   spec_fold   one thread per (t, r, column): table[t][r][.] += the partials in DOUBLE, samples ascending, then kx ascending.
//
// Transform: radix-2 decimation in time, log2 N stages in place in LDS, input stored bit-reversed.  Twiddles exp(-2 pi i j / N), j < N/2:
// sincospi in DOUBLE, rounded once to fp32, built per workgroup in LDS.  All other arithmetic is fp32.  No atomics, a fixed order
// everywhere: the same calls on the same table give the same bits, whatever the workspace held.
#include "scored_pair.h"

namespace {
constexpr int kBlock = 256, kFoldBlock = 256;
constexpr int kMinN = 8, kMaxN = 512;
constexpr int kRowElems = 4096;                       // complex elements of a row workgroup: 2 fields x row pairs x W
constexpr int kRowBuf = kRowElems + kRowElems / kMinN;   // each packed row is W + 1 apart: the unpack reads one column of many rows

// numpy's clip keeps a NaN (fmaxf would return the 0)
__device__ __forceinline__ float spec_field(float v, float value_scale) { return (v != v ? v : fminf(fmaxf(v, 0.f), 1.f)) * value_scale; }

// Re(a conj b): the ONE expression behind p_o, p_f and c, so that equal operands give equal bits
__device__ __forceinline__ float spec_dot(float2 a, float2 b) { return fmaf(a.x, b.x, __fmul_rn(a.y, b.y)); }

__device__ __forceinline__ void spec_twiddles(float2* tw, int N) {
  for (int j = threadIdx.x; j < N / 2; j += kBlock) {
    double s, c;
    sincospi(-2.0 * (double)j / (double)N, &s, &c);
    tw[j] = make_float2((float)c, (float)s);
  }
}

// nfft transforms of length N = 2^logN, transform q at buf + q * pitch, input in bit-reversed order.  Ends synchronised.
__device__ __forceinline__ void spec_stages(float2* buf, const float2* tw, int nfft, int logN, int pitch) {
  const int half_n = 1 << (logN - 1), total = nfft << (logN - 1);
  for (int s = 1; s <= logN; ++s) {
    const int half = 1 << (s - 1);
    for (int i = threadIdx.x; i < total; i += kBlock) {
      const int q = i >> (logN - 1), j = i & (half_n - 1), pos = j & (half - 1), i0 = q * pitch + ((j >> (s - 1)) << s) + pos, i1 = i0 + half;
      const float2 w = tw[pos << (logN - s)], a = buf[i0], b = buf[i1];
      const float2 t = make_float2(w.x * b.x - w.y * b.y, w.x * b.y + w.y * b.x);
      buf[i0] = make_float2(a.x + t.x, a.y + t.y);
      buf[i1] = make_float2(a.x - t.x, a.y - t.y);
    }
    __syncthreads();
  }
}

__device__ __forceinline__ int spec_brev(int x, int logN) { return (int)(__brev((unsigned)x) >> (32 - logN)); }

// grid (H / 2 / RP, frames): RP row pairs of frame blockIdx.y from pair blockIdx.x * RP on.  VEC: pair_quads (W always is a multiple of 4).
template <bool VEC>
__global__ __launch_bounds__(kBlock) void spec_rows_kernel(ScoredPair pair, float2* __restrict__ cols, int H, int W, int logW, int RP, float value_scale) {
  __shared__ float2 buf[kRowBuf];
  __shared__ float2 tw[kMaxN / 2];
  const int f = blockIdx.y, p0 = blockIdx.x * RP, pitch = W + 1;
  spec_twiddles(tw, W);
  // transform q = field * RP + pair: field 0 the target, 1 the forecast
  const float* src[2] = {pair.target(f) + (int64_t)2 * p0 * W, pair.forecast(f) + (int64_t)2 * p0 * W};
  if (VEC) {
    for (int i = threadIdx.x; i < RP * (W >> 2); i += kBlock) {
      const int pr = i / (W >> 2), x = (i % (W >> 2)) * 4;
#pragma unroll
      for (int fld = 0; fld < 2; ++fld) {
        const float* row = src[fld] + (int64_t)2 * pr * W + x;
        const float4 a = *(const float4*)row, b = *(const float4*)(row + W);
        float2* dst = buf + (fld * RP + pr) * pitch;
        dst[spec_brev(x + 0, logW)] = make_float2(spec_field(a.x, value_scale), spec_field(b.x, value_scale));
        dst[spec_brev(x + 1, logW)] = make_float2(spec_field(a.y, value_scale), spec_field(b.y, value_scale));
        dst[spec_brev(x + 2, logW)] = make_float2(spec_field(a.z, value_scale), spec_field(b.z, value_scale));
        dst[spec_brev(x + 3, logW)] = make_float2(spec_field(a.w, value_scale), spec_field(b.w, value_scale));
      }
    }
  } else {
    for (int i = threadIdx.x; i < RP * W; i += kBlock) {
      const int pr = i >> logW, x = i & (W - 1);
#pragma unroll
      for (int fld = 0; fld < 2; ++fld) {
        const float* row = src[fld] + (int64_t)2 * pr * W + x;
        buf[(fld * RP + pr) * pitch + spec_brev(x, logW)] = make_float2(spec_field(row[0], value_scale), spec_field(row[W], value_scale));
      }
    }
  }
  __syncthreads();
  spec_stages(buf, tw, 2 * RP, logW, pitch);
  const int nk = W / 2 + 1;
  for (int i = threadIdx.x; i < 2 * nk * RP; i += kBlock) {
    const int pr = i % RP, kx = (i / RP) % nk, fld = i / (RP * nk);
    const float2* z = buf + (fld * RP + pr) * pitch;
    const float2 zk = z[kx], zm = z[(W - kx) & (W - 1)];
    float2* dst = cols + (((int64_t)f * nk + kx) * 2 + fld) * H + 2 * (p0 + pr);
    dst[0] = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
    dst[1] = make_float2(0.5f * (zk.y + zm.y), 0.5f * (zm.x - zk.x));
  }
}

// r = round(sqrt(k2)) in integers: the r with r^2 - r < k2 <= r^2 + r (k2 = 0: r = 0)
__device__ __forceinline__ int spec_bin(int sy, int sx) {
  const int k2 = sy * sy + sx * sx;
  int r = (int)(sqrtf((float)k2) + 0.5f);
  while (r > 0 && r * r - r >= k2) --r;
  while (r * r + r < k2) ++r;
  return r;
}

// grid (W / 2 + 1, frames).  scale = 1 / (H W), a power of two.
__global__ __launch_bounds__(kBlock) void spec_cols_kernel(const float2* __restrict__ cols, float* __restrict__ part, int H, int W, int logH, int L, float scale) {
  __shared__ float2 buf[2 * kMaxN];
  __shared__ float2 tw[kMaxN / 2];
  __shared__ float val[3][kMaxN];
  __shared__ int lo[kMaxN / 2], hi[kMaxN / 2];
  const int kx = blockIdx.x, nk = gridDim.x, f = blockIdx.y, R = L / 2;
  const float2* src = cols + ((int64_t)f * nk + kx) * 2 * H;
  spec_twiddles(tw, H);
  for (int i = threadIdx.x; i < 2 * H; i += kBlock) buf[(i >> logH) * H + spec_brev(i & (H - 1), logH)] = src[i];
  for (int r = threadIdx.x; r < R; r += kBlock) lo[r] = -1, hi[r] = -1;
  __syncthreads();
  spec_stages(buf, tw, 2, logH, H);
  const float wgt = (kx == 0 || kx == W / 2) ? scale : 2.f * scale;   // 0 < kx < W/2 stands for -kx too
  for (int ky = threadIdx.x; ky < H; ky += kBlock) {
    const float2 o = buf[ky], g = buf[H + ky];
    val[0][ky] = spec_dot(o, o) * wgt;
    val[1][ky] = spec_dot(g, g) * wgt;
    val[2][ky] = spec_dot(g, o) * wgt;
  }
  // |ky| = m sits in bin b(m), which does not fall as m grows: bin b owns the run lo[b] .. hi[b]
  const int sx = kx * (L / W), my = L / H;
  for (int m = threadIdx.x; m <= H / 2; m += kBlock) {
    const int b = spec_bin(m * my, sx);
    if (b < R) {
      if (m == 0 || spec_bin((m - 1) * my, sx) != b) lo[b] = m;
      if (m == H / 2 || spec_bin((m + 1) * my, sx) != b) hi[b] = m;
    }
  }
  __syncthreads();
  float* out = part + ((int64_t)f * nk + kx) * R * 3;
  for (int r = threadIdx.x; r < R; r += kBlock) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    if (lo[r] >= 0)
      for (int m = lo[r]; m <= hi[r]; ++m) {
        if (m < H / 2) a0 += val[0][m], a1 += val[1][m], a2 += val[2][m];                   // ky = +m
        if (m > 0) a0 += val[0][H - m], a1 += val[1][H - m], a2 += val[2][H - m];          // ky = -m (-H/2 has no mirror image)
      }
    out[3 * r + 0] = a0;
    out[3 * r + 1] = a1;
    out[3 * r + 2] = a2;
  }
}

// One thread per (t, r, column), a fixed order (samples ascending, then kx ascending), double: table[t][r][.] += the batch's sums
__global__ __launch_bounds__(kFoldBlock) void spec_fold_kernel(const float* __restrict__ part, int nk, int frames, int T, int R, double* __restrict__ table) {
  const int B = frames / T, i = blockIdx.x * kFoldBlock + threadIdx.x;
  if (i >= T * R * 3) return;
  const int t = i / (R * 3), rc = i % (R * 3);
  double s = 0.0;
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < nk; ++k) s += (double)part[(((int64_t)b * T + t) * nk + k) * R * 3 + rc];
  table[i] += s;
}

inline bool spec_size_ok(int64_t n) { return n >= kMinN && n <= kMaxN && (n & (n - 1)) == 0; }
inline int spec_log2(int64_t n) {
  int l = 0;
  while ((1ll << l) < n) ++l;
  return l;
}
const char* spec_why(int64_t frames, int64_t T, int64_t H, int64_t W) {
  if (!spec_size_ok(H) || !spec_size_ok(W)) return "H and W must be powers of two in 8..512";
  return pair_frames_why(frames, T);
}
inline int64_t spec_cols_bytes(int64_t frames, int64_t H, int64_t W) { return frames * (W / 2 + 1) * 2 * H * (int64_t)sizeof(float2); }
}  // namespace

extern "C" int64_t adnm_valid_spectrum_block_bytes(int64_t T, int64_t H, int64_t W) {
  if (T < 1 || T > 65535 || !spec_size_ok(H) || !spec_size_ok(W)) return -1;
  return (int64_t)sizeof(double) * T * ((H > W ? H : W) / 2) * 3;
}

extern "C" int64_t adnm_valid_spectrum_accum_ws_bytes(int64_t frames, int64_t T, int64_t H, int64_t W) {
  if (spec_why(frames, T, H, W)) return -1;
  return spec_cols_bytes(frames, H, W) + frames * (W / 2 + 1) * ((H > W ? H : W) / 2) * 3 * (int64_t)sizeof(float);
}

extern "C" int adnm_valid_spectrum_accum(const float* pred, int64_t pred_sample_stride, int64_t pred_frame_stride, const float* target, void* table,
                                         float value_scale, void* ws, int64_t ws_bytes, int64_t frames, int64_t T, int64_t H, int64_t W,
                                         adnm_stream_t stream) {
  const PairCall call = {"valid_spectrum_accum", pred, pred_sample_stride, pred_frame_stride, target, table, ws, ws_bytes, H, W,
                         /*flat*/ false, /*ws_optional*/ false, /*ws_aligned*/ true, /*ws_rc*/ ADNM_EINVAL};
  if (int rc = pair_check(call, ws != nullptr, spec_why(frames, T, H, W),
                          adnm_valid_spectrum_accum_ws_bytes(frames, T, H, W),
                          "frames %lld T %lld %lld x %lld", (long long)frames, (long long)T, (long long)H, (long long)W))
    return rc;
  const int64_t L = H > W ? H : W, R = L / 2, nk = W / 2 + 1;
  const int64_t rp = (kRowElems / 2) / W < H / 2 ? (kRowElems / 2) / W : H / 2;   // row pairs per workgroup: a power of two that divides H / 2
  float2* cols = (float2*)ws;
  float* part = (float*)((char*)ws + spec_cols_bytes(frames, H, W));
  const bool vec = pair_quads(W, pred_sample_stride, pred_frame_stride, pred, target);
  const ScoredPair pair = {pred, pred_sample_stride, pred_frame_stride, target, (int)T, (int)(H * W)};
  hipStream_t st = (hipStream_t)stream;
  {
    ADNM_PROF("valid_spectrum_rows", st, 8.0 * frames * H * W + 16.0 * frames * nk * H);
    const dim3 grid((unsigned)(H / 2 / rp), (unsigned)frames);
    if (vec) spec_rows_kernel<true><<<grid, kBlock, 0, st>>>(pair, cols, (int)H, (int)W, spec_log2(W), (int)rp, value_scale);
    else spec_rows_kernel<false><<<grid, kBlock, 0, st>>>(pair, cols, (int)H, (int)W, spec_log2(W), (int)rp, value_scale);
  }
  ADNM_CHECK_LAUNCH("valid_spectrum_rows");
  {
    ADNM_PROF("valid_spectrum_cols", st, 16.0 * frames * nk * H + 12.0 * frames * nk * R);
    spec_cols_kernel<<<dim3((unsigned)nk, (unsigned)frames), kBlock, 0, st>>>(cols, part, (int)H, (int)W, spec_log2(H), (int)L, 1.f / (float)(H * W));
  }
  ADNM_CHECK_LAUNCH("valid_spectrum_cols");
  {
    ADNM_PROF("valid_spectrum_fold", st, 12.0 * frames * nk * R);
    spec_fold_kernel<<<(unsigned)adnm_cdiv(T * R * 3, kFoldBlock), kFoldBlock, 0, st>>>(part, (int)nk, (int)frames, (int)T, (int)R, (double*)table);
  }
  ADNM_CHECK_LAUNCH("valid_spectrum_fold");
  return ADNM_OK;
}
