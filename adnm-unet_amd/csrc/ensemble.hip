// Ensembles of M member forecasts (include/adnm_hip.h: adnm_d4_members, adnm_valid_ens_accum, adnm_ensemble_product).
//   adnm_d4_members        the members of a test-time-augmentation ensemble over the symmetries of the square, and their undoing: a copy
//                          of bit patterns, rows as 16-byte pieces where the shape allows, transposing members through a 32 x 33 LDS tile
//                          so that both sides stay coalesced.
//   adnm_valid_ens_accum   the ONE integer statistic behind CRPS, spread and skill, the rank histogram and the reliability / ROC of the
//                          ensemble exceedance probability: every float read once, the dry pixels counted by ballot, the others with
//                          their M levels as packed bytes, an LDS histogram for the rank and exceedance bins, double atomics of integers.
//   adnm_ensemble_product  the ensemble mean and the exceedance probabilities c / M as fields.
// This family has M forecasts, so it is no entry point of the scored-pair contract (scored_pair.h): it takes the thresholds and the
// quantisation from there and writes its own host check.
#include "scored_pair.h"

namespace {
constexpr int kBlock = 256, kTile = 32, kMaxM = 16;
constexpr int kItem = 4096;   // pixels of one frame a workgroup takes: 16 per thread

// ---- the symmetries of the square ----
struct Codes {
  int c[kMaxM];
};
// where out[y][x] comes from.  code: bit 0 flip left-right, bit 1 flip up-down, bit 2 transpose (adnm_batch_fetch_aug's bits).
//   forward  w.flip(-2), w.flip(-1), w.transpose(-1, -2) in that order: out[y][x] = in[a ^ ud][b ^ lr], (a, b) = T ? (x, y) : (y, x);
//   inverse  transpose first, then the flips:                            out[y][x] = T ? in[x ^ lr][y ^ ud] : in[y ^ ud][x ^ lr]
// (v ^ flip: the mirrored index).  With the transpose bit H == W (the host check).
__device__ __forceinline__ void d4_source(int code, bool inverse, int H, int W, int y, int x, int* sy, int* sx) {
  const bool lr = code & 1, ud = code & 2, tr = code & 4;
  if (!inverse) {
    const int a = tr ? x : y, b = tr ? y : x;
    *sy = ud ? H - 1 - a : a;
    *sx = lr ? W - 1 - b : b;
  } else {
    const int fy = ud ? H - 1 - y : y, fx = lr ? W - 1 - x : x;
    *sy = tr ? fx : fy;
    *sx = tr ? fy : fx;
  }
}

// grid (tiles, planes, M): one 32 x 32 tile of one output plane.  VEC: W % 4 == 0 and both bases on 16 bytes, so every row start of both
// sides is; the members without the transpose bit then move 16 bytes per access (a mirrored row swaps the components of each piece).
template <bool VEC>
__global__ __launch_bounds__(kBlock) void d4_members_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, Codes codes, int inverse,
                                                            int planes, int H, int W, int tiles_x) {
  __shared__ uint32_t tile[kTile][kTile + 1];
  const int m = blockIdx.z, p = blockIdx.y, code = codes.c[m];
  const int oy = ((int)blockIdx.x / tiles_x) * kTile, ox = ((int)blockIdx.x % tiles_x) * kTile;
  const int64_t hw = (int64_t)H * W;
  const uint32_t* in = src + (inverse ? (int64_t)m * planes + p : (int64_t)p) * hw;
  uint32_t* out = dst + ((int64_t)m * planes + p) * hw;
  if (code & 4) {   // (the same for the whole workgroup)
    // the source column follows the output ROW: lane j takes output row oy + j, so a wave reads along source rows
    for (int r = threadIdx.x >> 5; r < kTile; r += kBlock / kTile) {
      const int j = threadIdx.x & 31, y = oy + j, x = ox + r;
      if (y < H && x < W) {
        int sy, sx;
        d4_source(code, inverse, H, W, y, x, &sy, &sx);
        tile[r][j] = in[(int64_t)sy * W + sx];
      }
    }
    __syncthreads();
    for (int r = threadIdx.x >> 5; r < kTile; r += kBlock / kTile) {
      const int i = threadIdx.x & 31, y = oy + r, x = ox + i;
      if (y < H && x < W) out[(int64_t)y * W + x] = tile[i][r];
    }
  } else if (VEC) {
    const int y = oy + (threadIdx.x >> 3), x = ox + 4 * (threadIdx.x & 7);
    if (y < H && x < W) {   // W % 4 == 0: the four columns are inside
      int sy, sx;
      d4_source(code, inverse, H, W, y, x, &sy, &sx);   // sx: the source of column x; mirrored, the piece starts at sx - 3
      uint4 v;
      if (code & 1) {
        const uint4 a = *(const uint4*)(in + (int64_t)sy * W + sx - 3);
        v = make_uint4(a.w, a.z, a.y, a.x);
      } else {
        v = *(const uint4*)(in + (int64_t)sy * W + sx);
      }
      *(uint4*)(out + (int64_t)y * W + x) = v;
    }
  } else {
    for (int r = threadIdx.x >> 5; r < kTile; r += kBlock / kTile) {
      const int y = oy + r, x = ox + (threadIdx.x & 31);
      if (y < H && x < W) {
        int sy, sx;
        d4_source(code, inverse, H, W, y, x, &sy, &sx);
        out[(int64_t)y * W + x] = in[(int64_t)sy * W + sx];
      }
    }
  }
}

// ---- the members as a kernel argument ----
// Frame f = b * T + t of member m starts at base + m * mstride + b * sstride + t * fstride; a stride of 0 holds what lies below it.
struct Members {
  const float* base;
  int64_t mstride, sstride, fstride;
  int M, T, hw;
  __device__ __forceinline__ const float* frame(int f) const { return base + (int64_t)(f / T) * sstride + (int64_t)(f % T) * fstride; }
};

// the limits the score and the product share: nullptr, or the one that refuses
const char* ens_shape_why(int64_t M, int64_t frames, int64_t T, int64_t hw) {
  if (M < 2 || M > kMaxM) return "2 <= M <= 16";
  if (const char* w = pair_frames_why(frames, T)) return w;
  if (hw < 1 || hw >= (1ll << 24)) return "1 <= hw < 2^24";
  return nullptr;
}
const char* ens_strides_why(int64_t mstride, int64_t sstride, int64_t fstride, int64_t frames, int64_t T, int64_t hw) {
  const int64_t sample = (T - 1) * fstride + hw, member = (frames / T - 1) * sstride + sample;   // the extents below a sample / a member stride
  if (fstride != 0 && fstride < hw) return "frame_stride must be 0 or >= hw";
  if (sstride != 0 && sstride < sample) return "sample_stride must be 0 or >= the extent of a sample";
  if (mstride != 0 && mstride < member) return "member_stride must be 0 or >= the extent of a member";
  return nullptr;
}
inline bool ens_quads(const Members& mem, std::initializer_list<const void*> ptrs) {
  return mem.hw % 4 == 0 && mem.mstride % 4 == 0 && mem.sstride % 4 == 0 && mem.fstride % 4 == 0 && adnm_quad_aligned(ADNM_F32, ptrs);
}
// Q = floor(value_scale) when value_scale is finite and 1 <= Q <= 255, else -1
inline int ens_levels(float value_scale) {
  if (!(value_scale >= 1.f) || !(value_scale < 256.f)) return -1;   // (NaN fails the first test, +Inf the second)
  return (int)floorf(value_scale);
}

// ---- the score ----
// q >= thr_k for an integer level q is q >= ceil(thr_k): the thresholds as levels, 0 = every pixel, 256 = none (NaN compares false).
struct Levels {
  int t[kMaxThr], n;
};
inline Levels ens_threshold_levels(const Thr& thr) {
  Levels lv;
  lv.n = thr.n;
  for (int k = 0; k < kMaxThr; ++k) {
    const float t = thr.t[k];
    lv.t[k] = t != t ? 256 : t <= 0.f ? 0 : t > 255.f ? 256 : (int)ceilf(t);
  }
  return lv;
}
inline int64_t ens_cols(int64_t M, int64_t nthr) { return 7 + (M + 1) * (M + 1) + 2 * nthr * (M + 1); }

__device__ __forceinline__ uint32_t ens_q(float v, float value_scale) { return (uint32_t)eval_trunc(eval_scaled(v, value_scale)); }
__device__ __forceinline__ uint64_t ens_wave_sum64(uint64_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
    v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}

// What a lane keeps over its 16 pixels: S0, S1, S2 <= 16 * 120 * 255, V, E <= 16 * (M Q)^2 < 2^28.
struct EnsSums {
  uint32_t s0, s1, s2, v, e;
};
// One pixel that is not dry.  y: the target's level; lev: the M members' levels as packed bytes, member i in byte i % 4 of word i / 4.
// Everything is an integer; the M (M - 1) / 2 differences are the only quadratic part.  hist: the workgroup's bins, laid out as the
// table's columns from 7 on.
__device__ __forceinline__ void ens_wet_pixel(uint32_t y, const uint32_t (&lev)[kMaxM / 4], int M, const Levels& lv, uint32_t* hist, EnsSums& acc) {
  uint32_t x[kMaxM];
#pragma unroll
  for (int i = 0; i < kMaxM; ++i) x[i] = (lev[i >> 2] >> (8 * (i & 3))) & 0xffu;
  uint32_t sx = 0, sxx = 0, s1 = 0, s2 = 0, below = 0, equal = 0;
#pragma unroll
  for (int i = 0; i < kMaxM; ++i)
    if (i < M) {
      const int d = (int)x[i] - (int)y;
      sx += x[i], sxx += x[i] * x[i], s1 += (uint32_t)abs(d);
      below += d < 0 ? 1u : 0u, equal += d == 0 ? 1u : 0u;
#pragma unroll
      for (int j = 0; j < i; ++j) s2 += (uint32_t)abs((int)x[i] - (int)x[j]);
    }
  const int dm = (int)sx - M * (int)y;
  acc.s0 += (uint32_t)abs((int)x[0] - (int)y);
  acc.s1 += s1, acc.s2 += s2;
  acc.v += (uint32_t)M * sxx - sx * sx;
  acc.e += (uint32_t)(dm * dm);
  atomicAdd(&hist[below * (M + 1) + equal], 1u);
  uint32_t* ex = hist + (M + 1) * (M + 1);
#pragma unroll
  for (int k = 0; k < kMaxThr; ++k)
    if (k < lv.n) {
      uint32_t c = 0;
#pragma unroll
      for (int i = 0; i < kMaxM; ++i)
        if (i < M) c += (int)x[i] >= lv.t[k] ? 1u : 0u;
      atomicAdd(&ex[(2 * k + ((int)y >= lv.t[k] ? 1 : 0)) * (M + 1) + c], 1u);
    }
}

// grid (items, frames): 4096 pixels of one frame, 16 per thread.  VEC: four consecutive pixels per access (ens_quads).
template <bool VEC>
__global__ __launch_bounds__(kBlock) void ens_accum_kernel(Members mem, const float* __restrict__ tgt, double* __restrict__ table, int cols,
                                                           float value_scale, Levels lv) {
  __shared__ uint32_t hist[(kMaxM + 1) * (kMaxM + 1) + 2 * kMaxThr * (kMaxM + 1)];
  __shared__ uint64_t red[kBlock / 64][6];   // per wave: S0, S1, S2, V, E, Z
  const int f = blockIdx.y, M = mem.M, hw = mem.hw, p0 = (int)blockIdx.x * kItem;
  const int nbins = (M + 1) * (M + 1) + 2 * lv.n * (M + 1);
  for (int i = threadIdx.x; i < nbins; i += kBlock) hist[i] = 0u;
  __syncthreads();
  const float* mf = mem.frame(f);
  const float* tf = tgt + (int64_t)f * hw;
  EnsSums acc = {0, 0, 0, 0, 0};
  uint32_t zeros = 0;   // wave-uniform: the dry pixels of this wave
  constexpr int kPer = VEC ? 4 : 1;
#pragma unroll 1
  for (int it = 0; it < kItem / (kBlock * kPer); ++it) {   // the same trips for every lane: the ballots below see whole waves
    const int p = p0 + (it * kBlock + (int)threadIdx.x) * kPer;
    const bool valid = p < hw;   // VEC: hw % 4 == 0, a quad is inside or outside as a whole
    uint32_t y[kPer], any[kPer], lev[kPer][kMaxM / 4];
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      y[e] = any[e] = 0;
#pragma unroll
      for (int w = 0; w < kMaxM / 4; ++w) lev[e][w] = 0;
    }
    if (valid) {
      if constexpr (VEC) {
        const float4 t = *(const float4*)(tf + p);
        y[0] = ens_q(t.x, value_scale), y[1] = ens_q(t.y, value_scale), y[2] = ens_q(t.z, value_scale), y[3] = ens_q(t.w, value_scale);
      } else {
        y[0] = ens_q(tf[p], value_scale);
      }
#pragma unroll
      for (int i = 0; i < kMaxM; ++i)
        if (i < M) {
          uint32_t q[kPer];
          if constexpr (VEC) {
            const float4 a = *(const float4*)(mf + (int64_t)i * mem.mstride + p);
            q[0] = ens_q(a.x, value_scale), q[1] = ens_q(a.y, value_scale), q[2] = ens_q(a.z, value_scale), q[3] = ens_q(a.w, value_scale);
          } else {
            q[0] = ens_q(mf[(int64_t)i * mem.mstride + p], value_scale);
          }
#pragma unroll
          for (int e = 0; e < kPer; ++e) any[e] |= q[e], lev[e][i >> 2] |= q[e] << (8 * (i & 3));
        }
    }
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      const bool dry = valid && (y[e] | any[e]) == 0;
      zeros += (uint32_t)__popcll(__ballot(dry));
      if (valid && !dry) ens_wet_pixel(y[e], lev[e], M, lv, hist, acc);
    }
  }
  const uint64_t w0 = ens_wave_sum64(acc.s0), w1 = ens_wave_sum64(acc.s1), w2 = ens_wave_sum64(acc.s2), w3 = ens_wave_sum64(acc.v),
                 w4 = ens_wave_sum64(acc.e);
  if ((threadIdx.x & 63) == 0) {
    uint64_t* r = red[threadIdx.x >> 6];
    r[0] = w0, r[1] = w1, r[2] = w2, r[3] = w3, r[4] = w4, r[5] = zeros;
  }
  __syncthreads();
  double* row = table + (int64_t)(f % mem.T) * cols;
  if (threadIdx.x < 7) {   // columns N, Z, S0, S1, S2, V, E
    const int src = threadIdx.x == 1 ? 5 : (int)threadIdx.x - 2;
    const uint64_t s = threadIdx.x == 0 ? (uint64_t)min(kItem, hw - p0) : (red[0][src] + red[1][src]) + (red[2][src] + red[3][src]);
    if (s) unsafeAtomicAdd(&row[threadIdx.x], (double)s);   // integers below 2^53: exact in any order
  }
  for (int i = threadIdx.x; i < nbins; i += kBlock) {
    const uint32_t v = hist[i];
    if (v) unsafeAtomicAdd(&row[7 + i], (double)v);
  }
}

// ---- the product ----
// grid (items, frames).  VEC: 16-byte loads and stores.  mean = ((x_0 + x_1) + ... + x_(M-1)) / float(M), every operation rounded on its
// own (__fadd_rn / __fdiv_rn: nothing is contracted or reassociated); prob[k] = float(c) / float(M), one IEEE division.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void ens_product_kernel(Members mem, float* __restrict__ mean, float* __restrict__ prob, int frames, float value_scale,
                                                             Thr thr) {
  const int f = blockIdx.y, M = mem.M, hw = mem.hw, p0 = (int)blockIdx.x * kItem;
  const float* mf = mem.frame(f);
  const float fm = (float)M;
  constexpr int kPer = VEC ? 4 : 1;
#pragma unroll 1
  for (int it = 0; it < kItem / (kBlock * kPer); ++it) {
    const int p = p0 + (it * kBlock + (int)threadIdx.x) * kPer;
    if (p >= hw) break;
    float sum[kPer];
    uint32_t cnt[kPer][kMaxThr];
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      sum[e] = 0.f;
#pragma unroll
      for (int k = 0; k < kMaxThr; ++k) cnt[e][k] = 0;
    }
#pragma unroll
    for (int i = 0; i < kMaxM; ++i)
      if (i < M) {
        float v[kPer];
        if constexpr (VEC) {
          const float4 a = *(const float4*)(mf + (int64_t)i * mem.mstride + p);
          v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
        } else {
          v[0] = mf[(int64_t)i * mem.mstride + p];
        }
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
          sum[e] = i == 0 ? v[e] : __fadd_rn(sum[e], v[e]);
          if (thr.n) {
            const float q = eval_trunc(eval_scaled(v[e], value_scale));
#pragma unroll
            for (int k = 0; k < kMaxThr; ++k)
              if (k < thr.n) cnt[e][k] += q >= thr.t[k] ? 1u : 0u;
          }
        }
      }
    float* mo = mean + (int64_t)f * hw + p;
    if constexpr (VEC) {
      *(float4*)mo = make_float4(__fdiv_rn(sum[0], fm), __fdiv_rn(sum[1], fm), __fdiv_rn(sum[2], fm), __fdiv_rn(sum[3], fm));
    } else {
      mo[0] = __fdiv_rn(sum[0], fm);
    }
#pragma unroll
    for (int k = 0; k < kMaxThr; ++k)
      if (k < thr.n) {
        float* po = prob + ((int64_t)k * frames + f) * hw + p;
        if constexpr (VEC) {
          *(float4*)po = make_float4(__fdiv_rn((float)cnt[0][k], fm), __fdiv_rn((float)cnt[1][k], fm), __fdiv_rn((float)cnt[2][k], fm),
                                     __fdiv_rn((float)cnt[3][k], fm));
        } else {
          po[0] = __fdiv_rn((float)cnt[0][k], fm);
        }
      }
  }
}
}  // namespace

extern "C" int adnm_d4_members(const float* src, float* dst, const int* codes_host, int64_t M, int inverse, int64_t planes, int64_t H, int64_t W,
                               adnm_stream_t stream) {
  ADNM_REQUIRE(src && dst && codes_host, "d4_members: null pointer");
  ADNM_REQUIRE(((uintptr_t)src | (uintptr_t)dst) % 4 == 0, "d4_members: src and dst must be 4-byte aligned");
  ADNM_REQUIRE(M >= 1 && M <= kMaxM, "d4_members: 1 <= M <= 16, got %lld", (long long)M);
  ADNM_REQUIRE(planes >= 1 && planes <= 65535, "d4_members: 1 <= planes <= 65535, got %lld", (long long)planes);
  if (const char* w = pair_tiled_shape_why(H, W)) ADNM_REQUIRE(false, "d4_members: %s (got %lld x %lld)", w, (long long)H, (long long)W);
  Codes codes;
  for (int m = 0; m < kMaxM; ++m) {
    codes.c[m] = m < M ? codes_host[m] : 0;
    ADNM_REQUIRE(codes.c[m] >= 0 && codes.c[m] <= 7, "d4_members: a code is in 0..7, got %d", codes.c[m]);
    ADNM_REQUIRE(!(codes.c[m] & 4) || H == W, "d4_members: a transposing code needs square frames, got %lld x %lld", (long long)H, (long long)W);
  }
  const bool vec = W % 4 == 0 && adnm_quad_aligned(ADNM_F32, {src, dst});
  const int tiles_x = (int)adnm_cdiv(W, kTile);
  const dim3 grid((unsigned)(tiles_x * adnm_cdiv(H, kTile)), (unsigned)planes, (unsigned)M);
  hipStream_t st = (hipStream_t)stream;
  {
    ADNM_PROF("d4_members", st, 8.0 * M * planes * H * W);
    if (vec) d4_members_kernel<true><<<grid, kBlock, 0, st>>>((const uint32_t*)src, (uint32_t*)dst, codes, inverse ? 1 : 0, (int)planes, (int)H, (int)W, tiles_x);
    else d4_members_kernel<false><<<grid, kBlock, 0, st>>>((const uint32_t*)src, (uint32_t*)dst, codes, inverse ? 1 : 0, (int)planes, (int)H, (int)W, tiles_x);
  }
  ADNM_CHECK_LAUNCH("d4_members");
  return ADNM_OK;
}

extern "C" int64_t adnm_valid_ens_block_bytes(int64_t T, int64_t nthr, int64_t M) {
  if (T < 1 || T > 65535 || nthr < 1 || nthr > kMaxThr || M < 2 || M > kMaxM) return -1;
  return (int64_t)sizeof(double) * T * ens_cols(M, nthr);
}

extern "C" int64_t adnm_valid_ens_accum_ws_bytes(int64_t frames, int64_t T, int64_t hw, int64_t nthr, int64_t M, float value_scale) {
  if (nthr < 1 || nthr > kMaxThr || ens_shape_why(M, frames, T, hw) || ens_levels(value_scale) < 0) return -1;
  return 0;   // the partial histograms live in LDS
}

extern "C" int adnm_valid_ens_accum(const float* members, int64_t member_stride, int64_t sample_stride, int64_t frame_stride, const float* target,
                                    void* table, const float* thresholds_host, int64_t nthr, float value_scale, int64_t M, void* ws, int64_t ws_bytes,
                                    int64_t frames, int64_t T, int64_t hw, adnm_stream_t stream) {
  (void)ws, (void)ws_bytes;   // none is needed: the query answers 0
  ADNM_REQUIRE(members && target && table && thresholds_host, "valid_ens_accum: null pointer");
  ADNM_REQUIRE(((uintptr_t)members | (uintptr_t)target) % 4 == 0, "valid_ens_accum: members and target must be 4-byte aligned");
  ADNM_REQUIRE((uintptr_t)table % 8 == 0, "valid_ens_accum: the table must be 8-byte aligned");
  ADNM_REQUIRE(nthr >= 1 && nthr <= kMaxThr, "valid_ens_accum: 1..8 thresholds, got %lld", (long long)nthr);
  if (const char* w = ens_shape_why(M, frames, T, hw))
    ADNM_REQUIRE(false, "valid_ens_accum: %s (got M %lld frames %lld T %lld hw %lld)", w, (long long)M, (long long)frames, (long long)T, (long long)hw);
  ADNM_REQUIRE(ens_levels(value_scale) >= 0, "valid_ens_accum: value_scale finite with 1 <= floor(value_scale) <= 255, got %g", (double)value_scale);
  if (const char* w = ens_strides_why(member_stride, sample_stride, frame_stride, frames, T, hw))
    ADNM_REQUIRE(false, "valid_ens_accum: %s (got member %lld sample %lld frame %lld)", w, (long long)member_stride, (long long)sample_stride,
                 (long long)frame_stride);
  const Members mem = {members, member_stride, sample_stride, frame_stride, (int)M, (int)T, (int)hw};
  const Levels lv = ens_threshold_levels(thr_fill(thresholds_host, nthr));
  const int cols = (int)ens_cols(M, nthr);
  const dim3 grid((unsigned)adnm_cdiv(hw, kItem), (unsigned)frames);
  hipStream_t st = (hipStream_t)stream;
  {
    ADNM_PROF("valid_ens", st, 4.0 * (M + 1) * frames * hw);
    if (ens_quads(mem, {members, target})) ens_accum_kernel<true><<<grid, kBlock, 0, st>>>(mem, target, (double*)table, cols, value_scale, lv);
    else ens_accum_kernel<false><<<grid, kBlock, 0, st>>>(mem, target, (double*)table, cols, value_scale, lv);
  }
  ADNM_CHECK_LAUNCH("valid_ens_accum");
  return ADNM_OK;
}

extern "C" int adnm_ensemble_product(const float* members, int64_t member_stride, int64_t sample_stride, int64_t frame_stride, float* mean, float* prob,
                                     const float* thresholds_host, int64_t K, float value_scale, int64_t M, int64_t frames, int64_t T, int64_t hw,
                                     adnm_stream_t stream) {
  ADNM_REQUIRE(members && mean, "ensemble_product: null pointer");
  ADNM_REQUIRE(K >= 0 && K <= kMaxThr, "ensemble_product: 0..8 thresholds, got %lld", (long long)K);
  ADNM_REQUIRE(K == 0 || (prob && thresholds_host), "ensemble_product: null pointer");
  ADNM_REQUIRE(((uintptr_t)members | (uintptr_t)mean | (uintptr_t)prob) % 4 == 0, "ensemble_product: members, mean and prob must be 4-byte aligned");
  if (const char* w = ens_shape_why(M, frames, T, hw))
    ADNM_REQUIRE(false, "ensemble_product: %s (got M %lld frames %lld T %lld hw %lld)", w, (long long)M, (long long)frames, (long long)T, (long long)hw);
  if (const char* w = ens_strides_why(member_stride, sample_stride, frame_stride, frames, T, hw))
    ADNM_REQUIRE(false, "ensemble_product: %s (got member %lld sample %lld frame %lld)", w, (long long)member_stride, (long long)sample_stride,
                 (long long)frame_stride);
  const Members mem = {members, member_stride, sample_stride, frame_stride, (int)M, (int)T, (int)hw};
  const Thr thr = thr_fill(thresholds_host, K);   // (K = 0 reads nothing)
  const dim3 grid((unsigned)adnm_cdiv(hw, kItem), (unsigned)frames);
  hipStream_t st = (hipStream_t)stream;
  {
    ADNM_PROF("ensemble_product", st, 4.0 * (M + 1 + K) * frames * hw);
    if (ens_quads(mem, {members, mean, prob})) ens_product_kernel<true><<<grid, kBlock, 0, st>>>(mem, mean, prob, (int)frames, K ? value_scale : 0.f, thr);
    else ens_product_kernel<false><<<grid, kBlock, 0, st>>>(mem, mean, prob, (int)frames, K ? value_scale : 0.f, thr);
  }
  ADNM_CHECK_LAUNCH("ensemble_product");
  return ADNM_OK;
}
