// The Lagrangian-persistence baseline of the validation epoch (include/adnm_hip.h: adnm_trec_motion, adnm_advect): block-matched
// motion between the last two input frames (TREC, Rinehart & Garvey 1978) and the last frame moved along it over the horizon.
//
//   trec_cost   one workgroup per (block, sample).  The block of `last` and the (block + 2R)-row window of `prev` are staged ONCE as
//               quantised bytes q(v), four to a dword; cost(dy, dx) = SUM |q(last)(y, x) - q(prev)(y - dy, x - dx)| over the block's in-frame
//               pixels is formed from packed dwords: v_alignbyte_b32 takes the dword at any byte offset out of two neighbours and v_sad_u8
//               adds four byte differences to the running sum.  -> ws[sample][block][(2R+1)^2 costs | echo count] uint32.
//   trec_pick   one workgroup per sample: the 64-bit sum of the tables in block order (the whole-frame SAD), its pick g, the pick of every
//               block, validity, the vectors.
//   advect      adv[s, t, y, x] = last[s, y - (t+1) vy, x - (t+1) vx] with v of the block of (y, x): a gather of bit patterns.
//
// Integer arithmetic and bit copies only, no atomics: exact, and the same bits whatever the workspace held.
#include "trec.h"

namespace {
constexpr int kBlock = 256;
constexpr int kMaxBs = kTrecMaxBs, kMaxR = kTrecMaxR;
constexpr int kCurPitch = kMaxBs / 4;                        // dwords per staged row of the block
constexpr int kWinRows = kMaxBs + 2 * kMaxR;                 // 48
constexpr int kWinPitch = (kMaxBs + 2 * kMaxR) / 4 + 1;      // 12 dwords of window and one that is only ever the unused high operand: 13
constexpr int kParts = 8;                                    // adjacent lanes that share a displacement and split the block's rows

__device__ __forceinline__ uint32_t trec_q(float v, float value_scale) { return (uint32_t)eval_trunc(eval_scaled(v, value_scale)); }   // <= 255: value_scale <= 255

__device__ __forceinline__ uint32_t trec_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

// Four pixels (gy, gx .. gx + 3) of a frame as q bytes, byte e = pixel gx + e; 0 outside the frame.  VEC: gx is a multiple of 4, and so
// are W and the frame's offset from a 16-byte aligned base: the four lie inside or outside the frame together and are one 16-byte load.
template <bool VEC>
__device__ __forceinline__ uint32_t trec_quad(const float* __restrict__ frame, int gy, int gx, int H, int W, float value_scale) {
  if (gy < 0 || gy >= H) return 0;
  const float* row = frame + (int64_t)gy * W;
  if (VEC) {
    if (gx < 0 || gx >= W) return 0;
    const float4 a = *(const float4*)(row + gx);
    return trec_q(a.x, value_scale) | (trec_q(a.y, value_scale) << 8) | (trec_q(a.z, value_scale) << 16) | (trec_q(a.w, value_scale) << 24);
  }
  uint32_t d = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (gx + e >= 0 && gx + e < W) d |= trec_q(row[gx + e], value_scale) << (8 * e);
  return d;
}

// grid (nby * nbx, samples).  hs: the staged halo along x, R rounded up to 4, so that the window starts at a multiple of 4 columns.
// Byte c of a staged row of the window is prev(x0 - hs + c); the operand of cur's dword j under dx starts at byte 4j + hs - dx.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void trec_cost_kernel(const float* __restrict__ prev, const float* __restrict__ last, int64_t sstride,
                                                           uint32_t* __restrict__ ws, int H, int W, int nbx, int bs, int R, int hs, int echo,
                                                           float value_scale) {
  __shared__ uint32_t cur[kMaxBs][kCurPitch];
  __shared__ uint32_t win[kWinRows][kWinPitch];
  __shared__ uint32_t red[kBlock / 64];
  const int blk = blockIdx.x, s = blockIdx.y, y0 = (blk / nbx) * bs, x0 = (blk % nbx) * bs;
  const float* pf = prev + (int64_t)s * sstride;
  const float* lf = last + (int64_t)s * sstride;
  const int cq = bs >> 2, wq = (bs + 2 * hs) >> 2, wrows = bs + 2 * R;
  uint32_t cnt = 0;
  for (int i = threadIdx.x; i < bs * cq; i += kBlock) {
    const int r = i / cq, j = i % cq;
    const uint32_t d = trec_quad<VEC>(lf, y0 + r, x0 + 4 * j, H, W, value_scale);   // 0 outside the frame: never an echo (echo >= 1)
    cur[r][j] = d;
#pragma unroll
    for (int e = 0; e < 4; ++e) cnt += ((d >> (8 * e)) & 0xffu) >= (uint32_t)echo ? 1u : 0u;
  }
  for (int i = threadIdx.x; i < wrows * (wq + 1); i += kBlock) {
    const int r = i / (wq + 1), c = i % (wq + 1);
    win[r][c] = c < wq ? trec_quad<VEC>(pf, y0 - R + r, x0 - hs + 4 * c, H, W, value_scale) : 0u;
  }
  cnt = trec_wave_sum(cnt);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
  __syncthreads();
  // the block's in-frame part: rows [0, rin), columns [0, cin); the last dword of a clipped row keeps its first cin - 4 (jn - 1) bytes.
  // cur is 0 outside the frame; the mask takes the same pixels out of the window's operand.
  const int rin = min(bs, H - y0), cin = min(bs, W - x0), jn = (cin + 3) >> 2, tail = cin - 4 * (jn - 1);
  const uint32_t tail_mask = tail == 4 ? 0xffffffffu : (1u << (8 * tail)) - 1u;
  const int D = 2 * R + 1, nd = D * D;
  uint32_t* out = ws + ((int64_t)s * gridDim.x + blk) * (nd + 1);
  // item = (displacement, part): the same trips for every lane, the parts of a displacement are kParts adjacent lanes of one wave
  for (int i0 = 0; i0 < nd * kParts; i0 += kBlock) {
    const int item = i0 + threadIdx.x, d = item / kParts, part = item % kParts;
    uint32_t acc = 0;
    if (d < nd) {
      const int dy = d / D - R, dx = d % D - R;
      const int off = hs - dx, w0 = off >> 2;         // off in [hs - R, hs + R], >= 0
      const uint32_t sh = (uint32_t)(off & 3);
      for (int r = part; r < rin; r += kParts) {
        const uint32_t* wr = win[r - dy + R];         // row y0 + r - dy of prev: staged row r - dy + R in [0, bs + 2R)
        const uint32_t* cr = cur[r];
        for (int j = 0; j < jn; ++j) {
          // bytes 4j + off .. 4j + off + 3 of the row: ({hi, lo} >> 8 sh); w0 + j + 1 <= (bs - 4 + 2 hs) / 4 + 1 = wq, the zeroed dword
          uint32_t p = __builtin_amdgcn_alignbyte(wr[w0 + j + 1], wr[w0 + j], sh);
          if (j == jn - 1) p &= tail_mask;
          acc = __builtin_amdgcn_sad_u8(cr[j], p, acc);
        }
      }
    }
#pragma unroll
    for (int o = kParts >> 1; o >= 1; o >>= 1) acc += (uint32_t)__shfl_xor((int)acc, o, 64);
    if (d < nd && part == 0) out[d] = acc;
  }
  if (threadIdx.x == 0) out[nd] = (red[0] + red[1]) + (red[2] + red[3]);
}

// grid (samples).  ws: trec_cost's tables.  motion[s][b] = (vy, vx); cost_out (or null): the tables without the echo counts.
__global__ __launch_bounds__(kBlock) void trec_pick_kernel(const uint32_t* __restrict__ ws, int32_t* __restrict__ motion, uint32_t* __restrict__ cost_out,
                                                           int nblk, int bs, int R) {
  __shared__ uint64_t red[kBlock / 64];
  const int s = blockIdx.x, D = 2 * R + 1, nd = D * D, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t* tab = ws + (int64_t)s * nblk * (nd + 1);
  // the global vector: displacement d = threadIdx.x (and + 256: nd <= 289), blocks ascending, 64-bit sums
  uint64_t best = ~0ull;
  for (int d = threadIdx.x; d < nd; d += kBlock) {
    uint64_t sum = 0;
    for (int b = 0; b < nblk; ++b) sum += tab[(int64_t)b * (nd + 1) + d];
    const uint64_t k = trec_key(sum, d, R);
    best = k < best ? k : best;
  }
  best = trec_wave_min(best);
  if (lane == 0) red[wave] = best;
  __syncthreads();
  uint64_t g = red[0];
#pragma unroll
  for (int w = 1; w < kBlock / 64; ++w) g = red[w] < g ? red[w] : g;
  // a wave per block
  for (int b = wave; b < nblk; b += kBlock / 64) {
    const uint32_t* t = tab + (int64_t)b * (nd + 1);
    uint64_t k = ~0ull;
    for (int d = lane; d < nd; d += 64) {
      const uint32_t c = t[d];
      if (cost_out) cost_out[((int64_t)s * nblk + b) * nd + d] = c;
      const uint64_t kd = trec_key(c, d, R);
      k = kd < k ? kd : k;
    }
    k = trec_wave_min(k);
    if (t[nd] < (uint32_t)bs) k = g;   // fewer than `block` echo pixels: the block moves with the frame
    if (lane < 2) {
      const int v = lane == 0 ? (int)((k >> 5) & 31u) - R : (int)(k & 31u) - R;
      motion[((int64_t)s * nblk + b) * 2 + lane] = v;
    }
  }
}

// One thread per four pixels of a row (they share a block: block is a multiple of 4), grid-stride over samples * T * H * ceil(W / 4).
// VEC: W % 4 == 0 and out 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void advect_kernel(const uint32_t* __restrict__ last, int64_t sstride, const int32_t* __restrict__ motion,
                                                        uint32_t* __restrict__ out, int bs, int nby, int nbx, int64_t total, int64_t T, int H, int W) {
  const int wq = (W + 3) >> 2;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
    const int x = (int)(i % wq) * 4, y = (int)((i / wq) % H);
    const int64_t f = i / ((int64_t)wq * H);
    const int64_t t = f % T;
    const int64_t s = f / T;
    const int32_t* v = motion + ((s * nby + y / bs) * nbx + x / bs) * 2;
    const int64_t sy = (int64_t)y - (t + 1) * v[0], sx = (int64_t)x - (t + 1) * v[1];
    const uint32_t* src = last + s * sstride;
    uint32_t px[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool in = sy >= 0 && sy < H && sx + e >= 0 && sx + e < W;
      px[e] = in ? src[sy * W + sx + e] : 0u;   // +0.0f
    }
    uint32_t* dst = out + (f * H + y) * (int64_t)W + x;
    if (VEC) {
      *(uint4*)dst = make_uint4(px[0], px[1], px[2], px[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (x + e < W) dst[e] = px[e];
    }
  }
}

}  // namespace

extern "C" int64_t adnm_trec_ws_bytes(int64_t samples, int64_t H, int64_t W, int64_t block, int64_t radius) {
  if (!trec_shape_ok(samples, H, W, block, nullptr) || radius < 1 || radius > kMaxR) return -1;
  const int64_t D = 2 * radius + 1;
  return samples * adnm_cdiv(H, block) * adnm_cdiv(W, block) * (D * D + 1) * (int64_t)sizeof(uint32_t);
}

int adnm_trec_cost_launch(const char* what, const float* prev, const float* last, int64_t sample_stride, float value_scale, int64_t block, int64_t radius,
                          int64_t echo, void* ws, int64_t ws_bytes, int64_t samples, int64_t H, int64_t W, hipStream_t st) {
  ADNM_REQUIRE(prev && last, "%s: null pointer", what);
  ADNM_REQUIRE(((uintptr_t)prev | (uintptr_t)last) % 4 == 0, "%s: prev and last must be 4-byte aligned", what);
  const char* why = nullptr;
  if (!trec_shape_ok(samples, H, W, block, &why)) {
    adnm_set_error("%s: %s (got samples %lld %lld x %lld block %lld)", what, why, (long long)samples, (long long)H, (long long)W, (long long)block);
    return ADNM_EINVAL;
  }
  ADNM_REQUIRE(radius >= 1 && radius <= kMaxR, "%s: radius must be in 1..8, got %lld", what, (long long)radius);
  ADNM_REQUIRE(echo >= 1 && echo <= 255, "%s: echo must be in 1..255, got %lld", what, (long long)echo);
  ADNM_REQUIRE(value_scale > 0.f && value_scale <= 255.f, "%s: value_scale must be in (0, 255] so that q fits a byte, got %g", what, (double)value_scale);
  ADNM_REQUIRE(sample_stride >= H * W, "%s: sample_stride must be >= H*W, got %lld", what, (long long)sample_stride);
  const int64_t need = adnm_trec_ws_bytes(samples, H, W, block, radius);
  if (!ws || ws_bytes < need) {
    adnm_set_error("%s: workspace %lld < %lld bytes", what, (long long)ws_bytes, (long long)need);
    return ADNM_EWORKSPACE;
  }
  ADNM_REQUIRE((uintptr_t)ws % 4 == 0, "%s: the workspace must be 4-byte aligned", what);
  const int nby = (int)adnm_cdiv(H, block), nbx = (int)adnm_cdiv(W, block);
  // 16-byte loads need every frame and row start of both frames aligned; anything else (an odd W, a 4-byte aligned slice) is read float
  // by float: same result
  const bool vec = W % 4 == 0 && sample_stride % 4 == 0 && adnm_quad_aligned(ADNM_F32, {prev, last});
  const int hs = (int)adnm_align(radius, 4);
  {
    ADNM_PROF("trec_cost", st, 8.0 * samples * H * W);
    const dim3 grid((unsigned)(nby * nbx), (unsigned)samples);   // nby * nbx <= 2^24 / 64
    if (vec)
      trec_cost_kernel<true><<<grid, kBlock, 0, st>>>(prev, last, sample_stride, (uint32_t*)ws, (int)H, (int)W, nbx, (int)block, (int)radius, hs, (int)echo,
                                                      value_scale);
    else
      trec_cost_kernel<false><<<grid, kBlock, 0, st>>>(prev, last, sample_stride, (uint32_t*)ws, (int)H, (int)W, nbx, (int)block, (int)radius, hs, (int)echo,
                                                       value_scale);
  }
  ADNM_CHECK_LAUNCH("trec_cost");
  return ADNM_OK;
}

extern "C" int adnm_trec_motion(const float* prev, const float* last, int64_t sample_stride, void* motion_i32, void* cost_out_u32_or_null, float value_scale,
                                int64_t block, int64_t radius, int64_t echo, void* ws, int64_t ws_bytes, int64_t samples, int64_t H, int64_t W,
                                adnm_stream_t stream) {
  ADNM_REQUIRE(motion_i32, "trec_motion: null pointer");
  ADNM_REQUIRE(((uintptr_t)motion_i32 | (uintptr_t)cost_out_u32_or_null) % 4 == 0, "trec_motion: motion and cost_out must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = adnm_trec_cost_launch("trec_motion", prev, last, sample_stride, value_scale, block, radius, echo, ws, ws_bytes, samples, H, W, st)) return rc;
  const int nby = (int)adnm_cdiv(H, block), nbx = (int)adnm_cdiv(W, block);
  const int64_t need = adnm_trec_ws_bytes(samples, H, W, block, radius);
  {
    ADNM_PROF("trec_pick", st, (double)need);
    trec_pick_kernel<<<(unsigned)samples, kBlock, 0, st>>>((const uint32_t*)ws, (int32_t*)motion_i32, (uint32_t*)cost_out_u32_or_null, nby * nbx, (int)block,
                                                           (int)radius);
  }
  ADNM_CHECK_LAUNCH("trec_pick");
  return ADNM_OK;
}

extern "C" int adnm_advect(const float* last, int64_t sample_stride, const void* motion_i32, float* out, int64_t block, int64_t samples, int64_t T, int64_t H,
                           int64_t W, adnm_stream_t stream) {
  ADNM_REQUIRE(last && motion_i32 && out, "advect: null pointer");
  ADNM_REQUIRE(((uintptr_t)last | (uintptr_t)out) % 4 == 0, "advect: last and out must be 4-byte aligned");
  ADNM_REQUIRE((uintptr_t)motion_i32 % 4 == 0, "advect: motion must be 4-byte aligned");
  const char* why = nullptr;
  if (!trec_shape_ok(samples, H, W, block, &why)) {
    adnm_set_error("advect: %s (got samples %lld %lld x %lld block %lld)", why, (long long)samples, (long long)H, (long long)W, (long long)block);
    return ADNM_EINVAL;
  }
  ADNM_REQUIRE(T >= 1, "advect: T must be >= 1, got %lld", (long long)T);
  ADNM_REQUIRE(sample_stride >= H * W, "advect: sample_stride must be >= H*W, got %lld", (long long)sample_stride);
  const int nby = (int)adnm_cdiv(H, block), nbx = (int)adnm_cdiv(W, block);
  const int64_t total = samples * T * H * adnm_cdiv(W, 4);
  const bool vec = W % 4 == 0 && adnm_quad_aligned(ADNM_F32, {out});
  const int64_t blocks = adnm_cdiv(total, kBlock);
  const unsigned grid = (unsigned)(blocks < (1 << 20) ? blocks : (1 << 20));
  hipStream_t st = (hipStream_t)stream;
  {
    ADNM_PROF("advect", st, 8.0 * samples * T * H * W);
    if (vec)
      advect_kernel<true><<<grid, kBlock, 0, st>>>((const uint32_t*)last, sample_stride, (const int32_t*)motion_i32, (uint32_t*)out, (int)block, nby, nbx, total,
                                                   T, (int)H, (int)W);
    else
      advect_kernel<false><<<grid, kBlock, 0, st>>>((const uint32_t*)last, sample_stride, (const int32_t*)motion_i32, (uint32_t*)out, (int)block, nby, nbx, total,
                                                    T, (int)H, (int)W);
  }
  ADNM_CHECK_LAUNCH("advect");
  return ADNM_OK;
}
