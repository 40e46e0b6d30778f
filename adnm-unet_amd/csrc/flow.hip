// The flow advection of the validation epoch (include/adnm_hip.h: adnm_trec_flow, adnm_flow_field, adnm_advect_flow): the
// block scheme's costs, picks and validity (advect.hip), refined to 1/16 px by a parabola through the pick's neighbours, spread to a dense
// field in 1/256 px by bilinear weights between the block centres, and the last frame carried backwards along that field one step per frame.
//
//   trec_cost    advect.hip's, through adnm_trec_cost_launch: the same tables in the same workspace.
//   trec_flow    one workgroup per sample: the 64-bit sum of the tables in block order into LDS, its pick g, the pick of every block and
//                validity exactly as trec_pick forms them; then each axis of a valid block is refined on the block's table and that of an
//                invalid block on the sum table.  -> u (and the integer motion, when asked for).
//   flow_field   V at every pixel from u: for inspection; the transport does not read it.
//   advect_flow  one launch.  A sample's u is staged in LDS (up to 4096 blocks; read from memory beyond that: same result), a lane owns four
//                pixels of a row for all T frames: D += V(nearest pixel of the departure point), four taps of `last`, one store.
//
// Integers up to the four taps; the interpolation is fp32 with every product and sum rounded on its own.  No atomics: the same bits
// whatever the workspace held.
#include "trec.h"

namespace {
constexpr int kBlock = 256;
constexpr int kMaxNd = (2 * kTrecMaxR + 1) * (2 * kTrecMaxR + 1);   // 289
constexpr int kLdsBlocks = 4096;                                     // a sample's vectors in LDS: 32 KB
constexpr int64_t kMaxT = 4096;                                      // |V| <= 16 * 136 per step: |D| < 2^24, 256 * 32767 + |D| < 2^31

// the vertex of the parabola through (-1, cm), (0, c0), (1, cp) in 1/16 px, rounded half away from zero; c0 <= cm, cp gives |.| <= 8
__device__ __forceinline__ int flow_delta(int64_t cm, int64_t c0, int64_t cp) {
  const int64_t den = cm - 2 * c0 + cp;
  if (den <= 0) return 0;
  const int64_t num = 8 * (cm - cp), mag = (2 * (num < 0 ? -num : num) + den) / (2 * den);
  return (int)(num < 0 ? -mag : mag);
}
// one axis (0: y, 1: x) of the pick (dy, dx) refined on table t (row dy + R, column dx + R): 16 d + delta, delta = 0 at the edge of the range
template <typename C>
__device__ __forceinline__ int flow_refine(const C* t, int dy, int dx, int R, int axis) {
  const int D = 2 * R + 1, d = axis == 0 ? dy : dx;
  if (d == R || d == -R) return 16 * d;
  const int at = (dy + R) * D + dx + R, step = axis == 0 ? D : 1;
  return 16 * d + flow_delta((int64_t)t[at - step], (int64_t)t[at], (int64_t)t[at + step]);
}

// grid (samples).  ws: trec_cost's tables.  u[s][b] = (uy, ux) in 1/16 px; motion (or null): trec_pick's vectors.
__global__ __launch_bounds__(kBlock) void trec_flow_kernel(const uint32_t* __restrict__ ws, int32_t* __restrict__ u, int32_t* __restrict__ motion, int nblk,
                                                           int bs, int R) {
  __shared__ uint64_t total[kMaxNd];
  __shared__ uint64_t red[kBlock / 64];
  const int s = blockIdx.x, D = 2 * R + 1, nd = D * D, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t* tab = ws + (int64_t)s * nblk * (nd + 1);
  uint64_t best = ~0ull;
  for (int d = threadIdx.x; d < nd; d += kBlock) {
    uint64_t sum = 0;
    for (int b = 0; b < nblk; ++b) sum += tab[(int64_t)b * (nd + 1) + d];
    total[d] = sum;
    const uint64_t k = trec_key(sum, d, R);
    best = k < best ? k : best;
  }
  best = trec_wave_min(best);
  if (lane == 0) red[wave] = best;
  __syncthreads();
  uint64_t g = red[0];
#pragma unroll
  for (int w = 1; w < kBlock / 64; ++w) g = red[w] < g ? red[w] : g;
  // a wave per block; lane 0 refines y, lane 1 refines x
  for (int b = wave; b < nblk; b += kBlock / 64) {
    const uint32_t* t = tab + (int64_t)b * (nd + 1);
    uint64_t k = ~0ull;
    for (int d = lane; d < nd; d += 64) {
      const uint64_t kd = trec_key(t[d], d, R);
      k = kd < k ? kd : k;
    }
    k = trec_wave_min(k);
    const bool valid = t[nd] >= (uint32_t)bs;
    if (!valid) k = g;
    if (lane < 2) {
      const int dy = (int)((k >> 5) & 31u) - R, dx = (int)(k & 31u) - R;
      const int64_t at = ((int64_t)s * nblk + b) * 2 + lane;
      u[at] = valid ? flow_refine(t, dy, dx, R, lane) : flow_refine(total, dy, dx, R, lane);
      if (motion) motion[at] = lane == 0 ? dy : dx;
    }
  }
}

// the two block centres around pixel y of an axis with nb blocks of 2^lb pixels and their integer weights, w0 + w1 = 2 block; the vectors
// are clamped at the outermost centres
struct FlowAxis {
  int b0, b1, w0, w1;
};
__device__ __forceinline__ FlowAxis flow_axis(int y, int nb, int lb) {
  const int bs = 1 << lb, p = 2 * y + 1 - bs;
  FlowAxis a;
  a.b0 = p < 0 ? 0 : min(p >> (lb + 1), nb - 1);
  a.w1 = p < 0 ? 0 : min(p - 2 * bs * a.b0, 2 * bs);   // p >= 2 bs b0 here
  a.b1 = min(a.b0 + 1, nb - 1);
  a.w0 = 2 * bs - a.w1;
  return a;
}
// V(y, x) in 1/256 px from a sample's u (1/16 px): S <= (2 block)^2 * 16 * 136 < 2^24
__device__ __forceinline__ int2 flow_vec(const int32_t* u, int y, int x, int nby, int nbx, int lb) {
  const FlowAxis ay = flow_axis(y, nby, lb), ax = flow_axis(x, nbx, lb);
  const int32_t *r0 = u + (ay.b0 * nbx) * 2, *r1 = u + (ay.b1 * nbx) * 2;
  const int half = 2 << (2 * lb), sh = 2 * lb + 2;
  int2 v;
  v.x = (16 * (ay.w0 * (ax.w0 * r0[2 * ax.b0] + ax.w1 * r0[2 * ax.b1]) + ay.w1 * (ax.w0 * r1[2 * ax.b0] + ax.w1 * r1[2 * ax.b1])) + half) >> sh;
  v.y = (16 * (ay.w0 * (ax.w0 * r0[2 * ax.b0 + 1] + ax.w1 * r0[2 * ax.b1 + 1]) + ay.w1 * (ax.w0 * r1[2 * ax.b0 + 1] + ax.w1 * r1[2 * ax.b1 + 1])) + half) >> sh;
  return v;
}

// one thread per pixel, grid-stride over samples * H * W
__global__ __launch_bounds__(kBlock) void flow_field_kernel(const int32_t* __restrict__ u, int32_t* __restrict__ field, int64_t total, int H, int W, int nby,
                                                            int nbx, int lb) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const int64_t s = i / ((int64_t)W * H);
    const int2 v = flow_vec(u + s * nby * nbx * 2, y, x, nby, nbx, lb);
    field[2 * i] = v.x, field[2 * i + 1] = v.y;
  }
}

__device__ __forceinline__ float flow_tap(const float* __restrict__ f, int y, int x, int H, int W) {
  return y >= 0 && y < H && x >= 0 && x < W ? f[(int64_t)y * W + x] : 0.f;
}
// the frame at (sy, sx) / 256: four taps, +0.0f outside the frame, a tap of weight 0 is not read (a whole-pixel position is a copy).  Every
// product and every sum is rounded to fp32 on its own.
__device__ __forceinline__ float flow_sample(const float* __restrict__ f, int sy, int sx, int H, int W) {
#pragma clang fp contract(off)
  const int iy = sy >> 8, ix = sx >> 8, ky = sy & 255, kx = sx & 255;
  const float fy = (float)ky * (1.f / 256.f), fx = (float)kx * (1.f / 256.f), gy = 1.f - fy, gx = 1.f - fx;   // exact
  float top = flow_tap(f, iy, ix, H, W);
  if (kx) {
    const float ta = gx * top, tb = fx * flow_tap(f, iy, ix + 1, H, W);
    top = ta + tb;
  }
  if (ky) {
    float bot = flow_tap(f, iy + 1, ix, H, W);
    if (kx) {
      const float tc = gx * bot, td = fx * flow_tap(f, iy + 1, ix + 1, H, W);
      bot = tc + td;
    }
    const float tt = gy * top, tb = fy * bot;
    top = tt + tb;
  }
  return top;
}

// grid (ceil(H * ceil(W / 4) / blockDim.x), samples); dynamic LDS: LDS ? nby * nbx * 8 bytes : 0.  One thread per four pixels of a row, for
// all T frames.  VEC: W % 4 == 0 and out 16-byte aligned.
template <bool VEC, bool LDS>
__global__ __launch_bounds__(kBlock) void advect_flow_kernel(const float* __restrict__ last, int64_t sstride, const int32_t* __restrict__ u,
                                                             float* __restrict__ out, int lb, int nby, int nbx, int T, int H, int W) {
  extern __shared__ int32_t flow_u[];
  const int s = blockIdx.y, wq = (W + 3) >> 2, nu = nby * nbx * 2;
  const int32_t* us = u + (int64_t)s * nu;
  if (LDS) {
    for (int i = threadIdx.x; i < nu; i += blockDim.x) flow_u[i] = us[i];
    __syncthreads();
    us = flow_u;
  }
  const int item = blockIdx.x * blockDim.x + threadIdx.x;   // < 2^24
  if (item >= H * wq) return;
  const int y = item / wq, x = (item % wq) * 4;
  const float* lf = last + (int64_t)s * sstride;
  float* dst = out + (((int64_t)s * T) * H + y) * W + x;
  int dy[4] = {0, 0, 0, 0}, dx[4] = {0, 0, 0, 0};
  for (int t = 0; t < T; ++t, dst += (int64_t)H * W) {
    float px[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      px[e] = 0.f;
      if (VEC || x + e < W) {
        const int ry = min(max((256 * y - dy[e] + 128) >> 8, 0), H - 1), rx = min(max((256 * (x + e) - dx[e] + 128) >> 8, 0), W - 1);
        const int2 v = flow_vec(us, ry, rx, nby, nbx, lb);
        dy[e] += v.x, dx[e] += v.y;
        px[e] = flow_sample(lf, 256 * y - dy[e], 256 * (x + e) - dx[e], H, W);
      }
    }
    if (VEC) {
      *(float4*)dst = make_float4(px[0], px[1], px[2], px[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (x + e < W) dst[e] = px[e];
    }
  }
}

int flow_log2(int64_t block) { return block == 8 ? 3 : block == 16 ? 4 : 5; }
}  // namespace

extern "C" int64_t adnm_trec_flow_ws_bytes(int64_t samples, int64_t H, int64_t W, int64_t block, int64_t radius) {
  return adnm_trec_ws_bytes(samples, H, W, block, radius);
}

extern "C" int adnm_trec_flow(const float* prev, const float* last, int64_t sample_stride, void* flow_i32, void* motion_i32_or_null, float value_scale,
                              int64_t block, int64_t radius, int64_t echo, void* ws, int64_t ws_bytes, int64_t samples, int64_t H, int64_t W,
                              adnm_stream_t stream) {
  ADNM_REQUIRE(flow_i32, "trec_flow: null pointer");
  ADNM_REQUIRE(((uintptr_t)flow_i32 | (uintptr_t)motion_i32_or_null) % 4 == 0, "trec_flow: flow and motion must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = adnm_trec_cost_launch("trec_flow", prev, last, sample_stride, value_scale, block, radius, echo, ws, ws_bytes, samples, H, W, st)) return rc;
  const int nblk = (int)(adnm_cdiv(H, block) * adnm_cdiv(W, block));
  {
    ADNM_PROF("trec_flow", st, (double)adnm_trec_ws_bytes(samples, H, W, block, radius));
    trec_flow_kernel<<<(unsigned)samples, kBlock, 0, st>>>((const uint32_t*)ws, (int32_t*)flow_i32, (int32_t*)motion_i32_or_null, nblk, (int)block, (int)radius);
  }
  ADNM_CHECK_LAUNCH("trec_flow");
  return ADNM_OK;
}

extern "C" int adnm_flow_field(const void* flow_i32, void* field_i32, int64_t block, int64_t samples, int64_t H, int64_t W, adnm_stream_t stream) {
  ADNM_REQUIRE(flow_i32 && field_i32, "flow_field: null pointer");
  ADNM_REQUIRE(((uintptr_t)flow_i32 | (uintptr_t)field_i32) % 4 == 0, "flow_field: flow and field must be 4-byte aligned");
  const char* why = nullptr;
  if (!trec_shape_ok(samples, H, W, block, &why)) {
    adnm_set_error("flow_field: %s (got samples %lld %lld x %lld block %lld)", why, (long long)samples, (long long)H, (long long)W, (long long)block);
    return ADNM_EINVAL;
  }
  const int64_t total = samples * H * W, blocks = adnm_cdiv(total, kBlock);
  const unsigned grid = (unsigned)(blocks < (1 << 20) ? blocks : (1 << 20));
  hipStream_t st = (hipStream_t)stream;
  {
    ADNM_PROF("flow_field", st, 8.0 * total);
    flow_field_kernel<<<grid, kBlock, 0, st>>>((const int32_t*)flow_i32, (int32_t*)field_i32, total, (int)H, (int)W, (int)adnm_cdiv(H, block),
                                               (int)adnm_cdiv(W, block), flow_log2(block));
  }
  ADNM_CHECK_LAUNCH("flow_field");
  return ADNM_OK;
}

extern "C" int adnm_advect_flow(const float* last, int64_t sample_stride, const void* flow_i32, float* out, int64_t block, int64_t samples, int64_t T,
                                int64_t H, int64_t W, adnm_stream_t stream) {
  ADNM_REQUIRE(last && flow_i32 && out, "advect_flow: null pointer");
  ADNM_REQUIRE(((uintptr_t)last | (uintptr_t)out) % 4 == 0, "advect_flow: last and out must be 4-byte aligned");
  ADNM_REQUIRE((uintptr_t)flow_i32 % 4 == 0, "advect_flow: flow must be 4-byte aligned");
  const char* why = nullptr;
  if (!trec_shape_ok(samples, H, W, block, &why)) {
    adnm_set_error("advect_flow: %s (got samples %lld %lld x %lld block %lld)", why, (long long)samples, (long long)H, (long long)W, (long long)block);
    return ADNM_EINVAL;
  }
  ADNM_REQUIRE(T >= 1 && T <= kMaxT, "advect_flow: T must be in 1..4096 (the displacement is followed in int32), got %lld", (long long)T);
  ADNM_REQUIRE(sample_stride >= H * W, "advect_flow: sample_stride must be >= H*W, got %lld", (long long)sample_stride);
  const int nby = (int)adnm_cdiv(H, block), nbx = (int)adnm_cdiv(W, block), lb = flow_log2(block);
  const int64_t items = H * adnm_cdiv(W, 4);
  const bool vec = W % 4 == 0 && adnm_quad_aligned(ADNM_F32, {out}), lds = (int64_t)nby * nbx <= kLdsBlocks;
  // a lane's chain over t is sequential: small batches get one wave per workgroup, so that they spread over more compute units
  const int threads = samples * items <= 65536 ? 64 : kBlock;
  const dim3 grid((unsigned)adnm_cdiv(items, threads), (unsigned)samples);
  const size_t smem = lds ? (size_t)nby * nbx * 2 * sizeof(int32_t) : 0;
  hipStream_t st = (hipStream_t)stream;
  {
    ADNM_PROF("advect_flow", st, 4.0 * samples * (T + 1) * H * W);
#define ADNM_FLOW_LAUNCH(V, L) \
  advect_flow_kernel<V, L><<<grid, threads, smem, st>>>(last, sample_stride, (const int32_t*)flow_i32, out, lb, nby, nbx, (int)T, (int)H, (int)W)
    if (vec && lds) ADNM_FLOW_LAUNCH(true, true);
    else if (vec) ADNM_FLOW_LAUNCH(true, false);
    else if (lds) ADNM_FLOW_LAUNCH(false, true);
    else ADNM_FLOW_LAUNCH(false, false);
#undef ADNM_FLOW_LAUNCH
  }
  ADNM_CHECK_LAUNCH("advect_flow");
  return ADNM_OK;
}
