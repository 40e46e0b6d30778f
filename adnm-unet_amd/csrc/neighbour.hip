// The two neighbourhood scores of a scored pair (scored_pair.h): pooled contingency counts (include/adnm_hip.h: adnm_valid_pool_accum;
// DESIGN.md §4h) and the Fractions Skill Score's windowed sums (adnm_valid_fss_accum; §4i).  Both cut a frame into 32 x 32 tiles, one
// workgroup per (tile, frame).  A workgroup stages its tile and the margin its windows reach into ONCE, as pair_bits' 2 bytes per pixel in
// LDS (low byte target, high byte forecast), and serves every pool or scale and every threshold from that image in integers.  Each pass
// leaves 3 * nthr uint32 per workgroup, part[frame][tile][pass][3 * nthr], and one fold adds them to the table in double, in a fixed
// order.  What the two share is written once: the stager, the store of a pass's counts and the fold.  Behind them stand the neighbourhood
// exceedance probability's histogram (adnm_valid_nprob_accum; §4r), which shares the FSS pass's staging and running sums and flushes an LDS
// histogram instead of partials, and the probability field itself (adnm_neighbour_prob); and the intensity-scale skill score's dyadic
// block sums (adnm_valid_iscale_accum; §4t), which stage the same bits with no halo and have a fold of their own.
#include "scored_pair.h"

namespace {
constexpr int kBlock = 256, kFoldBlock = 256, kTile = 32;

// The event bits of the rectangle [y0, y0 + rows) x [x0, x0 + cols) of one frame (tp: the target's, pp: the forecast's first pixel)
// -> img[r * PITCH + c], 0 where the rectangle leaves the frame (INSIDE: the caller has clipped it, nothing is tested).  VEC: W, x0
// and cols are multiples of 4 and every row of both fields starts on 16 bytes (pair_quads), so four columns are one 16-byte load per
// field and lie inside or outside the frame as a whole.  Their four results leave as one 8-byte store where PITCH keeps a row start
// 8-byte aligned, as two 4-byte stores where it does not.
template <bool VEC, int PITCH, bool INSIDE>
__device__ __forceinline__ void stage_pair_bits(uint16_t* img, const float* __restrict__ tp, const float* __restrict__ pp, int H, int W, int y0, int x0,
                                                int rows, int cols, float value_scale, const Thr& thr) {
  if (VEC) {
    const int q = cols >> 2;
    for (int i = threadIdx.x; i < rows * q; i += kBlock) {
      const int r = i / q, c = (i % q) * 4, gy = y0 + r, gx = x0 + c;
      uint32_t lo = 0, hi = 0;
      if (INSIDE || (gy >= 0 && gy < H && gx >= 0 && gx < W)) {
        const float4 a = *(const float4*)(tp + (int64_t)gy * W + gx), b = *(const float4*)(pp + (int64_t)gy * W + gx);
        lo = pair_bits(a.x, b.x, value_scale, thr) | (pair_bits(a.y, b.y, value_scale, thr) << 16);
        hi = pair_bits(a.z, b.z, value_scale, thr) | (pair_bits(a.w, b.w, value_scale, thr) << 16);
      }
      if constexpr (PITCH % 4 == 0) {
        *(uint2*)&img[r * PITCH + c] = make_uint2(lo, hi);
      } else {
        uint32_t* dst = (uint32_t*)&img[r * PITCH + c];   // c and PITCH are even: 4-byte aligned
        dst[0] = lo;
        dst[1] = hi;
      }
    }
  } else {
    for (int i = threadIdx.x; i < rows * cols; i += kBlock) {
      const int r = i / cols, c = i % cols, gy = y0 + r, gx = x0 + c;
      uint32_t m = 0;
      if (INSIDE || (gy >= 0 && gy < H && gx >= 0 && gx < W)) m = pair_bits(tp[(int64_t)gy * W + gx], pp[(int64_t)gy * W + gx], value_scale, thr);
      img[r * PITCH + c] = (uint16_t)m;
    }
  }
}

// A pass's counts leave the workgroup: v[k], k < nout, is this WAVE's count (the same in every lane) -> red -> the four waves added as
// (0 + 1) + (2 + 3) -> part[frame][tile][pass p of npass][k].  Ends synchronised: the next pass may rewrite red and whatever it read.
__device__ __forceinline__ void store_part(uint32_t* __restrict__ part, uint32_t (*red)[3 * kMaxThr], const uint32_t (&v)[3 * kMaxThr], int f, int tile,
                                           int npass, int p, int nout) {
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 3 * kMaxThr; ++k)
      if (k < nout) red[threadIdx.x >> 6][k] = v[k];
  }
  __syncthreads();
  if ((int)threadIdx.x < nout)
    part[(((int64_t)f * gridDim.x + tile) * npass + p) * nout + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
  __syncthreads();
}

// One thread per (t, pass, threshold): the three uint32 columns of part[frame b * T + t][tile][pass][3k .. 3k + 2] summed in a fixed
// order (samples ascending, then tiles ascending: valid_fold_kernel's), in double arithmetic on integers, and handed to
// fin(t, p, k, B, s0, s1, s2), which adds the batch to the table.
template <typename FIN>
__device__ __forceinline__ void tile_fold(const uint32_t* __restrict__ part, int tiles, int frames, int T, int nthr, int npass, const FIN& fin) {
  const int B = frames / T, i = blockIdx.x * kFoldBlock + threadIdx.x;
  if (i >= T * npass * nthr) return;
  const int k = i % nthr, p = (i / nthr) % npass, t = i / (nthr * npass);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int b = 0; b < B; ++b)
    for (int tile = 0; tile < tiles; ++tile) {
      const uint32_t* q = part + ((((int64_t)b * T + t) * tiles + tile) * npass + p) * (3 * nthr) + 3 * k;
      s0 += (double)q[0], s1 += (double)q[1], s2 += (double)q[2];
    }
  fin(t, p, k, B, s0, s1, s2);
}
inline int64_t tiles_of(int64_t H, int64_t W) { return adnm_cdiv(H, kTile) * adnm_cdiv(W, kTile); }

// ---- neighbourhood (pooled) contingency counts ----
// A window of a pool (s, d) is an event at threshold k iff ANY pixel of it has q >= thr_k (thresholding commutes with the max), so a
// pixel's whole state is one byte per field (bit k = q >= thr_k) and max-pooling is a windowed OR.  A workgroup owns the windows whose
// top-left pixel lies in its tile.  From the staged image it serves every pool and every threshold: OR along rows, then along columns,
// then per bit the number of windows with the target bit, the forecast bit and both.  Those are wave ballots summed in scalar registers:
// integers throughout.  The fold turns (obs, sim, both) into TP, FN, FP, TN.
constexpr int kPoolMax = 4, kPoolWin = 32;
constexpr int kPoolSide = kTile + kPoolWin;   // staged rows / columns at most: a window reaches at most s - 1 <= 31 past the tile
constexpr int kPoolPitch = kPoolSide + 4;     // uint16 per staged row: 136 bytes, so that a row start stays 8-byte aligned
struct Pools {
  int s[kPoolMax], d[kPoolMax], n;
};

// grid (tiles, frames).  ext: how far past the tile the staged image goes (host: the largest s - gcd(d, 32) of the pools; VEC: rounded
// up to 4).  The staged rectangle is clipped to the frame: no window reads past rh x rw.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void pool_counts_kernel(ScoredPair pair, uint32_t* __restrict__ part, int H, int W, int tiles_x, int ext,
                                                             float value_scale, Thr thr, Pools pools) {
  __shared__ __attribute__((aligned(8))) uint16_t img[kPoolSide][kPoolPitch];
  __shared__ uint16_t rowor[kPoolSide][kTile + 1];
  __shared__ uint32_t red[kBlock / 64][3 * kMaxThr];
  const int f = blockIdx.y, tile = blockIdx.x, oy = (tile / tiles_x) * kTile, ox = (tile % tiles_x) * kTile;
  const int rh = min(kTile + ext, H - oy), rw = min(kTile + ext, W - ox);   // VEC: rw is a multiple of 4, as W, ox and 32 + ext are
  stage_pair_bits<VEC, kPoolPitch, true>(&img[0][0], pair.target(f), pair.forecast(f), H, W, oy, ox, rh, rw, value_scale, thr);
  __syncthreads();
  const int nout = 3 * thr.n;
  for (int p = 0; p < pools.n; ++p) {
    const int s = pools.s[p], d = pools.d[p];
    // the windows anchored in this tile: indices [j0, j0 + na) along each axis, the first one at offset c0 from the tile's origin
    const int jx0 = (ox + d - 1) / d, jy0 = (oy + d - 1) / d;
    const int nax = max(0, min((W - s) / d + 1, (ox + kTile + d - 1) / d) - jx0), nay = max(0, min((H - s) / d + 1, (oy + kTile + d - 1) / d) - jy0);
    const int cx0 = jx0 * d - ox, cy0 = jy0 * d - oy;
    for (int i = threadIdx.x; i < rh * nax; i += kBlock) {
      const int r = i / nax, j = i % nax;
      const uint16_t* src = &img[r][cx0 + j * d];   // cx0 + j*d + s <= min(W - ox, 32 + ext) = rw
      uint32_t m = 0;
      for (int u = 0; u < s; ++u) m |= src[u];
      rowor[r][j] = (uint16_t)m;
    }
    __syncthreads();
    uint32_t cnt[3 * kMaxThr];   // wave-uniform: windows with the target bit k, the forecast bit k, both
#pragma unroll
    for (int k = 0; k < 3 * kMaxThr; ++k) cnt[k] = 0;
    const int na = nax * nay;
    for (int i0 = 0; i0 < na; i0 += kBlock) {   // the same trips for every lane: the ballots below see whole waves
      const int i = i0 + threadIdx.x;
      uint32_t m = 0;
      if (i < na) {
        const int r0 = cy0 + (i / nax) * d, j = i % nax;   // r0 + s <= rh
        for (int u = 0; u < s; ++u) m |= rowor[r0 + u][j];
      }
      const uint32_t o = m & 0xffu, sim = m >> 8, v = o | (sim << 8) | ((o & sim) << 16);
#pragma unroll
      for (int k = 0; k < kMaxThr; ++k)
        if (k < thr.n) {
#pragma unroll
          for (int c = 0; c < 3; ++c) cnt[3 * k + c] += (uint32_t)__popcll(__ballot((v >> (8 * c + k)) & 1u));
        }
    }
    store_part(part, red, cnt, f, tile, pools.n, p, nout);   // rowor too is rewritten by the next pool
  }
}

// table[t][pool][4k .. 4k+3] += TP, FN, FP, TN of the batch, TN from the number of windows of the pool
__global__ __launch_bounds__(kFoldBlock) void pool_fold_kernel(const uint32_t* __restrict__ part, int tiles, int frames, int T, int nthr, int H, int W,
                                                               Pools pools, double* __restrict__ table) {
  tile_fold(part, tiles, frames, T, nthr, pools.n, [&](int t, int p, int k, int B, double obs, double sim, double both) {
    const double windows = (double)B * (double)((H - pools.s[p]) / pools.d[p] + 1) * (double)((W - pools.s[p]) / pools.d[p] + 1);
    double* out = table + ((int64_t)t * pools.n + p) * (4 * nthr) + 4 * k;
    out[0] += both;
    out[1] += obs - both;
    out[2] += sim - both;
    out[3] += windows - obs - sim + both;
  });
}

int pool_gcd(int a, int b) { return b == 0 ? a : pool_gcd(b, a % b); }

// the pooled pass's own limits: nullptr, or the one that refuses
const char* pool_why(int64_t frames, int64_t T, int64_t H, int64_t W, int64_t nthr, const int64_t* pools_host, int64_t npool) {
  if (!pools_host) return "null pointer";
  if (npool < 1 || npool > kPoolMax) return "1..4 pools";
  if (nthr < 1 || nthr > kMaxThr) return "1..8 thresholds";
  if (const char* w = pair_frames_why(frames, T)) return w;
  if (const char* w = pair_tiled_shape_why(H, W)) return w;
  for (int64_t p = 0; p < npool; ++p) {
    const int64_t s = pools_host[2 * p], d = pools_host[2 * p + 1];
    if (!(1 <= d && d <= s && s <= kPoolWin)) return "a pool needs 1 <= stride <= size <= 32";
    if (s > (H < W ? H : W)) return "a pool window is larger than the frame";
  }
  return nullptr;
}
}  // namespace

extern "C" int64_t adnm_valid_pool_block_bytes(int64_t T, int64_t nthr, int64_t npool) {
  if (T < 1 || T > 65535 || nthr < 1 || nthr > kMaxThr || npool < 1 || npool > kPoolMax) return -1;
  return (int64_t)sizeof(double) * T * npool * 4 * nthr;
}

extern "C" int64_t adnm_valid_pool_accum_ws_bytes(int64_t frames, int64_t T, int64_t H, int64_t W, int64_t nthr, const int64_t* pools_host, int64_t npool) {
  if (pool_why(frames, T, H, W, nthr, pools_host, npool)) return -1;
  return frames * tiles_of(H, W) * npool * 3 * nthr * (int64_t)sizeof(uint32_t);
}

extern "C" int adnm_valid_pool_accum(const float* pred, int64_t pred_sample_stride, int64_t pred_frame_stride, const float* target, void* table,
                                     const float* thresholds_host, int64_t nthr, float value_scale, const int64_t* pools_host, int64_t npool, void* ws,
                                     int64_t ws_bytes, int64_t frames, int64_t T, int64_t H, int64_t W, adnm_stream_t stream) {
  const PairCall call = {"valid_pool_accum", pred, pred_sample_stride, pred_frame_stride, target, table, ws, ws_bytes, H, W,
                         /*flat*/ false, /*ws_optional*/ false, /*ws_aligned*/ false, /*ws_rc*/ ADNM_EWORKSPACE};
  if (int rc = pair_check(call, thresholds_host && pools_host, pool_why(frames, T, H, W, nthr, pools_host, npool),
                          adnm_valid_pool_accum_ws_bytes(frames, T, H, W, nthr, pools_host, npool),
                          "frames %lld T %lld %lld x %lld nthr %lld npool %lld", (long long)frames, (long long)T, (long long)H, (long long)W,
                          (long long)nthr, (long long)npool))
    return rc;
  const Thr thr = thr_fill(thresholds_host, nthr);
  Pools pools;
  pools.n = (int)npool;
  int ext = 0;
  for (int p = 0; p < kPoolMax; ++p) {
    pools.s[p] = p < npool ? (int)pools_host[2 * p] : 1;
    pools.d[p] = p < npool ? (int)pools_host[2 * p + 1] : 1;
    // windows start at multiples of d and tiles at multiples of 32: the last start in a tile is at most 32 - gcd(d, 32) into it
    const int e = pools.s[p] - pool_gcd(pools.d[p], kTile);
    ext = e > ext ? e : ext;
  }
  const bool vec = pair_quads(W, pred_sample_stride, pred_frame_stride, pred, target);
  if (vec) ext = (int)adnm_align(ext, 4);
  const ScoredPair pair = {pred, pred_sample_stride, pred_frame_stride, target, (int)T, (int)(H * W)};
  const int tiles_x = (int)adnm_cdiv(W, kTile), tiles = (int)tiles_of(H, W);
  hipStream_t st = (hipStream_t)stream;
  {
    ADNM_PROF("valid_pool", st, 8.0 * frames * H * W);
    const dim3 grid((unsigned)tiles, (unsigned)frames);
    if (vec) pool_counts_kernel<true><<<grid, kBlock, 0, st>>>(pair, (uint32_t*)ws, (int)H, (int)W, tiles_x, ext, value_scale, thr, pools);
    else pool_counts_kernel<false><<<grid, kBlock, 0, st>>>(pair, (uint32_t*)ws, (int)H, (int)W, tiles_x, ext, value_scale, thr, pools);
  }
  ADNM_CHECK_LAUNCH("valid_pool_accum");
  {
    ADNM_PROF("valid_pool_fold", st, 4.0 * frames * tiles * npool * 3 * nthr);
    pool_fold_kernel<<<(unsigned)adnm_cdiv(T * npool * nthr, kFoldBlock), kFoldBlock, 0, st>>>((const uint32_t*)ws, tiles, (int)frames, (int)T, (int)nthr, (int)H,
                                                                                             (int)W, pools, (double*)table);
  }
  ADNM_CHECK_LAUNCH("valid_pool_fold");
  return ADNM_OK;
}

// ---- Fractions Skill Score: windowed fraction sums ----
// c_o(y, x) / c_f(y, x): the number of threshold-k pixels of the target / the forecast in the n x n window CENTRED on (y, x), zero outside
// the frame.  A workgroup owns the 32 x 32 window centres of its tile.  It stages the tile and a halo of hs >= max(n) / 2 pixels on all
// four sides (0 outside the frame), and serves every scale and threshold from that image, separably and with running sums:
//   rows     wave q takes nibble q of the pixel (0, 1: target thresholds 0-3, 4-7; 2, 3: forecast), lane R the staged row R.  A nibble
//            is spread to one count per BYTE (bit j -> byte j), and a running sum along the row (add the pixel entering the window,
//            take the one leaving) gives the four thresholds' row counts (<= 33 each: bytes never carry) for the 32 centres' columns.
//   columns  a thread owns 4 consecutive centres of one column; the row counts are summed down the window in 16-bit lanes (even bytes
//            in one dword, odd bytes in another; <= 1089 each), again running: n adds for the first centre, one add and one
//            subtraction for each of the next three.
// c_o^2, c_f^2, c_o c_f per lane in uint32 (a tile's sum is at most 1024 * 1089^2 < 2^32), integer adds across the wave and the four
// waves.  LDS: image rows 33 dwords and row-count rows 33 dwords apart, so the lanes of the row pass (one row each) and of the column
// pass (consecutive columns) hit distinct banks.  The pooled pass's pitch cannot serve here (34 dwords: an even row distance puts two
// lanes of the row pass on one bank), nor this one there (132-byte rows are not 8-byte aligned): the stager takes the pitch as a parameter.
namespace {
constexpr int kFssMax = 4, kFssWin = 33;
constexpr int kFssSide = kTile + 2 * (kFssWin / 2);   // 64 staged rows / columns at most
constexpr int kFssPitch = kFssSide + 2;               // uint16 per staged row: 33 dwords
struct Scales {
  int n[kFssMax], cnt;
};

// bit j of a nibble -> byte j of a dword (0 or 1): x * (1 + 2^7 + 2^14 + 2^21) puts bit j at 8j among 16 distinct positions (no carries)
__device__ __forceinline__ uint32_t fss_spread(uint32_t nibble) { return (nibble * 0x00204081u) & 0x01010101u; }

__device__ __forceinline__ uint32_t fss_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

// grid (tiles, frames).  hs: the staged halo (host: the largest n / 2; VEC: rounded up to 4, so that the staged columns start at a
// multiple of 4).
template <bool VEC>
__global__ __launch_bounds__(kBlock) void fss_sums_kernel(ScoredPair pair, uint32_t* __restrict__ part, int H, int W, int tiles_x, int hs,
                                                          float value_scale, Thr thr, Scales scales) {
  __shared__ __attribute__((aligned(4))) uint16_t img[kFssSide][kFssPitch];
  __shared__ uint32_t rs[4][kFssSide][kTile + 1];   // [nibble][staged row][centre column]: four thresholds' row counts, one per byte
  __shared__ uint32_t red[kBlock / 64][3 * kMaxThr];
  const int f = blockIdx.y, tile = blockIdx.x, oy = (tile / tiles_x) * kTile, ox = (tile % tiles_x) * kTile;
  const int side = kTile + 2 * hs;
  stage_pair_bits<VEC, kFssPitch, false>(&img[0][0], pair.target(f), pair.forecast(f), H, W, oy - hs, ox - hs, side, side, value_scale, thr);
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nout = 3 * thr.n;
  const int cx = threadIdx.x & 31, cy0 = (threadIdx.x >> 5) * 4;   // the column pass: centres (cy0 .. cy0 + 3, cx) of the tile
  const bool col_in = ox + cx < W;
  for (int p = 0; p < scales.cnt; ++p) {
    const int n = scales.n[p], r = n >> 1, c0 = hs - r;   // centre x's window: staged columns c0 + x .. c0 + x + n - 1 (<= 2*hs + 31 < side)
    if (lane < side && (thr.n > 4 || !(wave & 1))) {      // (nibbles 1 and 3 hold thresholds 4-7)
      const uint16_t* row = img[lane];
      const int sh = 4 * wave;
      uint32_t s = 0;
      for (int u = 0; u < n - 1; ++u) s += fss_spread((row[c0 + u] >> sh) & 0xfu);
      for (int x = 0; x < kTile; ++x) {
        s += fss_spread((row[c0 + x + n - 1] >> sh) & 0xfu);
        rs[wave][lane][x] = s;
        s -= fss_spread((row[c0 + x] >> sh) & 0xfu);   // it was added: no byte borrows
      }
    }
    __syncthreads();
    // acc[q][e]: nibble q's bytes e and e + 2 as 16-bit lanes; centre y's window: staged rows c0 + y .. c0 + y + n - 1
    uint32_t acc[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    uint32_t sum[3 * kMaxThr];
#pragma unroll
    for (int k = 0; k < 3 * kMaxThr; ++k) sum[k] = 0;
    auto rows = [&](int R, bool add) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (thr.n > 4 || !(q & 1)) {
          const uint32_t v = rs[q][R][cx], e = v & 0x00ff00ffu, o = (v >> 8) & 0x00ff00ffu;
          acc[q][0] = add ? acc[q][0] + e : acc[q][0] - e;
          acc[q][1] = add ? acc[q][1] + o : acc[q][1] - o;
        }
    };
    for (int u = 0; u < n - 1; ++u) rows(c0 + cy0 + u, true);
    for (int j = 0; j < 4; ++j) {
      rows(c0 + cy0 + j + n - 1, true);   // <= 2*hs + 31 < side
      if (col_in && oy + cy0 + j < H) {
#pragma unroll
        for (int k = 0; k < kMaxThr; ++k)
          if (k < thr.n) {
            const int sh = 16 * ((k & 3) >> 1);
            const uint32_t co = (acc[k >> 2][k & 1] >> sh) & 0xffffu, cf = (acc[2 + (k >> 2)][k & 1] >> sh) & 0xffffu;
            sum[3 * k + 0] += co * co;
            sum[3 * k + 1] += cf * cf;
            sum[3 * k + 2] += co * cf;
          }
      }
      rows(c0 + cy0 + j, false);
    }
#pragma unroll
    for (int k = 0; k < 3 * kMaxThr; ++k)
      if (k < nout) sum[k] = fss_wave_sum(sum[k]);
    store_part(part, red, sum, f, tile, scales.cnt, p, nout);   // rs too is rewritten by the next scale
  }
}

// table[t][scale][3k .. 3k+2] += A, F, C of the batch
__global__ __launch_bounds__(kFoldBlock) void fss_fold_kernel(const uint32_t* __restrict__ part, int tiles, int frames, int T, int nthr, int ns,
                                                              double* __restrict__ table) {
  tile_fold(part, tiles, frames, T, nthr, ns, [&](int t, int p, int k, int, double a, double fc, double c) {
    double* out = table + ((int64_t)t * ns + p) * (3 * nthr) + 3 * k;
    out[0] += a;
    out[1] += fc;
    out[2] += c;
  });
}

// the FSS pass's own limits: nullptr, or the one that refuses
const char* fss_why(int64_t frames, int64_t T, int64_t H, int64_t W, int64_t nthr, const int64_t* scales_host, int64_t nscale) {
  if (!scales_host) return "null pointer";
  if (nscale < 1 || nscale > kFssMax) return "1..4 scales";
  if (nthr < 1 || nthr > kMaxThr) return "1..8 thresholds";
  if (const char* w = pair_frames_why(frames, T)) return w;
  if (const char* w = pair_tiled_shape_why(H, W)) return w;
  for (int64_t p = 0; p < nscale; ++p) {
    const int64_t n = scales_host[p];
    if (n < 1 || n > kFssWin || n % 2 == 0) return "a scale must be odd and in 1..33";
    for (int64_t o = 0; o < p; ++o)
      if (scales_host[o] == n) return "a scale is given twice";
  }
  return nullptr;
}
}  // namespace

extern "C" int64_t adnm_valid_fss_block_bytes(int64_t T, int64_t nthr, int64_t nscale) {
  if (T < 1 || T > 65535 || nthr < 1 || nthr > kMaxThr || nscale < 1 || nscale > kFssMax) return -1;
  return (int64_t)sizeof(double) * T * nscale * 3 * nthr;
}

extern "C" int64_t adnm_valid_fss_accum_ws_bytes(int64_t frames, int64_t T, int64_t H, int64_t W, int64_t nthr, const int64_t* scales_host, int64_t nscale) {
  if (fss_why(frames, T, H, W, nthr, scales_host, nscale)) return -1;
  return frames * tiles_of(H, W) * nscale * 3 * nthr * (int64_t)sizeof(uint32_t);
}

extern "C" int adnm_valid_fss_accum(const float* pred, int64_t pred_sample_stride, int64_t pred_frame_stride, const float* target, void* table,
                                    const float* thresholds_host, int64_t nthr, float value_scale, const int64_t* scales_host, int64_t nscale, void* ws,
                                    int64_t ws_bytes, int64_t frames, int64_t T, int64_t H, int64_t W, adnm_stream_t stream) {
  const PairCall call = {"valid_fss_accum", pred, pred_sample_stride, pred_frame_stride, target, table, ws, ws_bytes, H, W,
                         /*flat*/ false, /*ws_optional*/ false, /*ws_aligned*/ false, /*ws_rc*/ ADNM_EWORKSPACE};
  if (int rc = pair_check(call, thresholds_host && scales_host, fss_why(frames, T, H, W, nthr, scales_host, nscale),
                          adnm_valid_fss_accum_ws_bytes(frames, T, H, W, nthr, scales_host, nscale),
                          "frames %lld T %lld %lld x %lld nthr %lld nscale %lld", (long long)frames, (long long)T, (long long)H, (long long)W,
                          (long long)nthr, (long long)nscale))
    return rc;
  const Thr thr = thr_fill(thresholds_host, nthr);
  Scales scales;
  scales.cnt = (int)nscale;
  int hs = 0;
  for (int p = 0; p < kFssMax; ++p) {
    scales.n[p] = p < nscale ? (int)scales_host[p] : 1;
    hs = scales.n[p] / 2 > hs ? scales.n[p] / 2 : hs;
  }
  const bool vec = pair_quads(W, pred_sample_stride, pred_frame_stride, pred, target);
  if (vec) hs = (int)adnm_align(hs, 4);   // <= 16
  const ScoredPair pair = {pred, pred_sample_stride, pred_frame_stride, target, (int)T, (int)(H * W)};
  const int tiles_x = (int)adnm_cdiv(W, kTile), tiles = (int)tiles_of(H, W);
  hipStream_t st = (hipStream_t)stream;
  {
    ADNM_PROF("valid_fss", st, 8.0 * frames * H * W);
    const dim3 grid((unsigned)tiles, (unsigned)frames);
    if (vec) fss_sums_kernel<true><<<grid, kBlock, 0, st>>>(pair, (uint32_t*)ws, (int)H, (int)W, tiles_x, hs, value_scale, thr, scales);
    else fss_sums_kernel<false><<<grid, kBlock, 0, st>>>(pair, (uint32_t*)ws, (int)H, (int)W, tiles_x, hs, value_scale, thr, scales);
  }
  ADNM_CHECK_LAUNCH("valid_fss_accum");
  {
    ADNM_PROF("valid_fss_fold", st, 4.0 * frames * tiles * nscale * 3 * nthr);
    fss_fold_kernel<<<(unsigned)adnm_cdiv(T * nscale * nthr, kFoldBlock), kFoldBlock, 0, st>>>((const uint32_t*)ws, tiles, (int)frames, (int)T, (int)nthr,
                                                                                            (int)nscale, (double*)table);
  }
  ADNM_CHECK_LAUNCH("valid_fss_fold");
  return ADNM_OK;
}

// ---- intensity-scale skill score: sums of squared event counts over dyadic blocks ----
// The frame sits at the origin of a P x P domain, P the smallest power of two >= max(H, W), zeros outside the frame (the padding FSS uses).
// Block (l, i, j) is the 2^l x 2^l pixels at (i 2^l, j 2^l); o and f are its target and forecast events.  Per frame index, level
// l = 0 .. L = log2 P and threshold the statistic is A_l = SUM o^2, F_l = SUM f^2, C_l = SUM o f over the blocks of the level
// (include/adnm_hip.h: adnm_valid_iscale_accum): the Haar components of the binary error follow from it on the host.
//   the tile   grid (tiles, frames), one 32 x 32 tile staged ONCE with no halo.  A lane owns one 2 x 2 cell, the lanes in Morton order over
//              the tile's 16 x 16 cells, so that the 4 lanes that differ in bits 0-1 are a 4 x 4 block, the 16 that differ in bits 0-3 an
//              8 x 8 block, a wave a 16 x 16 block.  Levels 0 and 1 are counts inside the lane; levels 2, 3 and 4 are two xor shuffles each
//              on the packed pair (o, f <= 256: 16 bits each); level 5 is the four waves through LDS.  The leaders' squares of two levels
//              share a dword (a wave's sum is <= 256, 1024, 4096, 16384 at levels 0 .. 3: no carry) and are added across the wave.
//   the fold   one workgroup per (frame index, threshold): the tile partials of levels 0 .. min(L, 5) added over samples and tiles, and
//              levels 6 .. L built per frame from the tiles' counts by a 4-to-1 pyramid in LDS, all in uint64; each (l, k) sum is added
//              to the table once.
// Integers throughout, no atomics, no workgroup waits for another, every loop bounded at launch.
namespace {
constexpr int kIsMaxSide = 1024;                  // P <= 1024: at most 32 x 32 tiles, L <= 10
constexpr int kIsTileLevels = 6, kIsLevels = 11;  // levels a tile serves (0 .. 5), levels in all (0 .. 10)
constexpr int kIsPitch = kTile + 4;               // uint16 per staged row: 72 bytes, a row start stays 8-byte aligned
constexpr int kIsPyramid = 1024 + 256 + 64 + 16 + 4 + 1;

// L of a frame: the smallest L with 2^L >= max(H, W)
inline int iscale_levels(int64_t H, int64_t W) {
  int L = 0;
  while ((int64_t(1) << L) < (H > W ? H : W)) ++L;
  return L;
}
// uint32 per (frame, tile): [level 0 .. nl - 1][3 * nthr] A, F, C of the tile's blocks, then [nthr][2] the tile's two counts
__host__ __device__ inline int64_t iscale_tile_words(int nl, int64_t nthr) { return (3 * nl + 2) * nthr; }

// the even bits of an 8-bit Morton code
__device__ __forceinline__ uint32_t iscale_even_bits(uint32_t v) {
  v &= 0x55u;
  v = (v | (v >> 1)) & 0x33u;
  return (v | (v >> 2)) & 0x0fu;
}
__device__ __forceinline__ uint64_t iscale_wave_sum64(uint64_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
    v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}

// grid (tiles, frames).  nl = min(L, 5) + 1: the levels written.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void iscale_tile_kernel(ScoredPair pair, uint32_t* __restrict__ part, int H, int W, int tiles_x, int nl,
                                                             float value_scale, Thr thr) {
  __shared__ __attribute__((aligned(8))) uint16_t img[kTile][kIsPitch];
  __shared__ uint32_t wred[kBlock / 64][kMaxThr][16];   // per wave and threshold: A, F, C of levels 0 .. 4, then the wave's counts (o | f << 16)
  const int f = blockIdx.y, tile = blockIdx.x, oy = (tile / tiles_x) * kTile, ox = (tile % tiles_x) * kTile;
  if (oy + kTile <= H && ox + kTile <= W)
    stage_pair_bits<VEC, kIsPitch, true>(&img[0][0], pair.target(f), pair.forecast(f), H, W, oy, ox, kTile, kTile, value_scale, thr);
  else
    stage_pair_bits<VEC, kIsPitch, false>(&img[0][0], pair.target(f), pair.forecast(f), H, W, oy, ox, kTile, kTile, value_scale, thr);
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cx = (int)iscale_even_bits(threadIdx.x), cy = (int)iscale_even_bits(threadIdx.x >> 1);   // the lane's cell of the 16 x 16
  const uint32_t r0 = *(const uint32_t*)&img[2 * cy][2 * cx], r1 = *(const uint32_t*)&img[2 * cy + 1][2 * cx];   // two pixels each
  const uint32_t b0 = r0 & (r0 >> 8), b1 = r1 & (r1 >> 8);   // bit k of a pixel: an event in both fields
  const bool lead2 = (lane & 3) == 0, lead3 = (lane & 15) == 0;
#pragma unroll
  for (int k = 0; k < kMaxThr; ++k)
    if (k < thr.n) {
      auto cell = [](uint32_t a, uint32_t b, int sh) {   // the cell's pixels with bit sh set: 0 .. 4
        const uint32_t s = ((a >> sh) & 0x00010001u) + ((b >> sh) & 0x00010001u);
        return (s & 0xffffu) + (s >> 16);
      };
      const uint32_t o1 = cell(r0, r1, k), f1 = cell(r0, r1, 8 + k), c0 = cell(b0, b1, k);
      uint32_t v = o1 | (f1 << 16);
      v += (uint32_t)__shfl_xor((int)v, 1, 64);
      v += (uint32_t)__shfl_xor((int)v, 2, 64);
      const uint32_t o2 = v & 0xffffu, f2 = v >> 16;   // <= 16
      v += (uint32_t)__shfl_xor((int)v, 4, 64);
      v += (uint32_t)__shfl_xor((int)v, 8, 64);
      const uint32_t o3 = v & 0xffffu, f3 = v >> 16;   // <= 64
      v += (uint32_t)__shfl_xor((int)v, 16, 64);
      v += (uint32_t)__shfl_xor((int)v, 32, 64);
      const uint32_t o4 = v & 0xffffu, f4 = v >> 16;   // <= 256, the same in every lane
      // levels 0 | 1 and levels 2 | 3 as 16-bit lanes; o^2 = o for a single pixel
      uint32_t a01 = o1 | ((o1 * o1) << 16), f01 = f1 | ((f1 * f1) << 16), c01 = c0 | ((o1 * f1) << 16);
      uint32_t a23 = (lead2 ? o2 * o2 : 0u) | ((lead3 ? o3 * o3 : 0u) << 16), f23 = (lead2 ? f2 * f2 : 0u) | ((lead3 ? f3 * f3 : 0u) << 16),
               c23 = (lead2 ? o2 * f2 : 0u) | ((lead3 ? o3 * f3 : 0u) << 16);
      a01 = fss_wave_sum(a01), f01 = fss_wave_sum(f01), c01 = fss_wave_sum(c01);
      a23 = fss_wave_sum(a23), f23 = fss_wave_sum(f23), c23 = fss_wave_sum(c23);
      if (lane == 0) {
        uint32_t* w = wred[wave][k];
        w[0] = a01 & 0xffffu, w[1] = f01 & 0xffffu, w[2] = c01 & 0xffffu;
        w[3] = a01 >> 16, w[4] = f01 >> 16, w[5] = c01 >> 16;
        w[6] = a23 & 0xffffu, w[7] = f23 & 0xffffu, w[8] = c23 & 0xffffu;
        w[9] = a23 >> 16, w[10] = f23 >> 16, w[11] = c23 >> 16;
        w[12] = o4 * o4, w[13] = f4 * f4, w[14] = o4 * f4;
        w[15] = v;
      }
    }
  __syncthreads();
  const int nout = 3 * thr.n;
  if ((int)threadIdx.x < nout) {
    const int k = threadIdx.x / 3, c = threadIdx.x % 3;
    uint32_t* out = part + ((int64_t)f * gridDim.x + tile) * iscale_tile_words(nl, thr.n);
    for (int l = 0; l < kIsTileLevels - 1; ++l)
      if (l < nl) out[l * nout + threadIdx.x] = (wred[0][k][3 * l + c] + wred[1][k][3 * l + c]) + (wred[2][k][3 * l + c] + wred[3][k][3 * l + c]);
    const uint32_t both = (wred[0][k][15] + wred[1][k][15]) + (wred[2][k][15] + wred[3][k][15]);   // <= 1024 in each half
    const uint32_t o5 = both & 0xffffu, f5 = both >> 16;
    if (nl == kIsTileLevels) out[5 * nout + threadIdx.x] = c == 0 ? o5 * o5 : c == 1 ? f5 * f5 : o5 * f5;
    if (c < 2) out[nl * nout + 2 * k + c] = c == 0 ? o5 : f5;
  }
}

// grid (T, nthr).  table[t][l][3k .. 3k+2] += A_l, F_l, C_l of the batch's frames with frame index t
__global__ __launch_bounds__(kFoldBlock) void iscale_fold_kernel(const uint32_t* __restrict__ part, int tiles_x, int tiles_y, int frames, int T, int nthr,
                                                                 int L, double* __restrict__ table) {
  __shared__ uint2 pyr[kIsPyramid];   // (o, f) of the blocks of levels 5, 6, ... of one frame, one level behind the other
  __shared__ uint64_t red[kFoldBlock / 64][3 * kIsLevels];
  const int t = blockIdx.x, k = blockIdx.y, B = frames / T, tiles = tiles_x * tiles_y;
  const int nl = min(L, kIsTileLevels - 1) + 1, nout = 3 * nthr;
  const int64_t words = iscale_tile_words(nl, nthr);
  uint64_t acc[kIsLevels][3];
#pragma unroll
  for (int l = 0; l < kIsLevels; ++l) acc[l][0] = acc[l][1] = acc[l][2] = 0;
  for (int i = threadIdx.x; i < B * tiles; i += kFoldBlock) {   // B * tiles <= 65535 * 1024
    const int b = i / tiles, tile = i % tiles;
    const uint32_t* q = part + (((int64_t)b * T + t) * tiles + tile) * words + 3 * k;
#pragma unroll
    for (int l = 0; l < kIsTileLevels; ++l)
      if (l < nl) acc[l][0] += q[l * nout], acc[l][1] += q[l * nout + 1], acc[l][2] += q[l * nout + 2];
  }
  if (L >= kIsTileLevels) {
    const int up = L - (kIsTileLevels - 1), PT = 1 << up;   // PT x PT tile places in the domain, tiles_y x tiles_x of them in the frame
    for (int b = 0; b < B; ++b) {
      const uint32_t* q = part + ((int64_t)b * T + t) * tiles * words + nl * nout + 2 * k;
      for (int i = threadIdx.x; i < PT * PT; i += kFoldBlock) {
        const int ty = i >> up, tx = i & (PT - 1);
        uint2 v = make_uint2(0u, 0u);
        if (ty < tiles_y && tx < tiles_x) {
          const uint32_t* c = q + (int64_t)(ty * tiles_x + tx) * words;
          v = make_uint2(c[0], c[1]);
        }
        pyr[i] = v;
      }
      __syncthreads();
      int src = 0, side = PT;
#pragma unroll
      for (int j = 1; j <= kIsLevels - kIsTileLevels; ++j)
        if (j <= up) {   // (the same for the whole workgroup)
          const int dst = src + side * side, half = side >> 1;
          for (int i = threadIdx.x; i < half * half; i += kFoldBlock) {
            const uint2* p = &pyr[src + 2 * (i / half) * side + 2 * (i % half)];
            const uint32_t o = (p[0].x + p[1].x) + (p[side].x + p[side + 1].x), fc = (p[0].y + p[1].y) + (p[side].y + p[side + 1].y);   // <= 2^20
            pyr[dst + i] = make_uint2(o, fc);
            acc[kIsTileLevels - 1 + j][0] += (uint64_t)o * o, acc[kIsTileLevels - 1 + j][1] += (uint64_t)fc * fc, acc[kIsTileLevels - 1 + j][2] += (uint64_t)o * fc;
          }
          __syncthreads();   // the level is there; and after the last one the next frame may rewrite level 5
          src = dst, side = half;
        }
    }
  }
#pragma unroll
  for (int l = 0; l < kIsLevels; ++l)
    if (l <= L) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const uint64_t s = iscale_wave_sum64(acc[l][c]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][3 * l + c] = s;
      }
    }
  __syncthreads();
  if ((int)threadIdx.x < 3 * (L + 1)) {
    const int l = threadIdx.x / 3, c = threadIdx.x % 3;
    const uint64_t s = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    table[((int64_t)t * (L + 1) + l) * nout + 3 * k + c] += (double)s;
  }
}

// the intensity-scale pass's own limits: nullptr, or the one that refuses
const char* iscale_why(int64_t frames, int64_t T, int64_t H, int64_t W, int64_t nthr) {
  if (nthr < 1 || nthr > kMaxThr) return "1..8 thresholds";
  if (const char* w = pair_frames_why(frames, T)) return w;
  if (H < 1 || W < 1 || H > kIsMaxSide || W > kIsMaxSide) return "H and W must be in [1, 1024]";
  return nullptr;
}
}  // namespace

extern "C" int64_t adnm_valid_iscale_block_bytes(int64_t T, int64_t nthr, int64_t H, int64_t W) {
  if (T < 1 || T > 65535 || iscale_why(1, 1, H, W, nthr)) return -1;
  return (int64_t)sizeof(double) * T * (iscale_levels(H, W) + 1) * 3 * nthr;
}

extern "C" int64_t adnm_valid_iscale_accum_ws_bytes(int64_t frames, int64_t T, int64_t H, int64_t W, int64_t nthr) {
  if (iscale_why(frames, T, H, W, nthr)) return -1;
  const int L = iscale_levels(H, W), nl = (L < kIsTileLevels - 1 ? L : kIsTileLevels - 1) + 1;
  return frames * tiles_of(H, W) * iscale_tile_words(nl, nthr) * (int64_t)sizeof(uint32_t);
}

extern "C" int adnm_valid_iscale_accum(const float* pred, int64_t pred_sample_stride, int64_t pred_frame_stride, const float* target, void* table,
                                       const float* thresholds_host, int64_t nthr, float value_scale, void* ws, int64_t ws_bytes, int64_t frames,
                                       int64_t T, int64_t H, int64_t W, adnm_stream_t stream) {
  const PairCall call = {"valid_iscale_accum", pred, pred_sample_stride, pred_frame_stride, target, table, ws, ws_bytes, H, W,
                         /*flat*/ false, /*ws_optional*/ false, /*ws_aligned*/ true, /*ws_rc*/ ADNM_EWORKSPACE};
  if (int rc = pair_check(call, thresholds_host != nullptr, iscale_why(frames, T, H, W, nthr), adnm_valid_iscale_accum_ws_bytes(frames, T, H, W, nthr),
                          "frames %lld T %lld %lld x %lld nthr %lld", (long long)frames, (long long)T, (long long)H, (long long)W, (long long)nthr))
    return rc;
  const Thr thr = thr_fill(thresholds_host, nthr);
  const bool vec = pair_quads(W, pred_sample_stride, pred_frame_stride, pred, target);
  const ScoredPair pair = {pred, pred_sample_stride, pred_frame_stride, target, (int)T, (int)(H * W)};
  const int tiles_x = (int)adnm_cdiv(W, kTile), tiles_y = (int)adnm_cdiv(H, kTile), tiles = tiles_x * tiles_y;
  const int L = iscale_levels(H, W), nl = (L < kIsTileLevels - 1 ? L : kIsTileLevels - 1) + 1;
  hipStream_t st = (hipStream_t)stream;
  {
    ADNM_PROF("valid_iscale", st, 8.0 * frames * H * W);
    const dim3 grid((unsigned)tiles, (unsigned)frames);
    if (vec) iscale_tile_kernel<true><<<grid, kBlock, 0, st>>>(pair, (uint32_t*)ws, (int)H, (int)W, tiles_x, nl, value_scale, thr);
    else iscale_tile_kernel<false><<<grid, kBlock, 0, st>>>(pair, (uint32_t*)ws, (int)H, (int)W, tiles_x, nl, value_scale, thr);
  }
  ADNM_CHECK_LAUNCH("valid_iscale_accum");
  {
    ADNM_PROF("valid_iscale_fold", st, 4.0 * frames * tiles * iscale_tile_words(nl, nthr));
    iscale_fold_kernel<<<dim3((unsigned)T, (unsigned)nthr), kFoldBlock, 0, st>>>((const uint32_t*)ws, tiles_x, tiles_y, (int)frames, (int)T, (int)nthr, L,
                                                                                (double*)table);
  }
  ADNM_CHECK_LAUNCH("valid_iscale_fold");
  return ADNM_OK;
}

// ---- neighbourhood exceedance probability: the histogram of (window count, observed bit), and the probability field ----
// p(y, x) = c_f(y, x) / n^2 with FSS's c_f above (zeros outside the frame, the denominator always n^2), read as the probability of the
// event at the pixel; o(y, x) is the target's event bit at the pixel itself.  The statistic (include/adnm_hip.h: adnm_valid_nprob_accum;
// DESIGN.md §4r) is N[t][k][scale][o][c]: how many pixels have the observed bit o and the window count c.  Brier score, its decomposition,
// the reliability diagram and the ROC curve are host arithmetic on it (validate.nprob_entries).
//   one launch    grid (tiles, frames), FSS's staging.  Only the FORECAST is counted in windows, so a scale and a nibble (four thresholds)
//                 need one plane of row counts, rs[staged row][centre column]: wave q takes the centre columns 8q .. 8q + 7, lane R the
//                 staged row R, running along the row as the FSS pass does.  The column pass is FSS's: a thread owns four consecutive
//                 centres of a column and keeps the four thresholds' counts in 16-bit lanes.
//   the histogram u32 in LDS, hist[threshold of the nibble][o][c], 4 * 2 * (n^2 + 1) <= 8720 bins (34.9 KB).  Thresholds are taken four at
//                 a time, so img + rs + hist is 51.8 KB of static LDS: below 64 KB, no function attribute, three workgroups per CU.  All
//                 eight at once would be 78 KB of histogram and one workgroup less per CU for a pass that the row and column sums bound.
//   the hot bin   radar fields are mostly empty, so nearly every lane holds (o = 0, c = 0): those lanes are counted with a ballot and a
//                 popcount into a per-wave scalar per threshold, added to LDS once per wave (joint.hip's trick); the others issue an atomic.
//   the flush     after a scale's nibble only the non-zero bins go to the table, as no-return double atomics, and are cleared.  Every
//                 addend is an integer and every sum stays below 2^53: exact and the same bits on every run whatever the order.
// No workgroup waits for another; every loop has a bound known at launch; no floating-point sum anywhere.
namespace {
constexpr int kNprobBins = 2 * (kFssWin * kFssWin + 1);   // of one threshold at the largest scale: 2180

// The row pass of one nibble of one plane of staged bits: lane `R` of wave `q` takes staged row R and the centre columns 8q .. 8q + 7.
// row: the staged row; sh: where the nibble stands in a pixel; c0: the staged column of centre 0's window.  rs[R][x] = the four
// thresholds' counts over the staged columns c0 + x .. c0 + x + n - 1, one per byte (<= 33: bytes never carry).
template <typename PX>
__device__ __forceinline__ void nprob_row_pass(uint32_t (*rs)[kTile + 1], const PX* row, int R, int q, int sh, int c0, int n) {
  const int x0 = 8 * q;
  uint32_t s = 0;
  for (int u = 0; u < n - 1; ++u) s += fss_spread((row[c0 + x0 + u] >> sh) & 0xfu);
  for (int x = x0; x < x0 + 8; ++x) {
    s += fss_spread((row[c0 + x + n - 1] >> sh) & 0xfu);   // c0 + x + n - 1 <= hs + n / 2 + 31 < side
    rs[R][x] = s;
    s -= fss_spread((row[c0 + x] >> sh) & 0xfu);           // it was added: no byte borrows
  }
}

// The column pass: acc[e] holds bytes e and e + 2 of the row counts of column cx summed over a window of staged rows, as 16-bit lanes
// (<= 1089 each).  Threshold kk of the nibble: nprob_count(acc, kk).
__device__ __forceinline__ void nprob_rows(uint32_t (&acc)[2], const uint32_t (*rs)[kTile + 1], int R, int cx, bool add) {
  const uint32_t v = rs[R][cx], e = v & 0x00ff00ffu, o = (v >> 8) & 0x00ff00ffu;
  acc[0] = add ? acc[0] + e : acc[0] - e;
  acc[1] = add ? acc[1] + o : acc[1] - o;
}
__device__ __forceinline__ uint32_t nprob_count(const uint32_t (&acc)[2], int kk) { return (acc[kk & 1] >> (16 * (kk >> 1))) & 0xffffu; }

// grid (tiles, frames).  hs: as for fss_sums_kernel.  off[p]: where scale p's two runs start in a (t, k) row of S doubles.
struct NprobOff {
  int at[kFssMax], S;
};
template <bool VEC>
__global__ __launch_bounds__(kBlock) void nprob_hist_kernel(ScoredPair pair, double* __restrict__ table, int H, int W, int tiles_x, int hs,
                                                            float value_scale, Thr thr, Scales scales, NprobOff off, int clear) {
  __shared__ __attribute__((aligned(4))) uint16_t img[kFssSide][kFssPitch];
  __shared__ uint32_t rs[kFssSide][kTile + 1];
  __shared__ uint32_t hist[4 * kNprobBins];
  const int f = blockIdx.y, tile = blockIdx.x, oy = (tile / tiles_x) * kTile, ox = (tile % tiles_x) * kTile;
  const int side = kTile + 2 * hs;
  stage_pair_bits<VEC, kFssPitch, false>(&img[0][0], pair.target(f), pair.forecast(f), H, W, oy - hs, ox - hs, side, side, value_scale, thr);
  for (int i = threadIdx.x; i < clear; i += kBlock) hist[i] = 0u;   // clear = 4 * 2 * (max n^2 + 1): the bins any scale of this call uses
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cx = threadIdx.x & 31, cy0 = (threadIdx.x >> 5) * 4;   // the column pass: centres (cy0 .. cy0 + 3, cx) of the tile
  const bool col_in = ox + cx < W;
  double* row_t = table + (int64_t)(f % pair.T) * thr.n * off.S;
  for (int p = 0; p < scales.cnt; ++p) {
    const int n = scales.n[p], c0 = hs - (n >> 1), per = n * n + 1;   // a threshold's bins: [o = 0: c = 0 .. n^2][o = 1: c = 0 .. n^2]
    for (int h = 0; 4 * h < thr.n; ++h) {                            // the nibble: thresholds 4h .. 4h + 3
      const int nk = min(4, thr.n - 4 * h);
      if (lane < side) nprob_row_pass(rs, img[lane], lane, wave, 8 + 4 * h, c0, n);
      __syncthreads();
      uint32_t acc[2] = {0, 0}, zeros[4] = {0, 0, 0, 0};   // zeros: wave-uniform, the lanes of this wave in bin (o = 0, c = 0) per threshold
      for (int u = 0; u < n - 1; ++u) nprob_rows(acc, rs, c0 + cy0 + u, cx, true);
      for (int j = 0; j < 4; ++j) {                        // the same trips for every lane: the ballots below see whole waves
        nprob_rows(acc, rs, c0 + cy0 + j + n - 1, cx, true);   // <= 2 * hs + 31 < side
        const bool valid = col_in && oy + cy0 + j < H;
        const uint32_t obs = img[hs + cy0 + j][hs + cx] >> (4 * h);   // the centre's target bits of this nibble
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
          if (kk < nk) {
            const int bin = (int)((obs >> kk) & 1u) * per + (int)nprob_count(acc, kk);
            zeros[kk] += (uint32_t)__popcll(__ballot(valid && bin == 0));
            if (valid && bin != 0) atomicAdd(&hist[kk * 2 * per + bin], 1u);
          }
        nprob_rows(acc, rs, c0 + cy0 + j, cx, false);
      }
      if (lane == 0) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
          if (kk < nk && zeros[kk]) atomicAdd(&hist[kk * 2 * per], zeros[kk]);
      }
      __syncthreads();
      for (int i = threadIdx.x; i < nk * 2 * per; i += kBlock) {
        const uint32_t v = hist[i];
        if (v) {
          const int kk = i / (2 * per), bin = i % (2 * per);
          unsafeAtomicAdd(&row_t[(int64_t)(4 * h + kk) * off.S + off.at[p] + bin], (double)v);   // integers below 2^53: exact in any order
          hist[i] = 0u;
        }
      }
      __syncthreads();   // rs and hist are rewritten by the next nibble or scale
    }
  }
}

// the histogram pass's own limits: nullptr, or the one that refuses.  The scales are FSS's, so that one staging serves both.
const char* nprob_why(int64_t frames, int64_t T, int64_t H, int64_t W, int64_t nthr, const int64_t* scales_host, int64_t nscale) {
  if (!scales_host) return "null pointer";
  if (nscale < 1 || nscale > kFssMax) return "1..4 scales";
  if (nthr < 1 || nthr > kMaxThr) return "1..8 thresholds";
  if (const char* w = pair_frames_why(frames, T)) return w;
  if (const char* w = pair_tiled_shape_why(H, W)) return w;
  for (int64_t p = 0; p < nscale; ++p) {
    const int64_t n = scales_host[p];
    if (n < 1 || n > kFssWin || n % 2 == 0) return "a scale must be odd and in 1..33";
    for (int64_t o = 0; o < p; ++o)
      if (scales_host[o] == n) return "a scale is given twice";
  }
  return nullptr;
}
// S of a (t, k) row: the doubles of all scales; the scales have passed nprob_why
inline int64_t nprob_row(const int64_t* scales_host, int64_t nscale) {
  int64_t s = 0;
  for (int64_t p = 0; p < nscale; ++p) s += 2 * (scales_host[p] * scales_host[p] + 1);
  return s;
}
}  // namespace

extern "C" int64_t adnm_valid_nprob_block_bytes(int64_t T, int64_t nthr, const int64_t* scales_host, int64_t nscale) {
  if (T < 1 || T > 65535 || nprob_why(1, 1, 1, 1, nthr, scales_host, nscale)) return -1;
  return (int64_t)sizeof(double) * T * nthr * nprob_row(scales_host, nscale);
}

extern "C" int64_t adnm_valid_nprob_accum_ws_bytes(int64_t frames, int64_t T, int64_t H, int64_t W, int64_t nthr, const int64_t* scales_host, int64_t nscale) {
  return nprob_why(frames, T, H, W, nthr, scales_host, nscale) ? -1 : 0;   // the partial histograms live in LDS
}

extern "C" int adnm_valid_nprob_accum(const float* pred, int64_t pred_sample_stride, int64_t pred_frame_stride, const float* target, void* table,
                                      const float* thresholds_host, int64_t nthr, float value_scale, const int64_t* scales_host, int64_t nscale, void* ws,
                                      int64_t ws_bytes, int64_t frames, int64_t T, int64_t H, int64_t W, adnm_stream_t stream) {
  const PairCall call = {"valid_nprob_accum", pred, pred_sample_stride, pred_frame_stride, target, table, ws, ws_bytes, H, W,
                         /*flat*/ false, /*ws_optional*/ true, /*ws_aligned*/ false, /*ws_rc*/ ADNM_EINVAL};
  if (int rc = pair_check(call, thresholds_host && scales_host, nprob_why(frames, T, H, W, nthr, scales_host, nscale),
                          adnm_valid_nprob_accum_ws_bytes(frames, T, H, W, nthr, scales_host, nscale),
                          "frames %lld T %lld %lld x %lld nthr %lld nscale %lld", (long long)frames, (long long)T, (long long)H, (long long)W,
                          (long long)nthr, (long long)nscale))
    return rc;
  const Thr thr = thr_fill(thresholds_host, nthr);
  Scales scales;
  NprobOff off;
  scales.cnt = (int)nscale;
  off.S = (int)nprob_row(scales_host, nscale);   // <= 4 * 2180
  int hs = 0, at = 0, clear = 0;
  for (int p = 0; p < kFssMax; ++p) {
    scales.n[p] = p < nscale ? (int)scales_host[p] : 1;
    off.at[p] = at;
    if (p < nscale) at += 2 * (scales.n[p] * scales.n[p] + 1);
    hs = scales.n[p] / 2 > hs ? scales.n[p] / 2 : hs;
    clear = 4 * 2 * (scales.n[p] * scales.n[p] + 1) > clear ? 4 * 2 * (scales.n[p] * scales.n[p] + 1) : clear;   // <= 4 * kNprobBins
  }
  const bool vec = pair_quads(W, pred_sample_stride, pred_frame_stride, pred, target);
  if (vec) hs = (int)adnm_align(hs, 4);   // <= 16
  const ScoredPair pair = {pred, pred_sample_stride, pred_frame_stride, target, (int)T, (int)(H * W)};
  const int tiles_x = (int)adnm_cdiv(W, kTile), tiles = (int)tiles_of(H, W);
  hipStream_t st = (hipStream_t)stream;
  {
    ADNM_PROF("valid_nprob", st, 8.0 * frames * H * W);
    const dim3 grid((unsigned)tiles, (unsigned)frames);
    if (vec) nprob_hist_kernel<true><<<grid, kBlock, 0, st>>>(pair, (double*)table, (int)H, (int)W, tiles_x, hs, value_scale, thr, scales, off, clear);
    else nprob_hist_kernel<false><<<grid, kBlock, 0, st>>>(pair, (double*)table, (int)H, (int)W, tiles_x, hs, value_scale, thr, scales, off, clear);
  }
  ADNM_CHECK_LAUNCH("valid_nprob_accum");
  return ADNM_OK;
}

// ---- the probability field of ONE field at ONE scale: out[k][f][y][x] = float(c_f) / float(n^2) ----
// The same tiles, halo and running sums on a one-byte image (bit k = q >= thr_k).  The counts of a nibble pass through LDS once more so
// that a thread leaves with four consecutive columns of a row: one 16-byte store where the output allows it.  The quotient is one IEEE
// division of two exactly represented integers (no reciprocal): the same bits as np.float32(c) / np.float32(n * n).
namespace {
constexpr int kProbPitch = kFssSide + 4;   // bytes per staged row: 17 dwords, so that the lanes of the row pass (one row each) hit distinct banks

// the event bits of one field's rectangle -> img[r * kProbPitch + c], 0 outside the frame.  VEC: W, x0 and cols are multiples of 4 and
// every row starts on 16 bytes.
template <bool VEC>
__device__ __forceinline__ void stage_field_bits(uint8_t* img, const float* __restrict__ src, int H, int W, int y0, int x0, int rows, int cols,
                                                 float value_scale, const Thr& thr) {
  auto bits = [&](float v) {
    const float q = eval_trunc(eval_scaled(v, value_scale));
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < kMaxThr; ++k)
      if (k < thr.n) m |= q >= thr.t[k] ? 1u << k : 0u;
    return m;
  };
  if (VEC) {
    const int q = cols >> 2;
    for (int i = threadIdx.x; i < rows * q; i += kBlock) {
      const int r = i / q, c = (i % q) * 4, gy = y0 + r, gx = x0 + c;
      uint32_t m = 0;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        const float4 a = *(const float4*)(src + (int64_t)gy * W + gx);
        m = bits(a.x) | (bits(a.y) << 8) | (bits(a.z) << 16) | (bits(a.w) << 24);
      }
      *(uint32_t*)&img[r * kProbPitch + c] = m;   // c and kProbPitch are multiples of 4
    }
  } else {
    for (int i = threadIdx.x; i < rows * cols; i += kBlock) {
      const int r = i / cols, c = i % cols, gy = y0 + r, gx = x0 + c;
      img[r * kProbPitch + c] = (uint8_t)((gy >= 0 && gy < H && gx >= 0 && gx < W) ? bits(src[(int64_t)gy * W + gx]) : 0u);
    }
  }
}

// grid (tiles, frames).  VIN: 16-byte loads (W % 4 == 0, src on 16 bytes); VOUT: 16-byte stores (W % 4 == 0, out on 16 bytes).
template <bool VIN, bool VOUT>
__global__ __launch_bounds__(kBlock) void nprob_field_kernel(const float* __restrict__ src, float* __restrict__ out, int frames, int H, int W, int tiles_x,
                                                             int hs, float value_scale, Thr thr, int n) {
  __shared__ __attribute__((aligned(4))) uint8_t img[kFssSide][kProbPitch];
  __shared__ uint32_t rs[kFssSide][kTile + 1];
  __shared__ __attribute__((aligned(8))) uint16_t cnt[4][kTile][kTile + 4];   // [threshold of the nibble][centre row][centre column]
  const int f = blockIdx.y, tile = blockIdx.x, oy = (tile / tiles_x) * kTile, ox = (tile % tiles_x) * kTile;
  const int side = kTile + 2 * hs, c0 = hs - (n >> 1);
  const int64_t hw = (int64_t)H * W;
  stage_field_bits<VIN>(&img[0][0], src + f * hw, H, W, oy - hs, ox - hs, side, side, value_scale, thr);
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cx = threadIdx.x & 31, cy0 = (threadIdx.x >> 5) * 4;   // the column pass: centres (cy0 .. cy0 + 3, cx)
  const int qy = threadIdx.x >> 3, qx = (threadIdx.x & 7) * 4;     // the store: centres (qy, qx .. qx + 3)
  const float nn = (float)(n * n);
  for (int h = 0; 4 * h < thr.n; ++h) {
    const int nk = min(4, thr.n - 4 * h);
    if (lane < side) nprob_row_pass(rs, img[lane], lane, wave, 4 * h, c0, n);
    __syncthreads();
    uint32_t acc[2] = {0, 0};
    for (int u = 0; u < n - 1; ++u) nprob_rows(acc, rs, c0 + cy0 + u, cx, true);
    for (int j = 0; j < 4; ++j) {
      nprob_rows(acc, rs, c0 + cy0 + j + n - 1, cx, true);   // <= 2 * hs + 31 < side
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) cnt[kk][cy0 + j][cx] = (uint16_t)nprob_count(acc, kk);
      nprob_rows(acc, rs, c0 + cy0 + j, cx, false);
    }
    __syncthreads();
    const int gy = oy + qy, gx = ox + qx;
    if (gy < H && gx < W) {
      for (int kk = 0; kk < nk; ++kk) {
        const uint16_t* c = &cnt[kk][qy][qx];
        float* dst = out + (((int64_t)(4 * h + kk) * frames + f) * H + gy) * W + gx;
        const float4 v = make_float4((float)c[0] / nn, (float)c[1] / nn, (float)c[2] / nn, (float)c[3] / nn);
        if (VOUT) {
          *(float4*)dst = v;   // W % 4 == 0: the four columns are inside
        } else {
          dst[0] = v.x;
          if (gx + 1 < W) dst[1] = v.y;
          if (gx + 2 < W) dst[2] = v.z;
          if (gx + 3 < W) dst[3] = v.w;
        }
      }
    }
    __syncthreads();   // rs and cnt are rewritten by the next nibble
  }
}
}  // namespace

extern "C" int adnm_neighbour_prob(const float* field, float* out, const float* thresholds_host, int64_t nthr, float value_scale, int64_t scale,
                                   int64_t frames, int64_t H, int64_t W, adnm_stream_t stream) {
  ADNM_REQUIRE(field && out && thresholds_host, "neighbour_prob: null pointer");
  ADNM_REQUIRE(((uintptr_t)field | (uintptr_t)out) % 4 == 0, "neighbour_prob: field and out must be 4-byte aligned");
  ADNM_REQUIRE(nthr >= 1 && nthr <= kMaxThr, "neighbour_prob: 1..8 thresholds, got %lld", (long long)nthr);
  ADNM_REQUIRE(scale >= 1 && scale <= kFssWin && scale % 2 == 1, "neighbour_prob: the scale must be odd and in 1..33, got %lld", (long long)scale);
  ADNM_REQUIRE(frames >= 1 && frames <= 65535, "neighbour_prob: 1 <= frames <= 65535, got %lld", (long long)frames);
  if (const char* w = pair_tiled_shape_why(H, W)) ADNM_REQUIRE(false, "neighbour_prob: %s (got %lld x %lld)", w, (long long)H, (long long)W);
  const Thr thr = thr_fill(thresholds_host, nthr);
  const bool vin = W % 4 == 0 && (uintptr_t)field % 16 == 0, vout = W % 4 == 0 && (uintptr_t)out % 16 == 0;
  int hs = (int)scale / 2;
  if (vin) hs = (int)adnm_align(hs, 4);   // <= 16
  const int tiles_x = (int)adnm_cdiv(W, kTile);
  const dim3 grid((unsigned)tiles_of(H, W), (unsigned)frames);
  hipStream_t st = (hipStream_t)stream;
  {
    ADNM_PROF("neighbour_prob", st, 4.0 * frames * H * W * (1 + nthr));
#define ADNM_NPROB_FIELD(VIN, VOUT) \
  nprob_field_kernel<VIN, VOUT><<<grid, kBlock, 0, st>>>(field, out, (int)frames, (int)H, (int)W, tiles_x, hs, value_scale, thr, (int)scale)
    if (vin && vout) ADNM_NPROB_FIELD(true, true);
    else if (vin) ADNM_NPROB_FIELD(true, false);
    else if (vout) ADNM_NPROB_FIELD(false, true);
    else ADNM_NPROB_FIELD(false, false);
#undef ADNM_NPROB_FIELD
  }
  ADNM_CHECK_LAUNCH("neighbour_prob");
  return ADNM_OK;
}
