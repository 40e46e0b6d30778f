// Space-time rain-cell tracks: connected-component labelling of the (t, y, x) event volume of every sample, threshold and field, and the track
// scores that follow from it (include/adnm_hip.h: adnm_valid_tracks_accum, adnm_label_tracks).  An event is q(v) >= thr with
// q = eval_trunc(eval_scaled(v, value_scale)) of adnm_common.h; a track is a 26-connected component of ONE sample's volume of ONE field; its label is
// 1 + the flat index t * H * W + y * W + x of its first voxel inside the sample.
//
//   a chain         one (sample, threshold, field).  Its slice of the workspace holds, per voxel, a parent word, a record word and a last-frame
//                   word, and per frame a bit plane padded to whole ballots of 64 pixels (so no frame's bits straddle a word of another frame).
//   four launches   no workgroup ever waits for another one: every barrier is a workgroup barrier, the order comes from the stream.
//     label         a workgroup of 1024 lanes per (frame, threshold) labels the frame's 8-connected objects of both fields with csrc/labelling.h,
//                   exactly as objects.hip does (words in LDS where the frame fits beside the bits, in the chain's own parent words otherwise),
//                   and writes per voxel: the parent as an index into the sample's volume (an object's first pixel is its own parent), the
//                   record (area | kMatched at an object's first pixel, 0 everywhere else) and the frame index.  EVERY word of the slice is
//                   written here, so what the workspace held does not matter.
//     merge         a workgroup per (frame boundary t-1 | t, threshold, field): an event voxel of frame t unites with the voxel below it in
//                   frame t-1 where that is an event (every other event of the 3 x 3 window is 8-adjacent to that one, so frame t-1's own
//                   labelling has united them), and otherwise with the first voxel of every arc of events on the ring of eight around it
//                   (neighbours on the ring are 8-adjacent).  The same lock-free unite on the global words; parents only decrease, so unions of
//                   different workgroups are safe.  BOUND: after a lost race max(a, b) is strictly smaller than before (the displaced value
//                   is below a, and b was below a), so a union ends within T * H * W rounds — the bound unite is given can never run out, and
//                   no union is dropped.
//     record        a workgroup per (frame, threshold, field): every object's first pixel (record != 0) finds its track's root and, where that
//                   is another voxel, adds its area, ors its matched flag and maxes its frame into the root's words.  A root is the smallest
//                   voxel of its track, hence the first pixel of its own object: its record starts as that object's.
//     reduce        a workgroup per (frame, threshold, field): the roots of that frame (parent == self, record != 0) with at least min_volume voxels
//                   add their columns to u64 counters in LDS, 4096 columns at a time; the non-zero ones go to the table as double atomics.
//                   adnm_label_tracks runs a labelling launch instead: every event voxel finds its root and writes root + 1 or 0.
//   exact           every addend is an integer and every sum stays below 2^53 while SUM v^2 does (one all-event volume of 2^22 voxels adds
//                   2^44; at 20 x 128^2 a sample adds at most 2^36.7, more than 80 000 samples), so the table is the same bits on every run
//                   although the order of the atomics is not fixed.
#include "labelling.h"

namespace {
constexpr int64_t kMaxPixels = 65536;          // as the object scores: an area fits kAreaMask
constexpr int64_t kMaxVoxels = 1ll << 22;      // a volume fits kVolMask, an index fits a word with room to spare
constexpr unsigned kVolMask = (1u << 23) - 1u;
constexpr int64_t kWsCap = 256ll << 20;        // thresholds are taken in chunks whose chains fit this (one threshold's chains always pass)
constexpr size_t kLdsLimit = 160 * 1024;
constexpr size_t kHead = 16;                   // the sweep flag
constexpr int kColChunk = 4096;                // u64 counters of a reduce pass

__host__ __device__ __forceinline__ int track_cols(int T) { return 7 + 4 * T; }

// one field of a call: frame t of sample b starts at pair_frame(p, ss, fs, b, t)
struct Src {
  const float* p;
  int64_t ss, fs;
};
// the workspace of one chunk of `kc` thresholds: chain c = (b * kc + kk) * nf + field
struct Ws {
  unsigned *word, *rec, *last, *bits;
  int kc, nf, T, hw, bw;   // bw = bit_words(hw)
  __device__ __forceinline__ int64_t chain(int b, int kk, int field) const { return ((int64_t)b * kc + kk) * nf + field; }
  __device__ __forceinline__ int64_t voxels(int64_t c) const { return c * T * hw; }
  __device__ __forceinline__ unsigned* plane(int64_t c, int t) const { return bits + (c * T + t) * bw; }
};

inline size_t label_lds(int64_t hw, bool words) { return kHead + 2 * sizeof(unsigned) * (size_t)bit_words((int)hw) + (words ? sizeof(unsigned) * (size_t)hw : 0); }
inline bool words_in_lds(int64_t hw) { return label_lds(hw, true) <= kLdsLimit; }

// grid (G): item = f * kc + kk labels frame f of threshold k0 + kk, the target (field 0) and with nf = 2 the forecast (field 1)
template <bool LDSW>
__global__ __launch_bounds__(kBlock) void tracks_label_kernel(Src s0, Src s1, Ws ws, Thr thr, int k0, float value_scale, int items, int W) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int hw = ws.hw, T = ws.T, tid = threadIdx.x;
  unsigned* flag = (unsigned*)smem;
  unsigned* bits0 = (unsigned*)(smem + kHead);
  unsigned* bits1 = bits0 + ws.bw;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int f = item / ws.kc, kk = item % ws.kc, b = f / T, t = f % T;
    __syncthreads();   // the item before is done with the bits
    stage_bits(bits0, pair_frame(s0.p, s0.ss, s0.fs, b, t), hw, thr.t[k0 + kk], value_scale);
    if (ws.nf == 2) stage_bits(bits1, pair_frame(s1.p, s1.ss, s1.fs, b, t), hw, thr.t[k0 + kk], value_scale);
    __syncthreads();
    for (int field = 0; field < ws.nf; ++field) {
      const unsigned* bits = field ? bits1 : bits0;
      const int64_t c = ws.chain(b, kk, field), at = ws.voxels(c) + (int64_t)t * hw;
      unsigned* plane = ws.plane(c, t);
      for (int w = tid; w < ws.bw; w += kBlock) plane[w] = bits[w];
      unsigned* word = LDSW ? bits0 + 2 * ws.bw : ws.word + at;
      label_field(word, bits, ws.nf == 2 ? (field ? bits0 : bits1) : nullptr, flag, hw, W);
      const unsigned base = (unsigned)t * (unsigned)hw;
      for (int p = tid; p < hw; p += kBlock) {
        const unsigned wd = ld(word + p);
        const bool ev = bit(bits, p), root = ev && (wd & kRoot);
        st(ws.word + at + p, base + (ev && !root ? wd : (unsigned)p));
        st(ws.rec + at + p, root ? (wd & kAreaMask) | (wd & kMatched) : 0u);
        st(ws.last + at + p, (unsigned)t);
      }
      __syncthreads();   // the words are read before the next field labels into them
    }
  }
}

// grid (G): item = ((b * (T - 1) + t - 1) * kc + kk) * nf + field unites frame t of a chain with frame t - 1
__global__ __launch_bounds__(kBlock) void tracks_merge_kernel(Ws ws, int items, int H, int W) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int hw = ws.hw, T = ws.T, tid = threadIdx.x, n = T * hw;
  unsigned* below = (unsigned*)smem;
  unsigned* here = below + ws.bw;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int field = item % ws.nf, kk = item / ws.nf % ws.kc, bt = item / ws.nf / ws.kc, b = bt / (T - 1), t = bt % (T - 1) + 1;
    const int64_t c = ws.chain(b, kk, field);
    __syncthreads();
    for (int w = tid; w < ws.bw; w += kBlock) below[w] = ws.plane(c, t - 1)[w], here[w] = ws.plane(c, t)[w];
    __syncthreads();
    unsigned* word = ws.word + ws.voxels(c);
    const unsigned at = (unsigned)t * (unsigned)hw, under = at - (unsigned)hw;
    for (int p = tid; p < hw; p += kBlock) {
      if (!bit(here, p)) continue;
      const int x = p % W, y = p / W;
      const bool l = x > 0, r = x + 1 < W, u = y > 0, d = y + 1 < H;
      // a union starts from the two voxels' parents (their objects' first pixels unless a find has moved them on): the find then shortens
      // the path of a word that every voxel of the object starts from, not of the voxel's own
      if (bit(below, p)) {
        if (!(l && bit(here, p - 1) && bit(below, p - 1))) unite(word, ld(word + at + p), ld(word + under + p), n);   // else the left neighbour makes this union
        continue;
      }
      // the ring around p in frame t - 1, clockwise from NW: consecutive ones are 8-adjacent, so the first of every arc speaks for the arc
      const int q[8] = {p - W - 1, p - W, p - W + 1, p + 1, p + W + 1, p + W, p + W - 1, p - 1};
      const bool in[8] = {u && l, u, u && r, r, d && r, d, d && l, l};
      bool before = false;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const bool ev = in[i] && bit(below, q[i]);
        if (ev && !before) unite(word, ld(word + at + p), ld(word + under + q[i]), n);
        before = ev;
      }
    }
  }
}

// grid (G): item = (f * kc + kk) * nf + field
__global__ __launch_bounds__(kBlock) void tracks_record_kernel(Ws ws, int items) {
  const int hw = ws.hw, T = ws.T, n = T * hw;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int field = item % ws.nf, kk = item / ws.nf % ws.kc, f = item / ws.nf / ws.kc, b = f / T, t = f % T;
    const int64_t v0 = ws.voxels(ws.chain(b, kk, field));
    unsigned *word = ws.word + v0, *rec = ws.rec + v0, *last = ws.last + v0;
    const unsigned at = (unsigned)t * (unsigned)hw;
    for (int p = threadIdx.x; p < hw; p += kBlock) {
      const unsigned own = ld(rec + at + p);   // != 0: the first pixel of an object; nobody adds to it unless it is its track's root
      if (own == 0u) continue;
      const unsigned root = find_root(word, at + p, n);
      if (root == at + p) continue;
      atomicAdd(rec + root, own & kVolMask);
      if (own & kMatched) atomicOr(rec + root, kMatched);
      atomicMax(last + root, (unsigned)t);
    }
  }
}

// grid (G): item = (f * kc + kk) * nf + field; table (2, nthr, C), field 0 = target
__global__ __launch_bounds__(kBlock) void tracks_reduce_kernel(Ws ws, double* __restrict__ table, int k0, int nthr, unsigned min_volume, int items) {
  __shared__ unsigned long long acc[kColChunk];
  const int hw = ws.hw, T = ws.T, tid = threadIdx.x, C = track_cols(T);
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int field = item % ws.nf, kk = item / ws.nf % ws.kc, f = item / ws.nf / ws.kc, b = f / T, t = f % T;
    const int64_t v0 = ws.voxels(ws.chain(b, kk, field));
    const unsigned *word = ws.word + v0, *rec = ws.rec + v0, *last = ws.last + v0;
    const unsigned at = (unsigned)t * (unsigned)hw;
    double* row = table + ((int64_t)field * nthr + k0 + kk) * C;
    for (int c0 = 0; c0 < C; c0 += kColChunk) {
      const int c1 = c0 + kColChunk < C ? c0 + kColChunk : C;
      __syncthreads();   // the pass before has read its counters
      for (int c = tid; c < c1 - c0; c += kBlock) acc[c] = 0ull;
      __syncthreads();
      auto add = [&](int col, unsigned long long val) {
        if (col >= c0 && col < c1) atomicAdd(&acc[col - c0], val);
      };
      for (int p = tid; p < hw; p += kBlock) {
        const unsigned r = ld(rec + at + p), v = r & kVolMask;
        if (r == 0u || ld(word + at + p) != at + p || v < min_volume) continue;
        const int t1 = (int)ld(last + at + p), d = t1 - t + 1;   // t is t0: a root is its track's first voxel
        add(0, 1ull), add(1, v), add(2, (unsigned long long)v * v), add(3, (unsigned long long)d);
        if (r & kMatched) add(4, 1ull), add(5, v);
        if (t == 0 && t1 == T - 1) add(6, 1ull);
        add(7 + t, 1ull), add(7 + T + t1, 1ull), add(7 + 3 * T + d - 1, 1ull);
        if (t == 0) add(7 + 2 * T + t1, 1ull);
      }
      __syncthreads();
      for (int c = tid; c < c1 - c0; c += kBlock)
        if (acc[c]) unsafeAtomicAdd(&row[c0 + c], (double)acc[c]);
    }
  }
}

// grid (G): item = f; one field, one threshold (kc = nf = 1): every element of labels (frames, H, W) is written
__global__ __launch_bounds__(kBlock) void tracks_write_kernel(Ws ws, int* __restrict__ labels, unsigned min_volume, int items) {
  const int hw = ws.hw, T = ws.T, n = T * hw;
  for (int f = blockIdx.x; f < items; f += gridDim.x) {
    const int b = f / T, t = f % T;
    const int64_t c = ws.chain(b, 0, 0), v0 = ws.voxels(c);
    const unsigned* plane = ws.plane(c, t);
    const unsigned at = (unsigned)t * (unsigned)hw;
    int* out = labels + (int64_t)f * hw;
    for (int p = threadIdx.x; p < hw; p += kBlock) {
      int lab = 0;
      if (bit(plane, p)) {
        const unsigned root = find_root(ws.word + v0, at + p, n);
        if ((ld(ws.rec + v0 + root) & kVolMask) >= min_volume) lab = (int)root + 1;
      }
      out[p] = lab;
    }
  }
}

const char* volume_why(int64_t T, int64_t H, int64_t W) {
  if (H < 1 || W < 1 || H > kMaxPixels || W > kMaxPixels || H * W > kMaxPixels) return "1 <= H * W <= 65536";
  if (T * H * W > kMaxVoxels) return "T * H * W <= 4194304";
  return nullptr;
}
// the track scores' own limits: nullptr, or the one that refuses
const char* tracks_why(int64_t frames, int64_t T, int64_t H, int64_t W, int64_t nthr, int64_t min_volume) {
  if (nthr < 1 || nthr > kMaxThr) return "1..8 thresholds";
  if (min_volume < 1) return "min_volume >= 1";
  if (const char* w = pair_frames_why(frames, T)) return w;
  return volume_why(T, H, W);
}
// bytes of the chains of one threshold: three words per voxel and the padded bit planes
inline int64_t thr_bytes(int64_t frames, int64_t hw, int64_t nf) { return nf * frames * (int64_t)sizeof(unsigned) * (3 * hw + bit_words((int)hw)); }
// thresholds per chunk: as many as fit kWsCap, at least one
inline int64_t chunk_of(int64_t frames, int64_t hw, int64_t nthr) {
  const int64_t fit = kWsCap / thr_bytes(frames, hw, 2);
  return fit < 1 ? 1 : fit < nthr ? fit : nthr;
}
inline Ws carve(void* ws, int64_t frames, int64_t T, int64_t hw, int64_t kc, int64_t nf) {
  const int64_t voxels = nf * kc * frames * hw;
  Ws w;
  w.word = (unsigned*)ws, w.rec = w.word + voxels, w.last = w.rec + voxels, w.bits = w.last + voxels;
  w.kc = (int)kc, w.nf = (int)nf, w.T = (int)T, w.hw = (int)hw, w.bw = bit_words((int)hw);
  return w;
}
inline unsigned grid_of(int64_t items) { return (unsigned)(items < 65536 ? items : 65536); }

// label, merge and record of one chunk; s1 is read only with nf = 2
int link_chunk(const char* name, const Src& s0, const Src& s1, const Ws& w, const Thr& thr, int k0, float value_scale, int64_t frames, int64_t H, int64_t W,
               hipStream_t st) {
  const int64_t hw = H * W, T = w.T;
  const bool in_lds = words_in_lds(hw);
  const size_t lds = label_lds(hw, in_lds);
  const int64_t items = frames * w.kc;
  {
    ADNM_PROF("tracks_label", st, 4.0 * w.nf * items * hw * 4);
    if (in_lds) {
      ADNM_ALLOW_LDS(tracks_label_kernel<true>, lds, name);
      tracks_label_kernel<true><<<grid_of(items), kBlock, lds, st>>>(s0, s1, w, thr, k0, value_scale, (int)items, (int)W);
    } else {
      tracks_label_kernel<false><<<grid_of(items), kBlock, lds, st>>>(s0, s1, w, thr, k0, value_scale, (int)items, (int)W);
    }
  }
  ADNM_CHECK_LAUNCH(name);
  if (T > 1) {
    const int64_t seams = frames / T * (T - 1) * w.kc * w.nf;
    ADNM_PROF("tracks_merge", st, 4.0 * seams * hw);
    tracks_merge_kernel<<<grid_of(seams), kBlock, 2 * sizeof(unsigned) * (size_t)w.bw, st>>>(w, (int)seams, (int)H, (int)W);
    ADNM_CHECK_LAUNCH(name);
  }
  {
    ADNM_PROF("tracks_record", st, 4.0 * items * w.nf * hw);
    tracks_record_kernel<<<grid_of(items * w.nf), kBlock, 0, st>>>(w, (int)(items * w.nf));
  }
  ADNM_CHECK_LAUNCH(name);
  return ADNM_OK;
}
inline unsigned small_of(int64_t min_volume) { return (unsigned)(min_volume > kMaxVoxels + 1 ? kMaxVoxels + 1 : min_volume); }   // no track is larger than a volume
}  // namespace

extern "C" int64_t adnm_valid_tracks_block_bytes(int64_t T, int64_t nthr) {
  if (T < 1 || T > 65535 || nthr < 1 || nthr > kMaxThr) return -1;
  return (int64_t)sizeof(double) * 2 * nthr * track_cols((int)T);
}

extern "C" int64_t adnm_valid_tracks_accum_ws_bytes(int64_t frames, int64_t T, int64_t H, int64_t W, int64_t nthr) {
  if (tracks_why(frames, T, H, W, nthr, 1)) return -1;
  return chunk_of(frames, H * W, nthr) * thr_bytes(frames, H * W, 2);
}

extern "C" int64_t adnm_label_tracks_ws_bytes(int64_t frames, int64_t T, int64_t H, int64_t W) {
  if (pair_frames_why(frames, T) || volume_why(T, H, W)) return -1;
  return thr_bytes(frames, H * W, 1);
}

extern "C" int adnm_valid_tracks_accum(const float* pred, int64_t pred_sample_stride, int64_t pred_frame_stride, const float* target, void* table,
                                       const float* thresholds_host, int64_t nthr, float value_scale, int64_t min_volume, void* ws, int64_t ws_bytes,
                                       int64_t frames, int64_t T, int64_t H, int64_t W, adnm_stream_t stream) {
  const PairCall call = {"valid_tracks_accum", pred, pred_sample_stride, pred_frame_stride, target, table, ws, ws_bytes, H, W,
                         /*flat*/ false, /*ws_optional*/ false, /*ws_aligned*/ true, /*ws_rc*/ ADNM_EINVAL};
  if (int rc = pair_check(call, thresholds_host != nullptr, tracks_why(frames, T, H, W, nthr, min_volume),
                          adnm_valid_tracks_accum_ws_bytes(frames, T, H, W, nthr),
                          "frames %lld T %lld H %lld W %lld nthr %lld min_volume %lld", (long long)frames, (long long)T, (long long)H, (long long)W,
                          (long long)nthr, (long long)min_volume))
    return rc;
  const int64_t hw = H * W, chunk = chunk_of(frames, hw, nthr);
  const Thr thr = thr_fill(thresholds_host, nthr);
  const Src s0 = {target, T * hw, hw}, s1 = {pred, pred_sample_stride, pred_frame_stride};
  hipStream_t st = (hipStream_t)stream;
  for (int64_t k0 = 0; k0 < nthr; k0 += chunk) {   // the chunks use the same workspace one after the other, in stream order
    const int64_t kc = nthr - k0 < chunk ? nthr - k0 : chunk;
    const Ws w = carve(ws, frames, T, hw, kc, 2);
    if (int rc = link_chunk("valid_tracks", s0, s1, w, thr, (int)k0, value_scale, frames, H, W, st)) return rc;
    const int64_t items = frames * kc * 2;
    {
      ADNM_PROF("tracks_reduce", st, 12.0 * items * hw);
      tracks_reduce_kernel<<<grid_of(items), kBlock, 0, st>>>(w, (double*)table, (int)k0, (int)nthr, small_of(min_volume), (int)items);
    }
    ADNM_CHECK_LAUNCH("valid_tracks");
  }
  return ADNM_OK;
}

extern "C" int adnm_label_tracks(const float* src, int64_t sample_stride, int64_t frame_stride, void* labels_i32, float thr, float value_scale,
                                 int64_t min_volume, void* ws, int64_t ws_bytes, int64_t frames, int64_t T, int64_t H, int64_t W, adnm_stream_t stream) {
  ADNM_REQUIRE(src && labels_i32 && ws, "label_tracks: null pointer");
  ADNM_REQUIRE(((uintptr_t)src | (uintptr_t)labels_i32) % 4 == 0, "label_tracks: src and labels must be 4-byte aligned");
  ADNM_REQUIRE((uintptr_t)ws % 8 == 0, "label_tracks: the workspace must be 8-byte aligned");
  ADNM_REQUIRE(min_volume >= 1, "label_tracks: min_volume >= 1, got %lld", (long long)min_volume);
  const char* why = pair_frames_why(frames, T);
  if (!why) why = volume_why(T, H, W);
  if (why) {
    adnm_set_error("label_tracks: %s (got frames %lld T %lld H %lld W %lld)", why, (long long)frames, (long long)T, (long long)H, (long long)W);
    return ADNM_EINVAL;
  }
  const int64_t hw = H * W;
  ADNM_REQUIRE(frame_stride == 0 || frame_stride >= hw, "label_tracks: frame_stride must be 0 or >= H*W, got %lld", (long long)frame_stride);
  ADNM_REQUIRE(sample_stride >= 0, "label_tracks: sample_stride must be >= 0, got %lld", (long long)sample_stride);
  const int64_t need = thr_bytes(frames, hw, 1);
  ADNM_REQUIRE(ws_bytes >= need, "label_tracks: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)need);
  Thr one = {};
  one.n = 1, one.t[0] = thr;
  const Src s0 = {src, sample_stride, frame_stride};
  const Ws w = carve(ws, frames, T, hw, 1, 1);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = link_chunk("label_tracks", s0, s0, w, one, 0, value_scale, frames, H, W, st)) return rc;
  {
    ADNM_PROF("tracks_write", st, 12.0 * frames * hw);
    tracks_write_kernel<<<grid_of(frames), kBlock, 0, st>>>(w, (int*)labels_i32, small_of(min_volume), (int)frames);
  }
  ADNM_CHECK_LAUNCH("label_tracks");
  return ADNM_OK;
}
