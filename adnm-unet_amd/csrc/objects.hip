// Connected-component labelling of the event masks and the object scores that follow from it (include/adnm_hip.h: adnm_valid_objects_accum,
// adnm_label_objects).  An event is q(v) >= thr with q = eval_trunc(eval_scaled(v, value_scale)) of adnm_common.h; an object is
// an 8-connected component of one frame's event mask; its label is 1 + the row-major index of its first pixel.
//
//   one workgroup   per (frame, threshold) in objects_kernel — it labels the target, then the forecast, because matching needs both masks —
//                   and per frame in label_kernel.  No workgroup waits for another one: every barrier below is a workgroup barrier.
//   the bits        each field is read from HBM once per workgroup and kept as one event bit per pixel in LDS (a ballot per 64 pixels).
//                   Everything after that reads bits, never floats.
//   labelling       csrc/labelling.h, shared with sal.hip: the words (one u32 per pixel, in LDS where the frame fits beside the bits, H * W <=
//                   about 38 000, and in the workgroup's slice of the workspace otherwise), the runs, the unions and the areas are stated there.
//   the row         every root of at least min_area pixels adds its entries to 23 u64 counters in LDS; the non-zero ones go to the table
//                   as double atomics.  Every addend and every sum is an integer below 2^53, so the table is exact and the same bits on
//                   every run although the order of the atomics is not fixed.
#include "labelling.h"

namespace {
constexpr int kCols = 23, kBins = 17;          // count, area, area^2, largest, matched, matched area, 17 bins of floor(log2(area))
static_assert(kCols == 6 + kBins, "six sums, then the size histogram");
constexpr int64_t kMaxPixels = 65536;          // an area fits 17 bits (bin 16 is the last); area^2 <= 2^32
constexpr int kMaxGroups = 512;                // workgroups of a launch whose words live in the workspace
constexpr size_t kLdsLimit = 160 * 1024;
constexpr size_t kHead = 8 * 24 + 16;          // 23 u64 counters (24 for alignment), then the sweep flag

struct Smem {
  unsigned long long* acc;
  unsigned *flag, *bits_o, *bits_f, *word;
};
// dynamic LDS: counters, flag, the two bit fields, then (LDSW) the words
template <bool LDSW>
__device__ __forceinline__ Smem carve(unsigned char* smem, unsigned* ws, int hw) {
  Smem s;
  s.acc = (unsigned long long*)smem;
  s.flag = (unsigned*)(smem + 8 * 24);
  s.bits_o = (unsigned*)(smem + kHead);
  s.bits_f = s.bits_o + bit_words(hw);
  if constexpr (LDSW) s.word = s.bits_f + bit_words(hw);
  else s.word = ws + (int64_t)blockIdx.x * hw;
  return s;
}

// grid (G): item = frame * nthr + k
template <bool LDSW>
__global__ __launch_bounds__(kBlock) void objects_kernel(ScoredPair pair, double* __restrict__ table, Thr thr, float value_scale, unsigned min_area,
                                                         unsigned* __restrict__ ws, int items, int W) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int hw = pair.hw, nthr = thr.n, tid = threadIdx.x;
  const Smem s = carve<LDSW>(smem, ws, hw);
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int f = item / nthr, k = item % nthr, t = f % pair.T;
    __syncthreads();   // the item before is done with the bits
    stage_bits(s.bits_o, pair.target(f), hw, thr.t[k], value_scale);
    stage_bits(s.bits_f, pair.forecast(f), hw, thr.t[k], value_scale);
    for (int field = 0; field < 2; ++field) {
      const unsigned* bits = field ? s.bits_f : s.bits_o;
      if (tid < 24) s.acc[tid] = 0ull;
      __syncthreads();   // the bits and the zeroed counters
      label_field(s.word, bits, field ? s.bits_o : s.bits_f, s.flag, hw, W);
      unsigned n = 0, area = 0, largest = 0, matched = 0, matched_area = 0;
      unsigned long long squares = 0;
      for (int p = tid; p < hw; p += kBlock) {
        if (!bit(bits, p)) continue;
        const unsigned wd = ld(s.word + p), a = wd & kAreaMask;
        if (!(wd & kRoot) || a < min_area) continue;
        n += 1, area += a, squares += (unsigned long long)a * a, largest = a > largest ? a : largest;
        if (wd & kMatched) matched += 1, matched_area += a;
        atomicAdd(&s.acc[6 + 31 - __clz((int)a)], 1ull);   // a <= 65536: bin <= 16
      }
      if (n) {
        atomicAdd(&s.acc[0], (unsigned long long)n), atomicAdd(&s.acc[1], (unsigned long long)area), atomicAdd(&s.acc[2], squares);
        atomicMax(&s.acc[3], (unsigned long long)largest);
        if (matched) atomicAdd(&s.acc[4], (unsigned long long)matched), atomicAdd(&s.acc[5], (unsigned long long)matched_area);
      }
      __syncthreads();
      if (tid < kCols && s.acc[tid]) unsafeAtomicAdd(&table[(((int64_t)t * 2 + field) * nthr + k) * kCols + tid], (double)s.acc[tid]);
      __syncthreads();   // the counters are read before the next field zeroes them
    }
  }
}

// grid (G): one frame of one field per item; frame f = b * T + t of the field is pair_frame(src, sstride, fstride, b, t)
template <bool LDSW>
__global__ __launch_bounds__(kBlock) void label_kernel(const float* __restrict__ src, int64_t sstride, int64_t fstride, int* __restrict__ labels, float thr,
                                                       float value_scale, unsigned min_area, unsigned* __restrict__ ws, int frames, int T, int H, int W) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int hw = H * W, tid = threadIdx.x;
  const Smem s = carve<LDSW>(smem, ws, hw);
  for (int f = blockIdx.x; f < frames; f += gridDim.x) {
    __syncthreads();
    stage_bits(s.bits_o, pair_frame(src, sstride, fstride, f / T, f % T), hw, thr, value_scale);
    __syncthreads();
    label_field(s.word, s.bits_o, nullptr, s.flag, hw, W);
    int* out = labels + (int64_t)f * hw;
    for (int p = tid; p < hw; p += kBlock) {
      int lab = 0;
      if (bit(s.bits_o, p)) {
        const unsigned wd = ld(s.word + p), root = (wd & kRoot) ? (unsigned)p : wd;
        if ((ld(s.word + root) & kAreaMask) >= min_area) lab = (int)root + 1;
      }
      out[p] = lab;
    }
  }
}

inline size_t lds_bytes(int64_t hw, bool words) { return kHead + 2 * sizeof(unsigned) * (size_t)bit_words((int)hw) + (words ? sizeof(unsigned) * (size_t)hw : 0); }
inline bool words_in_lds(int64_t hw) { return lds_bytes(hw, true) <= kLdsLimit; }
const char* frame_why(int64_t H, int64_t W) {
  return H < 1 || W < 1 || H > kMaxPixels || W > kMaxPixels || H * W > kMaxPixels ? "1 <= H * W <= 65536" : nullptr;
}
// the object scores' own limits: nullptr, or the one that refuses
const char* objects_why(int64_t frames, int64_t T, int64_t H, int64_t W, int64_t nthr, int64_t min_area) {
  if (nthr < 1 || nthr > kMaxThr) return "1..8 thresholds";
  if (min_area < 1) return "min_area >= 1";
  if (const char* w = pair_frames_why(frames, T)) return w;
  return frame_why(H, W);
}
inline int64_t groups_of(int64_t items, int64_t hw) { return words_in_lds(hw) || items < kMaxGroups ? items : kMaxGroups; }
inline int64_t ws_need(int64_t items, int64_t hw) { return words_in_lds(hw) ? 0 : (int64_t)sizeof(unsigned) * groups_of(items, hw) * hw; }
}  // namespace

extern "C" int64_t adnm_valid_objects_block_bytes(int64_t T, int64_t nthr) {
  if (T < 1 || T > 65535 || nthr < 1 || nthr > kMaxThr) return -1;
  return (int64_t)sizeof(double) * T * 2 * nthr * kCols;
}

extern "C" int64_t adnm_valid_objects_accum_ws_bytes(int64_t frames, int64_t T, int64_t H, int64_t W, int64_t nthr) {
  if (objects_why(frames, T, H, W, nthr, 1)) return -1;
  return ws_need(frames * nthr, H * W);
}

extern "C" int64_t adnm_label_objects_ws_bytes(int64_t frames, int64_t T, int64_t H, int64_t W) {
  if (pair_frames_why(frames, T) || frame_why(H, W)) return -1;
  return ws_need(frames, H * W);
}

extern "C" int adnm_valid_objects_accum(const float* pred, int64_t pred_sample_stride, int64_t pred_frame_stride, const float* target, void* table,
                                        const float* thresholds_host, int64_t nthr, float value_scale, int64_t min_area, void* ws, int64_t ws_bytes,
                                        int64_t frames, int64_t T, int64_t H, int64_t W, adnm_stream_t stream) {
  const PairCall call = {"valid_objects_accum", pred, pred_sample_stride, pred_frame_stride, target, table, ws, ws_bytes, H, W,
                         /*flat*/ false, /*ws_optional*/ true, /*ws_aligned*/ true, /*ws_rc*/ ADNM_EINVAL};
  if (int rc = pair_check(call, thresholds_host != nullptr, objects_why(frames, T, H, W, nthr, min_area),
                          adnm_valid_objects_accum_ws_bytes(frames, T, H, W, nthr),
                          "frames %lld T %lld H %lld W %lld nthr %lld min_area %lld", (long long)frames, (long long)T, (long long)H, (long long)W,
                          (long long)nthr, (long long)min_area))
    return rc;
  const int64_t hw = H * W, items = frames * nthr;
  const Thr thr = thr_fill(thresholds_host, nthr);
  const ScoredPair pair = {pred, pred_sample_stride, pred_frame_stride, target, (int)T, (int)hw};
  const unsigned small = (unsigned)(min_area > kMaxPixels + 1 ? kMaxPixels + 1 : min_area);   // no object is larger than a frame
  const bool in_lds = words_in_lds(hw);
  const size_t lds = lds_bytes(hw, in_lds);
  const unsigned grid = (unsigned)groups_of(items, hw);
  hipStream_t st = (hipStream_t)stream;
  if (in_lds) {
    ADNM_ALLOW_LDS(objects_kernel<true>, lds, "valid_objects");
    ADNM_PROF("valid_objects", st, 8.0 * items * hw);
    objects_kernel<true><<<grid, kBlock, lds, st>>>(pair, (double*)table, thr, value_scale, small, nullptr, (int)items, (int)W);
  } else {
    ADNM_PROF("valid_objects", st, 8.0 * items * hw);
    objects_kernel<false><<<grid, kBlock, lds, st>>>(pair, (double*)table, thr, value_scale, small, (unsigned*)ws, (int)items, (int)W);
  }
  ADNM_CHECK_LAUNCH("valid_objects");
  return ADNM_OK;
}

extern "C" int adnm_label_objects(const float* src, int64_t sample_stride, int64_t frame_stride, void* labels_i32, float thr, float value_scale,
                                  int64_t min_area, void* ws, int64_t ws_bytes, int64_t frames, int64_t T, int64_t H, int64_t W, adnm_stream_t stream) {
  ADNM_REQUIRE(src && labels_i32, "label_objects: null pointer");
  ADNM_REQUIRE(((uintptr_t)src | (uintptr_t)labels_i32) % 4 == 0, "label_objects: src and labels must be 4-byte aligned");
  ADNM_REQUIRE((uintptr_t)ws % 8 == 0, "label_objects: the workspace must be 8-byte aligned");
  ADNM_REQUIRE(min_area >= 1, "label_objects: min_area >= 1, got %lld", (long long)min_area);
  const char* why = pair_frames_why(frames, T);
  if (!why) why = frame_why(H, W);
  if (why) {
    adnm_set_error("label_objects: %s (got frames %lld T %lld H %lld W %lld)", why, (long long)frames, (long long)T, (long long)H, (long long)W);
    return ADNM_EINVAL;
  }
  const int64_t hw = H * W;
  ADNM_REQUIRE(frame_stride == 0 || frame_stride >= hw, "label_objects: frame_stride must be 0 or >= H*W, got %lld", (long long)frame_stride);
  ADNM_REQUIRE(sample_stride >= 0, "label_objects: sample_stride must be >= 0, got %lld", (long long)sample_stride);
  const int64_t need = ws_need(frames, hw);
  ADNM_REQUIRE(ws_bytes >= need && (ws || !need), "label_objects: workspace %lld < %lld bytes", (long long)(ws ? ws_bytes : 0), (long long)need);
  const unsigned small = (unsigned)(min_area > kMaxPixels + 1 ? kMaxPixels + 1 : min_area);
  const bool in_lds = words_in_lds(hw);
  const size_t lds = lds_bytes(hw, in_lds);
  const unsigned grid = (unsigned)groups_of(frames, hw);
  hipStream_t st = (hipStream_t)stream;
  if (in_lds) {
    ADNM_ALLOW_LDS(label_kernel<true>, lds, "label_objects");
    ADNM_PROF("label_objects", st, 8.0 * frames * hw);
    label_kernel<true><<<grid, kBlock, lds, st>>>(src, sample_stride, frame_stride, (int*)labels_i32, thr, value_scale, small, nullptr, (int)frames, (int)T,
                                                  (int)H, (int)W);
  } else {
    ADNM_PROF("label_objects", st, 8.0 * frames * hw);
    label_kernel<false><<<grid, kBlock, lds, st>>>(src, sample_stride, frame_stride, (int*)labels_i32, thr, value_scale, small, (unsigned*)ws, (int)frames,
                                                   (int)T, (int)H, (int)W);
  }
  ADNM_CHECK_LAUNCH("label_objects");
  return ADNM_OK;
}
