// Per-object intensity moments and the SAL scores (Structure, Amplitude, Location; Wernli et al. 2008) that follow from them
// (include/adnm_hip.h: adnm_valid_sal_accum, adnm_object_moments).  Field, event, object, label and min_area are those of
// objects.hip; the intensity weight of a pixel is w = intensity[q], a table of at most 256 u16 entries (the identity by default).
//
//   one workgroup   per (frame, threshold) item in sal_kernel, per frame in moments_kernel.  No workgroup waits for another one.
//   staging         each field is read from HBM once per item: one event bit (a ballot per 64 pixels) and the level q as one byte per
//                   pixel, both in LDS.  Everything after that reads bits and bytes, never floats.
//   whole field     M = sum w, Mx = sum w x, My = sum w y in u64: lanes, then waves (shuffles), then integer atomics in LDS.  Exact.
//   labelling       csrc/labelling.h, one field at a time: afterwards the word of an object's first pixel is kRoot | area and the word of
//                   its other pixels is the index of that first pixel.
//   records         R = sum w, Q = max w, X = sum w x, Y = sum w y per object, integer atomics: the first pixel of each run forms the run's
//                   sums from the staged bytes (y is constant over a run) and adds them to its root's record.  Two roots never share an
//                   aligned 2 x 2 cell (they would be 8-connected), so record (y / 2) * ceil(W / 2) + x / 2 holds at most one object and no
//                   compaction is needed; a root zeroes its record before the runs add to it.
//   where           tier 0: records and words in LDS; tier 1: the words in LDS, the records in the workgroup's slice of the workspace;
//                   tier 2: both in the slice.  The bits and the bytes of both fields are always in LDS (at most 144 KB of 160).
//   the row         every kept object (area >= min_area, R > 0) adds R, R * (R / Q) and R * |centroid - field centre| in double in a FIXED
//                   order: a lane takes its pixels ascending, a wave folds its lanes by shuffles, lane 0 adds the 16 waves ascending.  Both
//                   fields go through the same instructions, so a forecast equal to the target gives S = L2 = 0 exactly.  Lane 0 writes
//                   the item's 12 entries to the workspace; sal_fold_kernel adds the batch's rows, samples ascending from 0.0, and adds that
//                   one sum to the table.  No floating-point atomics: the same bits on every run.
#include "labelling.h"

namespace {
constexpr int kSalCols = 12, kLevels = 256, kWaves = kBlock / 64;
constexpr int64_t kMaxPixels = 65536;
constexpr int kMaxGroups = 256;                // workgroups of a launch with a slice of the workspace: one is resident per CU
constexpr size_t kLdsLimit = 160 * 1024;
// dynamic LDS: the weights (512 B), 8 u64 of whole-field sums, 16 x 4 doubles of wave partials, 2 x 4 doubles of field results, the sweep flag
constexpr size_t kTabAt = 0, kMassAt = 512, kRedAt = 576, kResAt = 1088, kFlagAt = 1152, kHead = 1168;
static_assert(kHead % 16 == 0 && kRedAt == kMassAt + 8 * 8 && kResAt == kRedAt + 8 * kWaves * 4 && kFlagAt == kResAt + 8 * 8, "the head of the LDS");

struct Weights {
  unsigned short w[kLevels];
};

__device__ __forceinline__ unsigned long long ld64(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st64(unsigned long long* p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__host__ __device__ __forceinline__ int64_t pad16(int64_t n) { return (n + 15) / 16 * 16; }
__host__ __device__ __forceinline__ int64_t cells_of(int64_t H, int64_t W) { return ((H + 1) / 2) * ((W + 1) / 2); }
// bytes of a workgroup's slice of the workspace: the records (24 per cell) from tier 1, the words (4 per pixel) in tier 2
__host__ __device__ __forceinline__ int64_t slice_bytes(int64_t hw, int64_t cells, int tier) {
  return (tier >= 1 ? 24 * cells : 0) + (tier == 2 ? (4 * hw + 7) / 8 * 8 : 0);
}

struct Rec {
  unsigned long long *X, *Y;
  unsigned *R, *Q;
};
struct Smem {
  unsigned short* tab;
  unsigned long long* mass;   // [field * 3 + (M, Mx, My)]
  double *red, *res;          // [wave * 4 + j], [field * 4 + (sum R, sum R R / Q, sum R dist, kept objects)]
  unsigned* flag;
  unsigned *bits_o, *bits_f;
  unsigned char *lev_o, *lev_f;
  Rec rec;
  unsigned* word;
};
template <int TIER>
__device__ __forceinline__ Smem carve(unsigned char* smem, unsigned char* slices, int hw, int cells) {
  Smem s;
  s.tab = (unsigned short*)(smem + kTabAt), s.mass = (unsigned long long*)(smem + kMassAt);
  s.red = (double*)(smem + kRedAt), s.res = (double*)(smem + kResAt), s.flag = (unsigned*)(smem + kFlagAt);
  unsigned char* at = smem + kHead;
  s.bits_o = (unsigned*)at, s.bits_f = s.bits_o + bit_words(hw), at += 8 * bit_words(hw);   // 16 bytes per ballot pair
  s.lev_o = at, s.lev_f = at + pad16(hw), at += 2 * pad16(hw);
  unsigned char* mine = slices + (int64_t)blockIdx.x * slice_bytes(hw, cells, TIER);
  unsigned char*& recs = TIER == 0 ? at : mine;
  s.rec.X = (unsigned long long*)recs, s.rec.Y = s.rec.X + cells, s.rec.R = (unsigned*)(s.rec.Y + cells), s.rec.Q = s.rec.R + cells;
  recs += 24 * (int64_t)cells;
  s.word = (unsigned*)(TIER <= 1 ? at : mine);
  return s;
}

// one event bit and one level byte per pixel; every word of bits[0 .. bit_words(hw)) and every byte of lev[0 .. hw) is written
__device__ __forceinline__ void stage_levels(unsigned* bits, unsigned char* lev, const float* __restrict__ src, int hw, float thr, float value_scale) {
  const int lane = threadIdx.x & 63, span = bit_words(hw) * 32;
  for (int base = (threadIdx.x >> 6) * 64; base < span; base += kBlock) {
    const int p = base + lane;
    const float q = p < hw ? eval_trunc(eval_scaled(src[p], value_scale)) : 0.f;   // 0 .. floor(value_scale) <= 255
    if (p < hw) lev[p] = (unsigned char)(int)q;
    const unsigned long long m = __ballot(p < hw && q >= thr);
    if (lane == 0) bits[base >> 5] = (unsigned)m, bits[(base >> 5) + 1] = (unsigned)(m >> 32);
  }
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off; off >>= 1) v += __shfl_down(v, off);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {   // a fixed tree: the same bits on every run
#pragma unroll
  for (int off = 32; off; off >>= 1) v += __shfl_down(v, off);
  return v;
}

// mass[0..3) += M, Mx, My of the field; the caller zeroed them and synchronises afterwards
__device__ __forceinline__ void field_mass(unsigned long long* mass, const unsigned char* lev, const unsigned short* tab, int hw, int W) {
  unsigned long long m = 0, mx = 0, my = 0;
  for (int p = threadIdx.x; p < hw; p += kBlock) {
    const unsigned w = tab[lev[p]];
    const int y = p / W;
    m += w, mx += (unsigned long long)w * (unsigned)(p - y * W), my += (unsigned long long)w * (unsigned)y;
  }
  m = wave_sum(m), mx = wave_sum(mx), my = wave_sum(my);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(mass, m), atomicAdd(mass + 1, mx), atomicAdd(mass + 2, my);
}

__device__ __forceinline__ int cell_of(int p, int W, int cw) {
  const int y = p / W;
  return (y >> 1) * cw + ((p - y * W) >> 1);
}

// labels the field and fills the record of every object: afterwards word[p] = kRoot | area at the first pixel p of an object, and
// rec.*[cell_of(p)] are its R, Q, X, Y.  Every lane of the workgroup calls it, after a barrier behind the staging.
__device__ __forceinline__ void object_records(const Smem& s, const unsigned* bits, const unsigned char* lev, int hw, int W) {
  const int tid = threadIdx.x, cw = (W + 1) / 2;
  label_field(s.word, bits, nullptr, s.flag, hw, W);
  for (int p = tid; p < hw; p += kBlock) {
    if (!bit(bits, p) || !(ld(s.word + p) & kRoot)) continue;
    const int c = cell_of(p, W, cw);
    st64(s.rec.X + c, 0ull), st64(s.rec.Y + c, 0ull), st(s.rec.R + c, 0u), st(s.rec.Q + c, 0u);
  }
  __syncthreads();
  for (int p = tid; p < hw; p += kBlock) {
    const int y = p / W, row0 = y * W;
    if (!bit(bits, p) || (p > row0 && bit(bits, p - 1))) continue;   // the first pixel of a run speaks for the run
    const int e = run_end(bits, p, row0 + W);
    unsigned sum = 0, top = 0;   // a run has at most 65 536 pixels of at most 65 535 each: below 2^32
    unsigned long long sx = 0;
    for (int i = p; i < e; ++i) {   // at most W pixels
      const unsigned w = s.tab[lev[i]];
      sum += w, sx += (unsigned long long)w * (unsigned)(i - row0), top = w > top ? w : top;
    }
    const unsigned wd = ld(s.word + p), root = (wd & kRoot) ? (unsigned)p : wd;
    const int c = cell_of((int)root, W, cw);
    atomicAdd(s.rec.R + c, sum), atomicMax(s.rec.Q + c, top);
    atomicAdd(s.rec.X + c, sx), atomicAdd(s.rec.Y + c, (unsigned long long)sum * (unsigned)y);
  }
  __syncthreads();
}

// grid (G): item = frame * nthr + k; rows: (items, 12) doubles, every entry of every row is written
template <int TIER>
__global__ __launch_bounds__(kBlock) void sal_kernel(ScoredPair pair, double* __restrict__ rows, Thr thr, float value_scale, unsigned min_area, Weights wts,
                                                     unsigned char* __restrict__ slices, int items, int H, int W, double diag) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int hw = pair.hw, nthr = thr.n, tid = threadIdx.x, cw = (W + 1) / 2;
  const Smem s = carve<TIER>(smem, slices, hw, (int)cells_of(H, W));
  if (tid < kLevels) s.tab[tid] = wts.w[tid];
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int f = item / nthr, k = item % nthr;
    __syncthreads();   // the item before is done with the bits, the bytes and the sums; the weights are staged
    stage_levels(s.bits_o, s.lev_o, pair.target(f), hw, thr.t[k], value_scale);
    stage_levels(s.bits_f, s.lev_f, pair.forecast(f), hw, thr.t[k], value_scale);
    if (tid < 8) s.mass[tid] = 0ull;
    __syncthreads();
    for (int field = 0; field < 2; ++field) {
      const unsigned* bits = field ? s.bits_f : s.bits_o;
      const unsigned char* lev = field ? s.lev_f : s.lev_o;
      field_mass(s.mass + 3 * field, lev, s.tab, hw, W);
      object_records(s, bits, lev, hw, W);   // its barriers cover the sums of the mass
      const double mass = (double)s.mass[3 * field];
      const double cx = mass > 0.0 ? (double)s.mass[3 * field + 1] / mass : 0.0, cy = mass > 0.0 ? (double)s.mass[3 * field + 2] / mass : 0.0;
      double sr = 0.0, sv = 0.0, sd = 0.0, kept = 0.0;
      for (int p = tid; p < hw; p += kBlock) {   // a lane's objects in ascending order of their first pixel
        if (!bit(bits, p)) continue;
        const unsigned wd = ld(s.word + p);
        if (!(wd & kRoot) || (wd & kAreaMask) < min_area) continue;
        const int c = cell_of(p, W, cw);
        const unsigned R = ld(s.rec.R + c);
        if (!R) continue;   // only with a zero weight: contributes nothing
        const double r = (double)R, q = (double)ld(s.rec.Q + c);
        const double dx = (double)ld64(s.rec.X + c) / r - cx, dy = (double)ld64(s.rec.Y + c) / r - cy;
        sr += r, sv += r * (r / q), sd += r * sqrt(dx * dx + dy * dy), kept += 1.0;
      }
      sr = wave_sum(sr), sv = wave_sum(sv), sd = wave_sum(sd), kept = wave_sum(kept);
      if ((tid & 63) == 0) {
        double* mine = s.red + 4 * (tid >> 6);
        mine[0] = sr, mine[1] = sv, mine[2] = sd, mine[3] = kept;
      }
      __syncthreads();
      if (tid < 4) {
        double sum = 0.0;
        for (int w = 0; w < kWaves; ++w) sum += s.red[4 * w + tid];
        s.res[4 * field + tid] = sum;
      }
      __syncthreads();   // the partials are read before the next field writes them
    }
    if (tid == 0) {
      const double mo = (double)s.mass[0], mf = (double)s.mass[3];
      double a = 0.0, l1 = 0.0, sv = 0.0, l2 = 0.0;
      const bool has_a = mo + mf > 0.0, has_l1 = mo > 0.0 && mf > 0.0, ko = s.res[3] > 0.0, kf = s.res[7] > 0.0;
      if (has_a) a = (mf - mo) / (0.5 * (mf + mo));
      if (has_l1) {
        const double dx = (double)s.mass[4] / mf - (double)s.mass[1] / mo, dy = (double)s.mass[5] / mf - (double)s.mass[2] / mo;
        l1 = sqrt(dx * dx + dy * dy) / diag;
      }
      if (ko && kf) {
        const double vo = s.res[1] / s.res[0], vf = s.res[5] / s.res[4], ro = s.res[2] / s.res[0], rf = s.res[6] / s.res[4];
        sv = (vf - vo) / (0.5 * (vf + vo)), l2 = 2.0 * fabs(rf - ro) / diag;
      }
      double* out = rows + (int64_t)item * kSalCols;   // all 12 entries, whatever is defined
      out[0] = has_a ? 1.0 : 0.0, out[1] = a, out[2] = fabs(a), out[3] = has_l1 ? 1.0 : 0.0, out[4] = l1;
      out[5] = ko && kf ? 1.0 : 0.0, out[6] = sv, out[7] = fabs(sv), out[8] = l2, out[9] = ko && kf ? l1 + l2 : 0.0;
      out[10] = ko && !kf ? 1.0 : 0.0, out[11] = kf && !ko ? 1.0 : 0.0;
    }
  }
}

// one thread per (t, k, column): table[t][k][c] += the batch's rows of frame index t, samples ascending from 0.0
__global__ void sal_fold_kernel(const double* __restrict__ rows, double* __restrict__ table, int samples, int T, int nthr) {
  const int per = nthr * kSalCols, i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T * per) return;
  const int t = i / per, rem = i - t * per;
  double sum = 0.0;
  for (int b = 0; b < samples; ++b) sum += rows[((int64_t)b * T + t) * per + rem];
  table[i] += sum;
}

// grid (G): one frame of one field per item; out: (frames, 4, hw) int64, every element written
template <int TIER>
__global__ __launch_bounds__(kBlock) void moments_kernel(const float* __restrict__ src, int64_t sstride, int64_t fstride, long long* __restrict__ out, float thr,
                                                         float value_scale, unsigned min_area, Weights wts, unsigned char* __restrict__ slices, int frames,
                                                         int T, int H, int W) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int hw = H * W, tid = threadIdx.x, cw = (W + 1) / 2;
  const Smem s = carve<TIER>(smem, slices, hw, (int)cells_of(H, W));
  if (tid < kLevels) s.tab[tid] = wts.w[tid];
  for (int f = blockIdx.x; f < frames; f += gridDim.x) {
    __syncthreads();
    stage_levels(s.bits_o, s.lev_o, pair_frame(src, sstride, fstride, f / T, f % T), hw, thr, value_scale);
    __syncthreads();
    object_records(s, s.bits_o, s.lev_o, hw, W);
    long long* img = out + (int64_t)f * 4 * hw;
    for (int p = tid; p < hw; p += kBlock) {
      long long R = 0, Q = 0, X = 0, Y = 0;
      if (bit(s.bits_o, p)) {
        const unsigned wd = ld(s.word + p);
        if ((wd & kRoot) && (wd & kAreaMask) >= min_area) {
          const int c = cell_of(p, W, cw);
          R = ld(s.rec.R + c), Q = ld(s.rec.Q + c), X = (long long)ld64(s.rec.X + c), Y = (long long)ld64(s.rec.Y + c);
        }
      }
      img[p] = R, img[hw + p] = Q, img[2 * (int64_t)hw + p] = X, img[3 * (int64_t)hw + p] = Y;
    }
  }
}

inline size_t lds_bytes(int64_t hw, int64_t cells, int tier) {
  return kHead + 2 * 4 * (size_t)bit_words((int)hw) + 2 * (size_t)pad16(hw) + (tier == 0 ? 24 * (size_t)cells : 0) + (tier <= 1 ? 4 * (size_t)hw : 0);
}
// where records and words live: the first tier whose LDS fits
inline int tier_of(int64_t H, int64_t W) {
  const int64_t hw = H * W, cells = cells_of(H, W);
  return lds_bytes(hw, cells, 0) <= kLdsLimit ? 0 : lds_bytes(hw, cells, 1) <= kLdsLimit ? 1 : 2;
}
const char* frame_why(int64_t H, int64_t W) {
  return H < 1 || W < 1 || H > kMaxPixels || W > kMaxPixels || H * W > kMaxPixels ? "1 <= H * W <= 65536" : nullptr;
}
// the SAL pass's own limits: nullptr, or the one that refuses
const char* sal_why(int64_t frames, int64_t T, int64_t H, int64_t W, int64_t nthr, int64_t min_area) {
  if (nthr < 1 || nthr > kMaxThr) return "1..8 thresholds";
  if (min_area < 1) return "min_area >= 1";
  if (const char* w = pair_frames_why(frames, T)) return w;
  return frame_why(H, W);
}
inline bool scale_ok(float value_scale) { return value_scale >= 1.f && value_scale < 256.f; }   // a NaN fails both
inline int64_t groups_of(int64_t items, int tier) { return tier == 0 || items < kMaxGroups ? items : kMaxGroups; }
inline int64_t slices_need(int64_t items, int64_t H, int64_t W) {
  const int tier = tier_of(H, W);
  return groups_of(items, tier) * slice_bytes(H * W, cells_of(H, W), tier);
}
inline Weights weights_fill(const uint16_t* intensity_host, float value_scale) {
  Weights w;
  const int levels = (int)floorf(value_scale) + 1;
  for (int i = 0; i < kLevels; ++i) w.w[i] = i < levels ? (intensity_host ? intensity_host[i] : (unsigned short)i) : (unsigned short)0;
  return w;
}
inline unsigned area_floor(int64_t min_area) { return (unsigned)(min_area > kMaxPixels + 1 ? kMaxPixels + 1 : min_area); }   // no object is larger than a frame
}  // namespace

extern "C" int64_t adnm_valid_sal_block_bytes(int64_t T, int64_t nthr) {
  if (T < 1 || T > 65535 || nthr < 1 || nthr > kMaxThr) return -1;
  return (int64_t)sizeof(double) * T * nthr * kSalCols;
}

extern "C" int64_t adnm_valid_sal_accum_ws_bytes(int64_t frames, int64_t T, int64_t H, int64_t W, int64_t nthr) {
  if (sal_why(frames, T, H, W, nthr, 1)) return -1;
  return (int64_t)sizeof(double) * frames * nthr * kSalCols + slices_need(frames * nthr, H, W);
}

extern "C" int64_t adnm_object_moments_ws_bytes(int64_t frames, int64_t T, int64_t H, int64_t W) {
  if (pair_frames_why(frames, T) || frame_why(H, W)) return -1;
  return slices_need(frames, H, W);
}

extern "C" int adnm_valid_sal_accum(const float* pred, int64_t pred_sample_stride, int64_t pred_frame_stride, const float* target, void* table,
                                    const float* thresholds_host, int64_t nthr, float value_scale, int64_t min_area, const uint16_t* intensity_host,
                                    void* ws, int64_t ws_bytes, int64_t frames, int64_t T, int64_t H, int64_t W, adnm_stream_t stream) {
  const PairCall call = {"valid_sal_accum", pred, pred_sample_stride, pred_frame_stride, target, table, ws, ws_bytes, H, W,
                         /*flat*/ false, /*ws_optional*/ false, /*ws_aligned*/ true, /*ws_rc*/ ADNM_EINVAL};
  const char* why = sal_why(frames, T, H, W, nthr, min_area);
  if (!why && !scale_ok(value_scale)) why = "value_scale finite with 1 <= floor(value_scale) <= 255";
  if (int rc = pair_check(call, thresholds_host != nullptr, why, adnm_valid_sal_accum_ws_bytes(frames, T, H, W, nthr),
                          "frames %lld T %lld H %lld W %lld nthr %lld min_area %lld value_scale %g", (long long)frames, (long long)T, (long long)H,
                          (long long)W, (long long)nthr, (long long)min_area, (double)value_scale))
    return rc;
  const int64_t hw = H * W, items = frames * nthr, cells = cells_of(H, W);
  const Thr thr = thr_fill(thresholds_host, nthr);
  const ScoredPair pair = {pred, pred_sample_stride, pred_frame_stride, target, (int)T, (int)hw};
  const Weights wts = weights_fill(intensity_host, value_scale);
  const unsigned small = area_floor(min_area);
  const int tier = tier_of(H, W);
  const size_t lds = lds_bytes(hw, cells, tier);
  const unsigned grid = (unsigned)groups_of(items, tier);
  double* rows = (double*)ws;
  unsigned char* slices = (unsigned char*)ws + sizeof(double) * items * kSalCols;
  const double diag = sqrt((double)H * (double)H + (double)W * (double)W);
  hipStream_t st = (hipStream_t)stream;
#define ADNM_SAL_LAUNCH(TIER)                                                                                                                   \
  {                                                                                                                                             \
    ADNM_ALLOW_LDS(sal_kernel<TIER>, lds, "valid_sal");                                                                                         \
    ADNM_PROF("valid_sal", st, 8.0 * items * hw);                                                                                               \
    sal_kernel<TIER><<<grid, kBlock, lds, st>>>(pair, rows, thr, value_scale, small, wts, slices, (int)items, (int)H, (int)W, diag);            \
  }
  if (tier == 0) ADNM_SAL_LAUNCH(0) else if (tier == 1) ADNM_SAL_LAUNCH(1) else ADNM_SAL_LAUNCH(2)
#undef ADNM_SAL_LAUNCH
  ADNM_CHECK_LAUNCH("valid_sal");
  {
    const int cellsT = (int)(T * nthr * kSalCols);
    ADNM_PROF("valid_sal_fold", st, 8.0 * items * kSalCols);
    sal_fold_kernel<<<(cellsT + 255) / 256, 256, 0, st>>>(rows, (double*)table, (int)(frames / T), (int)T, (int)nthr);
  }
  ADNM_CHECK_LAUNCH("valid_sal_fold");
  return ADNM_OK;
}

extern "C" int adnm_object_moments(const float* src, int64_t sample_stride, int64_t frame_stride, void* moments_i64, float thr, float value_scale,
                                   int64_t min_area, const uint16_t* intensity_host, void* ws, int64_t ws_bytes, int64_t frames, int64_t T, int64_t H,
                                   int64_t W, adnm_stream_t stream) {
  ADNM_REQUIRE(src && moments_i64, "object_moments: null pointer");
  ADNM_REQUIRE((uintptr_t)src % 4 == 0 && (uintptr_t)moments_i64 % 8 == 0, "object_moments: src must be 4-byte and moments 8-byte aligned");
  ADNM_REQUIRE((uintptr_t)ws % 8 == 0, "object_moments: the workspace must be 8-byte aligned");
  ADNM_REQUIRE(min_area >= 1, "object_moments: min_area >= 1, got %lld", (long long)min_area);
  ADNM_REQUIRE(scale_ok(value_scale), "object_moments: value_scale finite with 1 <= floor(value_scale) <= 255, got %g", (double)value_scale);
  const char* why = pair_frames_why(frames, T);
  if (!why) why = frame_why(H, W);
  if (why) {
    adnm_set_error("object_moments: %s (got frames %lld T %lld H %lld W %lld)", why, (long long)frames, (long long)T, (long long)H, (long long)W);
    return ADNM_EINVAL;
  }
  const int64_t hw = H * W, cells = cells_of(H, W);
  ADNM_REQUIRE(frame_stride == 0 || frame_stride >= hw, "object_moments: frame_stride must be 0 or >= H*W, got %lld", (long long)frame_stride);
  ADNM_REQUIRE(sample_stride >= 0, "object_moments: sample_stride must be >= 0, got %lld", (long long)sample_stride);
  const int64_t need = slices_need(frames, H, W);
  ADNM_REQUIRE(ws_bytes >= need && (ws || !need), "object_moments: workspace %lld < %lld bytes", (long long)(ws ? ws_bytes : 0), (long long)need);
  const Weights wts = weights_fill(intensity_host, value_scale);
  const unsigned small = area_floor(min_area);
  const int tier = tier_of(H, W);
  const size_t lds = lds_bytes(hw, cells, tier);
  const unsigned grid = (unsigned)groups_of(frames, tier);
  hipStream_t st = (hipStream_t)stream;
#define ADNM_MOMENTS_LAUNCH(TIER)                                                                                                               \
  {                                                                                                                                             \
    ADNM_ALLOW_LDS(moments_kernel<TIER>, lds, "object_moments");                                                                                \
    ADNM_PROF("object_moments", st, 36.0 * frames * hw);                                                                                        \
    moments_kernel<TIER><<<grid, kBlock, lds, st>>>(src, sample_stride, frame_stride, (long long*)moments_i64, thr, value_scale, small, wts,   \
                                                    (unsigned char*)ws, (int)frames, (int)T, (int)H, (int)W);                                   \
  }
  if (tier == 0) ADNM_MOMENTS_LAUNCH(0) else if (tier == 1) ADNM_MOMENTS_LAUNCH(1) else ADNM_MOMENTS_LAUNCH(2)
#undef ADNM_MOMENTS_LAUNCH
  ADNM_CHECK_LAUNCH("object_moments");
  return ADNM_OK;
}
