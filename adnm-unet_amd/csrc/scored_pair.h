// The scored pair: what every Validator score that compares a forecast with a target is handed, stated ONCE.
//
// An entry point of this contract (adnm_valid_pool_accum, adnm_valid_fss_accum, adnm_valid_iscale_accum, adnm_valid_nprob_accum: neighbour.hip;
// adnm_valid_spectrum_accum: spectrum.hip;
// adnm_valid_joint_accum: joint.hip; adnm_valid_objects_accum: objects.hip; adnm_valid_sal_accum: sal.hip; adnm_valid_tracks_accum: tracks.hip) takes
//   the forecast   `frames` frames addressed by (pred, pred_sample_stride, pred_frame_stride): frame f = b * T + t starts at
//                  pred + b * sstride + t * fstride.  fstride = 0 holds one frame for all T lead times (the persistence baseline);
//   the target     contiguous, frame f at target + f * hw;
//   the table      doubles in the Validator's one allocation, ADDED to, row t = f mod T (the ONE deviation: a track of tracks.hip spans frames and
//                  belongs to no single frame index, so that table is (2, nthr, 7 + 4 T) with its per-frame entries as columns);
//   a workspace    of at least the entry point's *_ws_bytes;
// and, where it counts events, up to kMaxThr thresholds from a host array.  pair_check is the first thing each of them calls: a stride
// or alignment mistake is refused there, on the host, before it can become an out-of-bounds read.  A new score writes its own limits
// (a `const char* why` function), its kernels and its row of the Validator's parts table; nothing of this file is repeated.
#pragma once
#include "adnm_common.h"

constexpr int kMaxThr = 8;
struct Thr {
  float t[kMaxThr];
  int n;
};
// the thresholds as a kernel argument; nthr is in 1..kMaxThr (the entry point's limits)
inline Thr thr_fill(const float* thresholds_host, int64_t nthr) {
  Thr thr;
  thr.n = (int)nthr;
  for (int k = 0; k < kMaxThr; ++k) thr.t[k] = k < nthr ? thresholds_host[k] : 0.f;
  return thr;
}

// The event bits of a pixel pair on the quantised values q = eval_trunc(eval_scaled(v)) of adnm_common.h: bit k = the target's
// q >= thr_k, bit 8 + k = the forecast's.
__device__ __forceinline__ uint32_t pair_bits(float tv, float pv, float value_scale, const Thr& thr) {
  const float ti = eval_trunc(eval_scaled(tv, value_scale)), pi = eval_trunc(eval_scaled(pv, value_scale));
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < kMaxThr; ++k)
    if (k < thr.n) m |= (ti >= thr.t[k] ? 1u << k : 0u) | (pi >= thr.t[k] ? 0x100u << k : 0u);
  return m;
}

// Frame t of sample b of a strided field.  This and ScoredPair::target are the two address formulas, written here and nowhere else.
__device__ __forceinline__ const float* pair_frame(const float* base, int64_t sstride, int64_t fstride, int b, int t) {
  return base + (int64_t)b * sstride + (int64_t)t * fstride;
}
// The pair as a kernel argument.
struct ScoredPair {
  const float* pred;
  int64_t sstride, fstride;
  const float* tgt;
  int T, hw;   // lead times per sample, pixels per frame
  __device__ __forceinline__ const float* forecast(int b, int t) const { return pair_frame(pred, sstride, fstride, b, t); }
  __device__ __forceinline__ const float* forecast(int f) const { return forecast(f / T, f % T); }
  __device__ __forceinline__ const float* target(int f) const { return tgt + (int64_t)f * hw; }
};

// frames and T of a pair (and of adnm_label_objects' one field): nullptr, or the limit that refuses them
inline const char* pair_frames_why(int64_t frames, int64_t T) {
  if (T < 1 || frames < 1 || frames % T != 0) return "T >= 1 must divide frames";
  if (frames > 65535) return "frames <= 65535";
  return nullptr;
}
// the frame shape of the two neighbourhood scores: 16-bit tile coordinates, and counts that stay exact in fp32
inline const char* pair_tiled_shape_why(int64_t H, int64_t W) {
  if (H < 1 || W < 1 || H >= 32768 || W >= 32768) return "H and W must be in [1, 32768)";
  if (H * W >= (1ll << 24)) return "pixels per frame < 2^24";
  return nullptr;
}

// 16-byte loads need every frame start of both fields, and with a row length `row` every row start, on a multiple of 4 floats;
// anything else (an odd W, a 4-byte aligned slice of a larger buffer) takes the scalar path: same result
inline bool pair_quads(int64_t row, int64_t sstride, int64_t fstride, const float* pred, const float* target) {
  return row % 4 == 0 && sstride % 4 == 0 && fstride % 4 == 0 && adnm_quad_aligned(ADNM_F32, {pred, target});
}

// What an entry point was called with, and what differs between the five.
struct PairCall {
  const char* name;      // as its messages begin
  const float* pred;
  int64_t sstride, fstride;
  const float* target;
  const void* table;
  const void* ws;
  int64_t ws_bytes, H, W;
  bool flat;             // a frame is W = hw pixels with no rows (the wording "hw" instead of "H*W")
  bool ws_optional;      // ws may be null when zero bytes are needed
  bool ws_aligned;       // the workspace holds 8-byte items
  int ws_rc;             // what a short workspace returns
};
// The one host check.  others: the entry point's further pointers (thresholds, its small table, a workspace that is always needed) are
// all there; why: the verdict of its limits, pair_frames_why among them at the place the entry point gives it (nullptr: inside);
// need: its *_ws_bytes, looked at only once the shape has passed; got_fmt, ...: the values its shape refusal prints after "got".
// ADNM_OK, or the error is set and the code to return is returned.
inline int pair_check(const PairCall& c, bool others, const char* why, int64_t need, const char* got_fmt, ...) {
  ADNM_REQUIRE(c.pred && c.target && c.table && others, "%s: null pointer", c.name);
  ADNM_REQUIRE(((uintptr_t)c.pred | (uintptr_t)c.target) % 4 == 0, "%s: pred and target must be 4-byte aligned", c.name);
  ADNM_REQUIRE((uintptr_t)c.table % 8 == 0, "%s: the table must be 8-byte aligned", c.name);
  ADNM_REQUIRE(!c.ws_aligned || (uintptr_t)c.ws % 8 == 0, "%s: the workspace must be 8-byte aligned", c.name);
  if (why) {
    char got[192];
    va_list ap;
    va_start(ap, got_fmt);
    vsnprintf(got, sizeof got, got_fmt, ap);
    va_end(ap);
    ADNM_REQUIRE(false, "%s: %s (got %s)", c.name, why, got);
  }
  ADNM_REQUIRE(c.fstride == 0 || c.fstride >= c.H * c.W, "%s: pred_frame_stride must be 0 or >= %s, got %lld", c.name, c.flat ? "hw" : "H*W",
               (long long)c.fstride);
  ADNM_REQUIRE(c.sstride >= 0, "%s: pred_sample_stride must be >= 0, got %lld", c.name, (long long)c.sstride);
  if (c.ws_bytes < need || (!c.ws && (need || !c.ws_optional))) {
    adnm_set_error("%s: workspace %lld < %lld bytes", c.name, (long long)(c.ws_optional && !c.ws ? 0 : c.ws_bytes), (long long)need);
    return c.ws_rc;
  }
  return ADNM_OK;
}
