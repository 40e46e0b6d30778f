// The joint histogram of the quantised observation and the quantised forecast per frame index (include/adnm_hip.h: adnm_valid_joint_accum;
// DESIGN.md §4l).  q(v) = eval_trunc(eval_scaled(v, value_scale)) of adnm_common.h, the level SimplifiedEvaluator compares with its
// thresholds; L = floor(value_scale) + 1 levels; table[t][q(target)][q(forecast)] += 1 for every pixel of every frame f with f mod T = t.
//
//   joint_kernel   grid (G, T).  Row t's work is cut into items of kChunk pixels of one frame (sample b, chunk c); workgroup g of row t takes
//                  the items g, g + G, ... and counts them into ONE u32 histogram of L * L bins in LDS (dynamic, 4 L^2 <= 64 KB), which it
//                  flushes once at the end.  Each pixel of each field is read from HBM once: 16 bytes per access (VEC) or float by float, all
//                  loads of an item issued before the first count.
//   the hot bin    radar fields are mostly zero, so nearly every lane of every wave holds bin (0, 0), and 64 LDS atomics on one address are
//                  served one after the other.  The lanes with bin 0 are therefore counted with a ballot and a popcount into a per-wave
//                  scalar, added to the LDS histogram once per workgroup; only the other lanes issue an LDS atomic.  A wave of zeros costs a
//                  compare, a ballot and a scalar add per pixel group and touches no LDS.
//   the flush      only the non-zero bins go to the table, as no-return double atomics (a real field fills a few hundred bins near the
//                  diagonal).  Every addend and every partial sum is an integer below 2^53, so the additions are exact in any order: the
//                  result is exact and the same bits on every run although the order of the atomics is not fixed.
//   counters       u32.  G is chosen so that a workgroup counts at most 2^31 pixels; no narrower counter is used.
#include "scored_pair.h"

namespace {
constexpr int kBlock = 256;
constexpr int kChunk = 4096;        // pixels of one item: 4 float4 (VEC) or 16 floats per thread and field
constexpr int kTargetGroups = 2048;   // workgroups of a launch that has that much work: 8 per CU, 4 of them resident at L = 91
constexpr int64_t kMaxItemsPerGroup = 1 << 19;   // * kChunk = 2^31 pixels: a u32 bin cannot overflow

__device__ __forceinline__ int joint_bin(float o, float f, float value_scale, int L) {
  return (int)eval_trunc(eval_scaled(o, value_scale)) * L + (int)eval_trunc(eval_scaled(f, value_scale));
}

// one pixel group of the whole wave: `valid` lanes with bin 0 are counted by ballot, the others add to LDS.  Every lane of the wave calls it.
__device__ __forceinline__ void joint_count(unsigned* hist, bool valid, int bin, unsigned& zeros) {
  zeros += (unsigned)__popcll(__ballot(valid && bin == 0));
  if (valid && bin != 0) atomicAdd(&hist[bin], 1u);
}

// VEC: pair_quads with hw as the row length.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void joint_kernel(ScoredPair pair, double* __restrict__ table, float value_scale, int L, int chunks, int items) {
  extern __shared__ __attribute__((aligned(16))) unsigned hist[];   // L * L
  const int t = blockIdx.y, bins = L * L, T = pair.T, hw = pair.hw;
  for (int i = threadIdx.x; i < bins; i += kBlock) hist[i] = 0u;
  __syncthreads();
  unsigned zeros = 0;   // wave-uniform: the pixels of this wave in bin (0, 0)
  constexpr int kIter = VEC ? kChunk / (4 * kBlock) : kChunk / kBlock;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int b = item / chunks, px0 = (item % chunks) * kChunk;
    const float* o_src = pair.target(b * T + t) + px0;
    const float* f_src = pair.forecast(b, t) + px0;
    const int left = hw - px0;   // pixels of the frame from px0 on (>= 1)
    if (VEC) {
      float4 o[kIter], f[kIter];
#pragma unroll
      for (int k = 0; k < kIter; ++k) {
        const int p = (k * kBlock + threadIdx.x) * 4;
        o[k] = f[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p < left) o[k] = *(const float4*)(o_src + p), f[k] = *(const float4*)(f_src + p);
      }
#pragma unroll
      for (int k = 0; k < kIter; ++k) {
        const bool valid = (k * kBlock + threadIdx.x) * 4 < left;   // hw is a multiple of 4: a group of four is inside or outside
        joint_count(hist, valid, joint_bin(o[k].x, f[k].x, value_scale, L), zeros);
        joint_count(hist, valid, joint_bin(o[k].y, f[k].y, value_scale, L), zeros);
        joint_count(hist, valid, joint_bin(o[k].z, f[k].z, value_scale, L), zeros);
        joint_count(hist, valid, joint_bin(o[k].w, f[k].w, value_scale, L), zeros);
      }
    } else {
      float o[kIter], f[kIter];
#pragma unroll
      for (int k = 0; k < kIter; ++k) {
        const int p = k * kBlock + threadIdx.x;
        o[k] = f[k] = 0.f;
        if (p < left) o[k] = o_src[p], f[k] = f_src[p];
      }
#pragma unroll
      for (int k = 0; k < kIter; ++k) joint_count(hist, k * kBlock + threadIdx.x < left, joint_bin(o[k], f[k], value_scale, L), zeros);
    }
  }
  if ((threadIdx.x & 63) == 0 && zeros) atomicAdd(&hist[0], zeros);
  __syncthreads();
  double* row = table + (int64_t)t * bins;
  for (int i = threadIdx.x; i < bins; i += kBlock) {
    const unsigned n = hist[i];
    if (n) unsafeAtomicAdd(&row[i], (double)n);   // integers below 2^53: exact in any order
  }
}

inline int64_t joint_levels(float value_scale) {
  if (!(value_scale >= 1.f && value_scale < 128.f)) return -1;   // a NaN fails both; 2 <= L <= 128
  return (int64_t)floorf(value_scale) + 1;
}
const char* joint_why(int64_t frames, int64_t T, int64_t hw, float value_scale) {
  if (joint_levels(value_scale) < 0) return "value_scale must be finite with 2 <= L = floor(value_scale) + 1 <= 128";
  if (const char* w = pair_frames_why(frames, T)) return w;
  if (hw < 1 || hw >= (1 << 24)) return "1 <= hw < 2^24";
  return nullptr;
}
}  // namespace

extern "C" int64_t adnm_valid_joint_levels(float value_scale) { return joint_levels(value_scale); }

extern "C" int64_t adnm_valid_joint_block_bytes(int64_t T, float value_scale) {
  const int64_t L = joint_levels(value_scale);
  if (L < 0 || T < 1 || T > 65535) return -1;
  return (int64_t)sizeof(double) * T * L * L;
}

extern "C" int64_t adnm_valid_joint_accum_ws_bytes(int64_t frames, int64_t T, int64_t hw, float value_scale) {
  return joint_why(frames, T, hw, value_scale) ? -1 : 0;   // the partial histograms live in LDS
}

extern "C" int adnm_valid_joint_accum(const float* pred, int64_t pred_sample_stride, int64_t pred_frame_stride, const float* target, void* table,
                                      float value_scale, void* ws, int64_t ws_bytes, int64_t frames, int64_t T, int64_t hw, adnm_stream_t stream) {
  const PairCall call = {"valid_joint_accum", pred, pred_sample_stride, pred_frame_stride, target, table, ws, ws_bytes, 1, hw,
                         /*flat*/ true, /*ws_optional*/ true, /*ws_aligned*/ true, /*ws_rc*/ ADNM_EINVAL};
  if (int rc = pair_check(call, true, joint_why(frames, T, hw, value_scale),
                          adnm_valid_joint_accum_ws_bytes(frames, T, hw, value_scale),
                          "frames %lld T %lld hw %lld value_scale %g", (long long)frames, (long long)T, (long long)hw, (double)value_scale))
    return rc;
  const int64_t L = joint_levels(value_scale), chunks = adnm_cdiv(hw, kChunk), items = (frames / T) * chunks;   // items <= 65535 * 4096 = 2^28
  int64_t groups = kTargetGroups / T > 1 ? kTargetGroups / T : 1;
  if (groups > items) groups = items;
  if (groups < adnm_cdiv(items, kMaxItemsPerGroup)) groups = adnm_cdiv(items, kMaxItemsPerGroup);
  const bool vec = pair_quads(hw, pred_sample_stride, pred_frame_stride, pred, target);
  const ScoredPair pair = {pred, pred_sample_stride, pred_frame_stride, target, (int)T, (int)hw};
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)groups, (unsigned)T);
  const size_t lds = sizeof(unsigned) * (size_t)(L * L);   // <= 64 KB: no function attribute is needed
  {
    ADNM_PROF("valid_joint", st, 8.0 * frames * hw);
    if (vec) joint_kernel<true><<<grid, kBlock, lds, st>>>(pair, (double*)table, value_scale, (int)L, (int)chunks, (int)items);
    else joint_kernel<false><<<grid, kBlock, lds, st>>>(pair, (double*)table, value_scale, (int)L, (int)chunks, (int)items);
  }
  ADNM_CHECK_LAUNCH("valid_joint");
  return ADNM_OK;
}
