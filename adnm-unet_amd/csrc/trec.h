// What the two advection schemes share (advect.hip: the block scheme; flow.hip: the sub-pixel flow): the limits, the
// order of the pick, and the launch of trec_cost, which stays in advect.hip.
#pragma once
#include "adnm_common.h"

constexpr int kTrecMaxBs = 32, kTrecMaxR = 8;

// (cost, dy^2 + dx^2, dy, dx) as one integer whose order is the lexicographic one: cost < 2^32 (a sample's whole-frame sum is below
// 2^24 * 255), dy^2 + dx^2 <= 128 in 8 bits, dy + R and dx + R <= 16 in 5 bits each.
static __device__ __forceinline__ uint64_t trec_key(uint64_t cost, int d, int R) {
  const int D = 2 * R + 1, dy = d / D - R, dx = d % D - R;
  return (cost << 18) | ((uint64_t)(dy * dy + dx * dx) << 10) | ((uint64_t)(dy + R) << 5) | (uint64_t)(dx + R);
}
static __device__ __forceinline__ uint64_t trec_wave_min(uint64_t k) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)k, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(k >> 32), o, 64);
    const uint64_t other = ((uint64_t)hi << 32) | lo;
    k = other < k ? other : k;
  }
  return k;
}

// the limits every entry point of the two schemes shares; on refusal `why` names the limit
static inline bool trec_shape_ok(int64_t samples, int64_t H, int64_t W, int64_t block, const char** why) {
  const char* w = nullptr;
  if (block != 8 && block != 16 && block != 32) w = "block must be 8, 16 or 32";
  else if (samples < 1 || samples > 65535) w = "samples must be in 1..65535";
  else if (H < 1 || W < 1 || H >= 32768 || W >= 32768) w = "H and W must be in [1, 32768)";
  else if (H * W >= (1ll << 24)) w = "pixels per frame < 2^24";
  if (why) *why = w;
  return w == nullptr;
}

// advect.hip.  Checks what adnm_trec_motion and adnm_trec_flow share (the frames, the limits, the workspace; `what` names the caller in the
// message) and launches trec_cost: ws[sample][block][(2R+1)^2 costs | echo count] uint32, adnm_trec_ws_bytes, every byte written.
int adnm_trec_cost_launch(const char* what, const float* prev, const float* last, int64_t sample_stride, float value_scale, int64_t block, int64_t radius,
                          int64_t echo, void* ws, int64_t ws_bytes, int64_t samples, int64_t H, int64_t W, hipStream_t st);
