// Exponential moving average of the flat fp32 parameter buffer (FlatTrainer(ema_decay=...)) and the exchange that lets the model compute
// with it (FlatTrainer.ema_weights()).  Two streaming passes over flat buffers: n > 0, n % 4 == 0, 16-byte aligned, p and ema disjoint.
// HBM-bound: the update moves 12 B per parameter (read p, read and write ema), the swap 16 B.
// Not fused into the AdamW pass (optim.hip): that would save the 4 B read of p, and change a kernel whose bits the tests pin.
#include "adnm_common.h"

namespace {
constexpr int kBlock = 256;
constexpr int kMaxBlocks = 2048;   // 8 workgroups of 256 lanes per CU on 256 CUs: every wave slot of the chip; the rest by grid stride
constexpr int kQuads = 2;          // float4 per lane, stream and trip: both trips' loads are issued before the first use

// d = warmup ? min(decay, (1 + t) / (10 + t)) : decay with t = state[0], the device's own step counter AFTER the optimiser pass of this
// step: a captured launch follows the counter, a skipped step (the counter stands still) included.  w = 1 - d is exact for d >= 0.5.
// ema[i] = fmaf(d, ema[i], w * p[i]): the product and the fma round once each, whatever the contraction mode.
// info[0] = d, info[1] += 1: lane 0 of workgroup 0, ordinary stores.
// GUARD: one uniform load and branch at entry (adamw_kernel's pattern): a skipped step writes neither ema nor info.
// ema is read and written once per step and not looked at in between: non-temporal; p was just written by the optimiser pass.
template <bool GUARD>
__global__ __launch_bounds__(kBlock) void ema_update_kernel(const float* __restrict__ p, float* __restrict__ ema, int64_t n4,
                                                            const float* __restrict__ state, float decay, int warmup, float* __restrict__ info,
                                                            const AdnmStepStats* __restrict__ stats) {
#pragma clang fp contract(off)
  if (GUARD && stats->skip) return;
  float d = decay;
  if (warmup) {
    const float t = state[0];
    d = fminf(decay, (1.0f + t) / (10.0f + t));
  }
  const float w = 1.0f - d;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    info[0] = d;
    info[1] = info[1] + 1.0f;
  }
  using f4 = __attribute__((ext_vector_type(4))) float;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i0 < n4; i0 += kQuads * stride) {
    f4 pp[kQuads], ee[kQuads];
#pragma unroll
    for (int u = 0; u < kQuads; ++u) {   // every load of the trip first
      const int64_t i = i0 + u * stride;
      if (i < n4) {
        pp[u] = reinterpret_cast<const f4*>(p)[i];
        ee[u] = __builtin_nontemporal_load(reinterpret_cast<const f4*>(ema) + i);
      }
    }
#pragma unroll
    for (int u = 0; u < kQuads; ++u) {
      const int64_t i = i0 + u * stride;
      if (i >= n4) break;
#pragma unroll
      for (int k = 0; k < 4; ++k) ee[u][k] = fmaf(d, ee[u][k], w * pp[u][k]);
      __builtin_nontemporal_store(ee[u], reinterpret_cast<f4*>(ema) + i);
    }
  }
}

// the two buffers exchange their contents as bit patterns (integer quads: a NaN keeps its payload), each quad read from both sides
// before either is written; no temporary buffer
__global__ __launch_bounds__(kBlock) void ema_swap_kernel(float* __restrict__ p, float* __restrict__ ema, int64_t n4) {
  using u4 = __attribute__((ext_vector_type(4))) unsigned int;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i0 < n4; i0 += kQuads * stride) {
    u4 pp[kQuads], ee[kQuads];
#pragma unroll
    for (int u = 0; u < kQuads; ++u) {
      const int64_t i = i0 + u * stride;
      if (i < n4) {
        pp[u] = reinterpret_cast<const u4*>(p)[i];
        ee[u] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(ema) + i);
      }
    }
#pragma unroll
    for (int u = 0; u < kQuads; ++u) {
      const int64_t i = i0 + u * stride;
      if (i >= n4) break;
      reinterpret_cast<u4*>(p)[i] = ee[u];   // (plain: the next forward reads p)
      __builtin_nontemporal_store(pp[u], reinterpret_cast<u4*>(ema) + i);
    }
  }
}

// one full pass of the grid covers kMaxBlocks * kBlock * kQuads quads
int64_t ema_blocks(int64_t n4) {
  int64_t blocks = adnm_cdiv(n4, (int64_t)kBlock * kQuads);
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  return blocks < 1 ? 1 : blocks;
}
bool overlap(const float* a, const float* b, int64_t n) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, bytes = (uintptr_t)n * 4;
  return x < y + bytes && y < x + bytes;
}
}  // namespace

extern "C" int adnm_ema_update(const float* p, float* ema, int64_t n, const float* state, float decay, int warmup, float* info,
                               const void* stats, adnm_stream_t stream) {
  ADNM_REQUIRE(p && ema && state && info, "ema_update: null pointer");
  ADNM_REQUIRE(n > 0 && n % 4 == 0, "ema_update: n=%lld must be a positive multiple of 4 (the flat layout pads every tensor)", (long long)n);
  ADNM_REQUIRE(((uintptr_t)p | (uintptr_t)ema) % 16 == 0, "ema_update: p and ema must be 16-byte aligned");
  ADNM_REQUIRE(((uintptr_t)state | (uintptr_t)info) % 4 == 0 && (uintptr_t)stats % 8 == 0,
               "ema_update: state and info must be 4-byte aligned, the statistics block 8-byte aligned");
  ADNM_REQUIRE(!overlap(p, ema, n), "ema_update: p and ema overlap");
  ADNM_REQUIRE(decay >= 0.0f && decay <= 1.0f, "ema_update: decay=%g must lie in [0, 1]", (double)decay);
  hipStream_t st = (hipStream_t)stream;
  const int64_t n4 = n / 4, blocks = ema_blocks(n4);
  ADNM_PROF("ema_update", st, 12.0 * n);
  if (stats) ema_update_kernel<true><<<(unsigned)blocks, kBlock, 0, st>>>(p, ema, n4, state, decay, warmup, info, (const AdnmStepStats*)stats);
  else ema_update_kernel<false><<<(unsigned)blocks, kBlock, 0, st>>>(p, ema, n4, state, decay, warmup, info, nullptr);
  ADNM_CHECK_LAUNCH("ema_update");
  return ADNM_OK;
}

extern "C" int adnm_ema_swap(float* p, float* ema, int64_t n, adnm_stream_t stream) {
  ADNM_REQUIRE(p && ema, "ema_swap: null pointer");
  ADNM_REQUIRE(n > 0 && n % 4 == 0, "ema_swap: n=%lld must be a positive multiple of 4 (the flat layout pads every tensor)", (long long)n);
  ADNM_REQUIRE(((uintptr_t)p | (uintptr_t)ema) % 16 == 0, "ema_swap: p and ema must be 16-byte aligned");
  ADNM_REQUIRE(!overlap(p, ema, n), "ema_swap: p and ema overlap");
  hipStream_t st = (hipStream_t)stream;
  const int64_t n4 = n / 4, blocks = ema_blocks(n4);
  ADNM_PROF("ema_swap", st, 16.0 * n);
  ema_swap_kernel<<<(unsigned)blocks, kBlock, 0, st>>>(p, ema, n4);
  ADNM_CHECK_LAUNCH("ema_swap");
  return ADNM_OK;
}
