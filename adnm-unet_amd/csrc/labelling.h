// Connected-component labelling of one frame's event bits by one workgroup: the device code objects.hip (the object scores)
// and sal.hip (the per-object intensity moments) share.  Every lane of a workgroup of kBlock lanes calls these together.
//
//   the bits        one event bit per pixel (a ballot per 64 pixels).  Everything after staging reads bits, never floats.
//   the words       one u32 per pixel, in LDS or in the workgroup's slice of a workspace.  While labelling, an event pixel's word is its
//                   parent: the index of a pixel of the same object that is not larger than its own.  A word only ever decreases.
//   runs            a pixel starts with the first pixel of its horizontal run of events as parent (bit scans, no memory traffic), so
//                   the left neighbour needs no union.
//   unions          label equivalence: union-find with atomicMin links and pointer jumping (Komura 2015; Playne & Hawick 2018).  A pixel
//                   unites with the row above only where no neighbour makes the same union: with N unless W and NW are events; else with
//                   NW unless W is an event and with NE unless E is.  A union finds both roots, links the larger to the smaller with an
//                   atomicMin and, where another lane was faster, goes on from the value it displaced.  ONE sweep of unions is complete
//                   whatever the shape (a serpentine included); a find is bounded by H * W steps (parents decrease strictly), a union by
//                   H * W retries, and a union that ran out raises a flag that repeats the sweep, itself at most H * W times.
//   areas           after a flattening pass every event pixel points at its root, the smallest index of the object.  Roots then become
//                   counters (kRoot | area, kMatched in the top bit): the first pixel of each run adds the run's length and ors the flag
//                   in when the OTHER field has an event inside the run.
#pragma once
#include "scored_pair.h"

namespace {
constexpr int kBlock = 1024;
constexpr unsigned kRoot = 1u << 30, kMatched = 1u << 31, kAreaMask = (1u << 20) - 1u;

__device__ __forceinline__ unsigned ld(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(unsigned* p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ bool bit(const unsigned* bits, int p) { return (bits[p >> 5] >> (p & 31)) & 1u; }

// words of one field's bits: whole ballots of 64 pixels
__host__ __device__ __forceinline__ int bit_words(int hw) { return 2 * ((hw + 63) / 64); }

// one event bit per pixel; every word of bits[0 .. bit_words(hw)) is written, pixels past hw as 0
__device__ __forceinline__ void stage_bits(unsigned* bits, const float* __restrict__ src, int hw, float thr, float value_scale) {
  const int lane = threadIdx.x & 63, span = bit_words(hw) * 32;
  for (int base = (threadIdx.x >> 6) * 64; base < span; base += kBlock) {
    const int p = base + lane;
    const bool ev = p < hw && eval_trunc(eval_scaled(src[p], value_scale)) >= thr;
    const unsigned long long m = __ballot(ev);
    if (lane == 0) bits[base >> 5] = (unsigned)m, bits[(base >> 5) + 1] = (unsigned)(m >> 32);
  }
}

// the first pixel of the run of events that holds p (bit p is set), not left of row0.  At most W / 32 + 1 words are looked at.
__device__ __forceinline__ int run_start(const unsigned* bits, int p, int row0) {
  int w = p >> 5;
  unsigned zeros = ~bits[w] & ((2u << (p & 31)) - 1u);   // the non-events at or below p in its word
  while (zeros == 0u) {
    if ((w << 5) <= row0) return row0;
    zeros = ~bits[--w];
  }
  const int s = (w << 5) + 32 - __clz((int)zeros);
  return s > row0 ? s : row0;
}
// one past the last pixel of that run, not right of row1 = the row's end.  Bits past H * W are 0, so no word past the array is read.
__device__ __forceinline__ int run_end(const unsigned* bits, int p, int row1) {
  int w = p >> 5;
  unsigned zeros = ~bits[w] & ~((2u << (p & 31)) - 1u);  // the non-events above p in its word
  while (zeros == 0u) {
    if (((++w) << 5) >= row1) return row1;
    zeros = ~bits[w];
  }
  const int e = (w << 5) + __ffs((int)zeros) - 1;
  return e < row1 ? e : row1;
}
// does bits hold an event in [s, e)?  s < e
__device__ __forceinline__ bool any_bit(const unsigned* bits, int s, int e) {
  const int w0 = s >> 5, w1 = (e - 1) >> 5;
  for (int w = w0; w <= w1; ++w) {
    unsigned m = bits[w];
    if (w == w0) m &= ~0u << (s & 31);
    if (w == w1) m &= ~0u >> (31 - ((e - 1) & 31));
    if (m) return true;
  }
  return false;
}

// the root above x as far as `bound` steps reach (parents decrease strictly: hw steps reach every root); x's word jumps to it
__device__ __forceinline__ unsigned find_root(unsigned* word, unsigned x, int bound) {
  const unsigned first = ld(word + x);
  unsigned r = x, p = first;
  for (int i = 0; p != r && i < bound; ++i) r = p, p = ld(word + r);
  if (r != first) atomicMin(word + x, r);
  return r;
}
// a and b are pixels of one object: afterwards they have one root.  false: gave up after `bound` lost races (the sweep is then repeated)
__device__ __forceinline__ bool unite(unsigned* word, unsigned a, unsigned b, int bound) {
  for (int i = 0; i < bound; ++i) {
    a = find_root(word, a, bound), b = find_root(word, b, bound);
    if (a == b) return true;
    if (a < b) {
      const unsigned t = a;
      a = b, b = t;
    }
    const unsigned old = atomicMin(word + a, b);   // a > b: hang a below b
    if (old == a) return true;
    a = old;   // another lane had linked a already, and that link may be gone now: go on with what it pointed at
  }
  return false;
}

// bits -> word[p] = kRoot | area (| kMatched) for the first pixel p of every object, the index of that pixel for the object's other pixels,
// 0 for non-events.  other: the other field's bits, or nullptr.  Every lane of the workgroup calls it.
__device__ __forceinline__ void label_field(unsigned* word, const unsigned* bits, const unsigned* other, unsigned* flag, int hw, int W) {
  const int tid = threadIdx.x;
  for (int p = tid; p < hw; p += kBlock) st(word + p, bit(bits, p) ? (unsigned)run_start(bits, p, p - p % W) : 0u);
  for (int sweep = 0; sweep < hw; ++sweep) {   // one sweep unless a union gave up
    __syncthreads();
    if (tid == 0) *flag = 0u;
    __syncthreads();
    bool ok = true;
    for (int p = tid + W; p < hw; p += kBlock) {
      if (!bit(bits, p)) continue;
      const int x = p % W, up = p - W;
      const bool l = x > 0, r = x + 1 < W;
      const bool n = bit(bits, up), w = l && bit(bits, p - 1), e = r && bit(bits, p + 1), nw = l && bit(bits, up - 1), ne = r && bit(bits, up + 1);
      if (n) {
        if (!(w && nw)) ok &= unite(word, p, up, hw);
      } else {
        if (nw && !w) ok &= unite(word, p, up - 1, hw);
        if (ne && !e) ok &= unite(word, p, up + 1, hw);
      }
    }
    if (!ok) *flag = 1u;
    __syncthreads();
    if (*flag == 0u) break;
  }
  for (int p = tid; p < hw; p += kBlock)
    if (bit(bits, p)) find_root(word, p, hw);   // the forest is final: every event's word becomes its root
  __syncthreads();
  for (int p = tid; p < hw; p += kBlock)
    if (bit(bits, p) && ld(word + p) == (unsigned)p) st(word + p, kRoot);
  __syncthreads();
  for (int p = tid; p < hw; p += kBlock) {
    const int row0 = p - p % W;
    if (!bit(bits, p) || (p > row0 && bit(bits, p - 1))) continue;   // the first pixel of a run speaks for the run
    const int e = run_end(bits, p, row0 + W);
    const unsigned wd = ld(word + p), root = (wd & kRoot) ? (unsigned)p : wd;
    atomicAdd(word + root, (unsigned)(e - p));
    if (other && any_bit(other, p, e)) atomicOr(word + root, kMatched);
  }
  __syncthreads();
}
}  // namespace
