// K1b — the chunked, bidirectional SSD scan of the `linear_attn_duality=False` branch
// (ADNssd.py:413-454, Vssd.py:245-275: mamba_ssm's mamba_chunk_scan_combined(x, dt, A, B, C, chunk_size, D, z=None),
// forward on one half of the heads, on the time-reversed sequence for the other half):
//
//     d_t = exp(dt_t * A_h),   S_t = d_t * S_{t-1} + dt_t * B_t (x) x_t,   y_t = C_t . S_t + D_h * x_t
//     dt = softplus(dt_raw + dt_bias),  A_h = -exp(A_log[h]),  head h reads K/Q group  h / (H/G)  (mamba_ssm convention)
//
// PARITY UNPINNED: the reference delegates this arithmetic to un-vendored mamba-ssm 2.2.2 Triton kernels; the oracle
// (oracle/adnm_oracle.py::ssd_chunk_scan) is a sequential fp64 restatement of the recurrence above.
//
// Chunked state-space-duality structure (three passes each way, all HBM streams):
//   1. per chunk (parallel): local end state  S_c = sum_t exp(a_end - a_t) dt_t B_t (x) x_t  and the chunk decay exp(a_end)
//   2. per (b,h,p) (sequential over the L/Q chunks — a few hundred steps of an N-float state): entering states S_in[c]
//   3. per chunk (parallel): replay the recurrence from S_in[c] and emit y.
// The state is only N x P (8..16 x 4) per head, so a lane owns the N-vector of one (head, p) column in registers and the
// intra-chunk work is a register recurrence rather than a Q x Q masked GEMM: at P = 4, N <= 16 the dense
// "attention-like" formulation would spend 2*Q*(N+P) flops per token on a contraction whose useful part is 2*N*P.
// Backward mirrors it in reverse time (gradient state R_t = C_t (x) dy_t + d_{t+1} R_{t+1}); the forward states needed
// by d(dt), dA are re-materialised per chunk into a scratch buffer (288 GB of HBM make that cheap) instead of inverting
// the recurrence (unstable: 1/d_t up to 5x per step).  All cross-thread sums are deterministic (no atomics).
#include "adnm_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int P = 4;

struct ScanArgs {
  const float *x, *Bm, *Cm, *dt_raw, *dt_bias, *A_log, *D;
  int64_t ldx, xhs, ldb, ldc, lddt, dths, phs;  // row strides, per-head strides (elements)
  int64_t L;
  int B, H, G, Q, NC, reverse;
};

__device__ __forceinline__ int64_t tok(const ScanArgs& a, int c, int t) {  // scan position -> token index
  const int64_t pos = (int64_t)c * a.Q + t;
  return a.reverse ? a.L - 1 - pos : pos;
}

// thread <-> (b, chunk, head, p): p fastest, then head, then chunk
__device__ __forceinline__ bool decode(const ScanArgs& a, int64_t gid, int& b, int& c, int& h, int& p) {
  const int64_t per_b = (int64_t)a.NC * a.H * P;
  if (gid >= per_b * a.B) return false;
  b = (int)(gid / per_b);
  int64_t r = gid - (int64_t)b * per_b;
  c = (int)(r / (a.H * P));
  r -= (int64_t)c * a.H * P;
  h = (int)(r / P);
  p = (int)(r - h * P);
  return true;
}

template <int N>
__global__ __launch_bounds__(kBlock) void scan_chunk_state_kernel(ScanArgs a, float* __restrict__ S_chunk, float* __restrict__ decay) {
  int b, c, h, p;
  if (!decode(a, (int64_t)blockIdx.x * kBlock + threadIdx.x, b, c, h, p)) return;
  const float A = -__expf(a.A_log[h * a.phs]), bias = a.dt_bias[h * a.phs];
  const int g = h / (a.H / a.G);
  float s[N];
#pragma unroll
  for (int n = 0; n < N; ++n) s[n] = 0.f;
  float acum = 0.f;
  const int tmax = (int)((a.L - (int64_t)c * a.Q) < a.Q ? (a.L - (int64_t)c * a.Q) : a.Q);
  for (int t = 0; t < tmax; ++t) {
    const int64_t row = (int64_t)b * a.L + tok(a, c, t);
    const float dtv = softplusf_(a.dt_raw[row * a.lddt + h * a.dths] + bias);
    const float d = __expf(dtv * A);
    const float xv = a.x[row * a.ldx + h * a.xhs + p] * dtv;
    const float* bp = a.Bm + row * a.ldb + g * N;
#pragma unroll
    for (int n = 0; n < N; ++n) s[n] = fmaf(d, s[n], bp[n] * xv);
    acum += dtv * A;
  }
  float* dst = S_chunk + ((((int64_t)b * a.H + h) * a.NC + c) * P + p) * N;
#pragma unroll
  for (int n = 0; n < N; ++n) dst[n] = s[n];
  if (p == 0) decay[((int64_t)b * a.H + h) * a.NC + c] = __expf(acum);
}

// forward: S_in[c] = state entering chunk c.   backward (REV): E[c] = gradient state entering chunk c from the future.
template <int N, bool REV>
__global__ __launch_bounds__(kBlock) void scan_carry_kernel(const float* __restrict__ S_chunk, const float* __restrict__ decay,
                                                            float* __restrict__ S_in, int BH, int NC) {
  const int gid = blockIdx.x * kBlock + threadIdx.x;
  if (gid >= BH * P) return;
  const int bh = gid / P, p = gid - bh * P;
  float s[N];
#pragma unroll
  for (int n = 0; n < N; ++n) s[n] = 0.f;
  for (int k = 0; k < NC; ++k) {
    const int c = REV ? NC - 1 - k : k;
    const int64_t off = (((int64_t)bh * NC + c) * P + p) * N;
    const float d = decay[(int64_t)bh * NC + c];
#pragma unroll
    for (int n = 0; n < N; ++n) {
      S_in[off + n] = s[n];
      s[n] = fmaf(d, s[n], S_chunk[off + n]);
    }
  }
}

template <int N>
__global__ __launch_bounds__(kBlock) void scan_output_kernel(ScanArgs a, const float* __restrict__ S_in, float* __restrict__ y, int64_t ldy,
                                                             int64_t yhs) {
  int b, c, h, p;
  if (!decode(a, (int64_t)blockIdx.x * kBlock + threadIdx.x, b, c, h, p)) return;
  const float A = -__expf(a.A_log[h * a.phs]), bias = a.dt_bias[h * a.phs], Dh = a.D[h * a.phs];
  const int g = h / (a.H / a.G);
  float s[N];
  const float* src = S_in + ((((int64_t)b * a.H + h) * a.NC + c) * P + p) * N;
#pragma unroll
  for (int n = 0; n < N; ++n) s[n] = src[n];
  const int tmax = (int)((a.L - (int64_t)c * a.Q) < a.Q ? (a.L - (int64_t)c * a.Q) : a.Q);
  for (int t = 0; t < tmax; ++t) {
    const int64_t row = (int64_t)b * a.L + tok(a, c, t);
    const float dtv = softplusf_(a.dt_raw[row * a.lddt + h * a.dths] + bias);
    const float d = __expf(dtv * A);
    const float xr = a.x[row * a.ldx + h * a.xhs + p];
    const float xv = xr * dtv;
    const float* bp = a.Bm + row * a.ldb + g * N;
    const float* cp = a.Cm + row * a.ldc + g * N;
    float o = Dh * xr;
#pragma unroll
    for (int n = 0; n < N; ++n) {
      s[n] = fmaf(d, s[n], bp[n] * xv);
      o = fmaf(cp[n], s[n], o);
    }
    y[row * ldy + h * yhs + p] = o;
  }
}

// backward pass 1: G_c = sum_t exp(a_t) C_t (x) dy_t   (a_t = inclusive cumulative log decay inside the chunk)
template <int N>
__global__ __launch_bounds__(kBlock) void scan_chunk_grad_kernel(ScanArgs a, const float* __restrict__ dy, int64_t lddy, int64_t dyhs,
                                                                 float* __restrict__ G_chunk) {
  int b, c, h, p;
  if (!decode(a, (int64_t)blockIdx.x * kBlock + threadIdx.x, b, c, h, p)) return;
  const float A = -__expf(a.A_log[h * a.phs]), bias = a.dt_bias[h * a.phs];
  const int g = h / (a.H / a.G);
  float s[N];
#pragma unroll
  for (int n = 0; n < N; ++n) s[n] = 0.f;
  float acum = 0.f;
  const int tmax = (int)((a.L - (int64_t)c * a.Q) < a.Q ? (a.L - (int64_t)c * a.Q) : a.Q);
  for (int t = 0; t < tmax; ++t) {
    const int64_t row = (int64_t)b * a.L + tok(a, c, t);
    acum += softplusf_(a.dt_raw[row * a.lddt + h * a.dths] + bias) * A;
    const float w = __expf(acum) * dy[row * lddy + h * dyhs + p];
    const float* cp = a.Cm + row * a.ldc + g * N;
#pragma unroll
    for (int n = 0; n < N; ++n) s[n] = fmaf(cp[n], w, s[n]);
  }
  float* dst = G_chunk + ((((int64_t)b * a.H + h) * a.NC + c) * P + p) * N;
#pragma unroll
  for (int n = 0; n < N; ++n) dst[n] = s[n];
}

// backward pass 3.  scratch: (B, L, H, P, N) forward states re-materialised by this same thread.
// per-head outputs: dBC_h (B*L, H, 2N) [summed over p here, over the heads of a group by the fold kernel],
// hpart (B*NC, H*P, 3) = per-thread [dD, ddt_bias, dA_log] partial sums.
template <int N>
__global__ __launch_bounds__(kBlock) void scan_bwd_kernel(ScanArgs a, const float* __restrict__ dy, int64_t lddy, int64_t dyhs,
                                                          const float* __restrict__ S_in, const float* __restrict__ E_in,
                                                          float* __restrict__ scratch, float* __restrict__ dx, int64_t lddx, int64_t dxhs,
                                                          float* __restrict__ ddt_raw, int64_t ldddt, int64_t ddths,
                                                          float* __restrict__ dBC_h, float* __restrict__ hpart) {
  int b, c, h, p;
  const bool live = decode(a, (int64_t)blockIdx.x * kBlock + threadIdx.x, b, c, h, p);
  // the p-lanes of a head are adjacent (p fastest) and blocks are multiples of 4 threads, so the xor-shuffles below stay
  // inside one (b, chunk, head); dead lanes only occur past the end of the grid, whole heads at a time.
  if (!live) return;
  const float A = -__expf(a.A_log[h * a.phs]), bias = a.dt_bias[h * a.phs], Dh = a.D[h * a.phs];
  const int g = h / (a.H / a.G);
  const int64_t soff = ((((int64_t)b * a.H + h) * a.NC + c) * P + p) * N;
  float s[N], r[N];
#pragma unroll
  for (int n = 0; n < N; ++n) s[n] = S_in[soff + n];
  const int tmax = (int)((a.L - (int64_t)c * a.Q) < a.Q ? (a.L - (int64_t)c * a.Q) : a.Q);
  // phase 1: replay forward, keep S_t (state AFTER token t) in scratch
  for (int t = 0; t < tmax; ++t) {
    const int64_t row = (int64_t)b * a.L + tok(a, c, t);
    const float dtv = softplusf_(a.dt_raw[row * a.lddt + h * a.dths] + bias);
    const float d = __expf(dtv * A);
    const float xv = a.x[row * a.ldx + h * a.xhs + p] * dtv;
    const float* bp = a.Bm + row * a.ldb + g * N;
    float* sp = scratch + ((row * a.H + h) * P + p) * N;
#pragma unroll
    for (int n = 0; n < N; ++n) {
      s[n] = fmaf(d, s[n], bp[n] * xv);
      sp[n] = s[n];
    }
  }
  // phase 2: reverse time
#pragma unroll
  for (int n = 0; n < N; ++n) r[n] = E_in[soff + n];  // gradient arriving from the chunks after this one
  float accD = 0.f, accB = 0.f, accA = 0.f;
  for (int t = tmax - 1; t >= 0; --t) {
    const int64_t row = (int64_t)b * a.L + tok(a, c, t);
    const float z = a.dt_raw[row * a.lddt + h * a.dths] + bias;
    const float dtv = softplusf_(z);
    const float d = __expf(dtv * A);
    const float xr = a.x[row * a.ldx + h * a.xhs + p];
    const float gy = dy[row * lddy + h * dyhs + p];
    const float* bp = a.Bm + row * a.ldb + g * N;
    const float* cp = a.Cm + row * a.ldc + g * N;
    const float* st = scratch + ((row * a.H + h) * P + p) * N;             // S_t
    float sprev[N];
    if (t > 0) {
      const int64_t rowp = (int64_t)b * a.L + tok(a, c, t - 1);
      const float* sp = scratch + ((rowp * a.H + h) * P + p) * N;
#pragma unroll
      for (int n = 0; n < N; ++n) sprev[n] = sp[n];
    } else {
#pragma unroll
      for (int n = 0; n < N; ++n) sprev[n] = S_in[soff + n];
    }
    float rb = 0.f, rs = 0.f, dBn[N], dCn[N];
#pragma unroll
    for (int n = 0; n < N; ++n) {
      r[n] = fmaf(cp[n], gy, r[n]);          // R_t = C_t (x) dy_t + d_{t+1} R_{t+1}
      rb = fmaf(r[n], bp[n], rb);            // sum_n R[n] B[n]
      rs = fmaf(r[n], sprev[n], rs);         // sum_n R[n] S_{t-1}[n]
      dBn[n] = r[n] * xr * dtv;              // dB_t[n] (this p)
      dCn[n] = gy * st[n];                   // dC_t[n] (this p)
    }
    dx[row * lddx + h * dxhs + p] = fmaf(dtv, rb, Dh * gy);
    // d(dt_t) = sum_p [ rb * x + rs * A * d ];   dA += sum_p rs * dt * d
    float ddt = rb * xr + rs * A * d;
    float dAh = rs * dtv * d;
    ddt += __shfl_xor(ddt, 1, 64); ddt += __shfl_xor(ddt, 2, 64);
    accA += dAh;
    accD = fmaf(gy, xr, accD);
    const float dz = ddt * sigmoidf_(z);
    if (p == 0) {
      ddt_raw[row * ldddt + h * ddths] = dz;
      accB += dz;
    }
    // sum the P lanes of this head, lane p==0 writes the per-head dB/dC row
#pragma unroll
    for (int n = 0; n < N; ++n) {
      dBn[n] += __shfl_xor(dBn[n], 1, 64); dBn[n] += __shfl_xor(dBn[n], 2, 64);
      dCn[n] += __shfl_xor(dCn[n], 1, 64); dCn[n] += __shfl_xor(dCn[n], 2, 64);
    }
    if (p == 0) {
      float* o = dBC_h + (row * a.H + h) * (2 * N);
#pragma unroll
      for (int n = 0; n < N; ++n) { o[n] = dBn[n]; o[N + n] = dCn[n]; }
    }
#pragma unroll
    for (int n = 0; n < N; ++n) r[n] *= d;   // carry to token t-1
  }
  float* hp = hpart + ((((int64_t)b * a.NC + c) * a.H + h) * P + p) * 3;
  hp[0] = accD; hp[1] = accB; hp[2] = accA * A;  // dA_log = dA * A  (A = -exp(A_log))
}

// dB[row, g, n] = sum_{h in group g} dBC_h[row, h, n]   (and dC likewise)
__global__ void scan_bc_fold_kernel(const float* __restrict__ dBC_h, int64_t rows, int H, int G, int N, float* __restrict__ dBm, int64_t lddb,
                                    float* __restrict__ dCm, int64_t lddc) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int per = 2 * G * N;
  if (i >= rows * per) return;
  const int64_t row = i / per;
  int k = (int)(i - row * per);
  const int isC = k >= G * N;
  if (isC) k -= G * N;
  const int g = k / N, n = k - g * N, hpg = H / G;
  float t = 0.f;
  for (int hh = 0; hh < hpg; ++hh) t += dBC_h[(row * H + g * hpg + hh) * (2 * N) + isC * N + n];
  (isC ? dCm + row * lddc : dBm + row * lddb)[g * N + n] = t;
}

// out[j][h] = sum over (b, chunk, p) of hpart[(b,c), h, p, j]
__global__ void scan_head_fold_kernel(const float* __restrict__ hpart, int BNC, int H, float* __restrict__ dD, float* __restrict__ ddt_bias,
                                      float* __restrict__ dA_log) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * H) return;
  const int j = i / H, h = i - j * H;
  float t = 0.f;
  for (int k = 0; k < BNC; ++k)
#pragma unroll
    for (int p = 0; p < P; ++p) t += hpart[(((int64_t)k * H + h) * P + p) * 3 + j];
  (j == 0 ? dD : j == 1 ? ddt_bias : dA_log)[h] = t;
}

struct ScanWs {
  float *S_chunk, *decay, *G_chunk, *E_in, *scratch, *dBC_h, *hpart;
  int64_t bytes;
};
ScanWs carve(void* ws, int64_t B, int64_t L, int64_t H, int64_t N, int64_t NC, bool bwd) {
  ScanWs w{};
  int64_t off = 0;
  auto take = [&](int64_t nf) {
    float* p = ws ? (float*)((char*)ws + off) : nullptr;
    off += adnm_align(nf * 4, 256);
    return p;
  };
  w.S_chunk = take(B * H * NC * P * N);
  w.decay = take(B * H * NC);
  if (bwd) {
    w.G_chunk = take(B * H * NC * P * N);
    w.E_in = take(B * H * NC * P * N);
    w.scratch = take(B * L * H * P * N);
    w.dBC_h = take(B * L * H * 2 * N);
    w.hpart = take(B * NC * H * P * 3);
  }
  w.bytes = off;
  return w;
}

int check(const char* who, int64_t B, int64_t L, int64_t H, int64_t Pp, int64_t N, int64_t G, int64_t Q, int dtype) {
  ADNM_REQUIRE(B > 0 && L > 0 && H > 0 && Q > 0, "%s: empty shape", who);
  ADNM_REQUIRE(Pp == 4 && (N == 8 || N == 16), "%s: (headdim, states per group) = (%lld, %lld) not in {(4,8),(4,16)}", who, (long long)Pp, (long long)N);
  ADNM_REQUIRE(G >= 1 && H % G == 0, "%s: heads %lld not divisible by groups %lld", who, (long long)H, (long long)G);
  ADNM_REQUIRE(dtype == ADNM_F32, "%s: the scan path is fp32 only", who);
  return ADNM_OK;
}

ScanArgs make_args(const void* x, int64_t ldx, int64_t xhs, const void* Bm, int64_t ldb, const void* Cm, int64_t ldc, const void* dt_raw,
                   int64_t lddt, int64_t dths, const float* dt_bias, const float* A_log, const float* D, int64_t phs, int64_t B, int64_t L,
                   int64_t H, int64_t G, int64_t Q, int reverse) {
  ScanArgs a;
  a.x = (const float*)x; a.Bm = (const float*)Bm; a.Cm = (const float*)Cm; a.dt_raw = (const float*)dt_raw;
  a.dt_bias = dt_bias; a.A_log = A_log; a.D = D;
  a.ldx = ldx; a.xhs = xhs; a.ldb = ldb; a.ldc = ldc; a.lddt = lddt; a.dths = dths; a.phs = phs;
  a.L = L; a.B = (int)B; a.H = (int)H; a.G = (int)G; a.Q = (int)Q; a.NC = (int)adnm_cdiv(L, Q); a.reverse = reverse;
  return a;
}

}  // namespace

extern "C" int64_t adnm_ssd_scan_ws_bytes(int64_t B, int64_t L, int64_t H, int64_t N, int64_t chunk, int backward) {
  if (B <= 0 || L <= 0 || H <= 0 || chunk <= 0) return 0;
  return carve(nullptr, B, L, H, N, adnm_cdiv(L, chunk), backward != 0).bytes;
}

extern "C" int adnm_ssd_scan_fwd(const void* x, int64_t ldx, int64_t x_hstride, const void* Bm, int64_t ldb, const void* Cm, int64_t ldc,
                                 const void* dt_raw, int64_t lddt, int64_t dt_hstride, const float* dt_bias, const float* A_log, const float* D,
                                 int64_t p_hstride, void* y, int64_t ldy, int64_t y_hstride, float* S_in, void* ws, int64_t ws_bytes, int64_t B,
                                 int64_t L, int64_t H, int64_t Pp, int64_t N, int64_t G, int64_t chunk, int reverse, int dtype,
                                 adnm_stream_t stream) {
  if (int rc = check("ssd_scan_fwd", B, L, H, Pp, N, G, chunk, dtype)) return rc;
  ADNM_REQUIRE(x && Bm && Cm && dt_raw && dt_bias && A_log && D && y && S_in, "ssd_scan_fwd: null pointer");
  ADNM_REQUIRE(x_hstride >= Pp && y_hstride >= Pp && dt_hstride >= 1 && p_hstride >= 1, "ssd_scan_fwd: head strides smaller than a head");
  ADNM_REQUIRE(ldx >= (H - 1) * x_hstride + Pp && ldy >= (H - 1) * y_hstride + Pp && lddt >= (H - 1) * dt_hstride + 1 && ldb >= G * N && ldc >= G * N,
               "ssd_scan_fwd: row strides smaller than the rows they address");
  const int64_t NC = adnm_cdiv(L, chunk);
  const ScanWs w = carve(ws, B, L, H, N, NC, false);
  if (!ws || ws_bytes < w.bytes) {
    adnm_set_error("ssd_scan_fwd: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)w.bytes);
    return ADNM_EWORKSPACE;
  }
  const ScanArgs a = make_args(x, ldx, x_hstride, Bm, ldb, Cm, ldc, dt_raw, lddt, dt_hstride, dt_bias, A_log, D, p_hstride, B, L, H, G, chunk, reverse);
  hipStream_t st = (hipStream_t)stream;
  const int64_t threads = B * NC * H * P;
  const unsigned grid = (unsigned)adnm_cdiv(threads, kBlock), gridc = (unsigned)adnm_cdiv(B * H * P, kBlock);
  const double tokbytes = 4.0 * B * L * (H * P + 2.0 * G * N + H);
  if (N == 8) {
    { ADNM_PROF("ssd_scan_chunk_state", st, tokbytes); scan_chunk_state_kernel<8><<<grid, kBlock, 0, st>>>(a, w.S_chunk, w.decay); }
    { ADNM_PROF("ssd_scan_carry", st, 8.0 * B * H * NC * P * N); scan_carry_kernel<8, false><<<gridc, kBlock, 0, st>>>(w.S_chunk, w.decay, S_in, (int)(B * H), (int)NC); }
    { ADNM_PROF("ssd_scan_output", st, tokbytes + 4.0 * B * L * H * P); scan_output_kernel<8><<<grid, kBlock, 0, st>>>(a, S_in, (float*)y, ldy, y_hstride); }
  } else {
    { ADNM_PROF("ssd_scan_chunk_state", st, tokbytes); scan_chunk_state_kernel<16><<<grid, kBlock, 0, st>>>(a, w.S_chunk, w.decay); }
    { ADNM_PROF("ssd_scan_carry", st, 8.0 * B * H * NC * P * N); scan_carry_kernel<16, false><<<gridc, kBlock, 0, st>>>(w.S_chunk, w.decay, S_in, (int)(B * H), (int)NC); }
    { ADNM_PROF("ssd_scan_output", st, tokbytes + 4.0 * B * L * H * P); scan_output_kernel<16><<<grid, kBlock, 0, st>>>(a, S_in, (float*)y, ldy, y_hstride); }
  }
  ADNM_CHECK_LAUNCH("ssd_scan_fwd");
  return ADNM_OK;
}

extern "C" int adnm_ssd_scan_bwd(const void* dy, int64_t lddy, int64_t dy_hstride, const void* x, int64_t ldx, int64_t x_hstride, const void* Bm,
                                 int64_t ldb, const void* Cm, int64_t ldc, const void* dt_raw, int64_t lddt, int64_t dt_hstride,
                                 const float* dt_bias, const float* A_log, const float* D, int64_t p_hstride, const float* S_in, void* dx,
                                 int64_t lddx, int64_t dx_hstride, void* dBm, int64_t lddb, void* dCm, int64_t lddc, void* ddt_raw, int64_t ldddt,
                                 int64_t ddt_hstride, float* ddt_bias, float* dA_log, float* dD, void* ws, int64_t ws_bytes, int64_t B, int64_t L,
                                 int64_t H, int64_t Pp, int64_t N, int64_t G, int64_t chunk, int reverse, int dtype, adnm_stream_t stream) {
  if (int rc = check("ssd_scan_bwd", B, L, H, Pp, N, G, chunk, dtype)) return rc;
  ADNM_REQUIRE(dy && x && Bm && Cm && dt_raw && dt_bias && A_log && D && S_in && dx && dBm && dCm && ddt_raw && ddt_bias && dA_log && dD,
               "ssd_scan_bwd: null pointer");
  ADNM_REQUIRE(x_hstride >= Pp && dy_hstride >= Pp && dx_hstride >= Pp && dt_hstride >= 1 && ddt_hstride >= 1 && p_hstride >= 1,
               "ssd_scan_bwd: head strides smaller than a head");
  ADNM_REQUIRE(ldx >= (H - 1) * x_hstride + Pp && lddy >= (H - 1) * dy_hstride + Pp && lddx >= (H - 1) * dx_hstride + Pp &&
                   lddt >= (H - 1) * dt_hstride + 1 && ldddt >= (H - 1) * ddt_hstride + 1 && ldb >= G * N && ldc >= G * N && lddb >= G * N && lddc >= G * N,
               "ssd_scan_bwd: row strides smaller than the rows they address");
  const int64_t NC = adnm_cdiv(L, chunk);
  const ScanWs w = carve(ws, B, L, H, N, NC, true);
  if (!ws || ws_bytes < w.bytes) {
    adnm_set_error("ssd_scan_bwd: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)w.bytes);
    return ADNM_EWORKSPACE;
  }
  const ScanArgs a = make_args(x, ldx, x_hstride, Bm, ldb, Cm, ldc, dt_raw, lddt, dt_hstride, dt_bias, A_log, D, p_hstride, B, L, H, G, chunk, reverse);
  hipStream_t st = (hipStream_t)stream;
  const int64_t threads = B * NC * H * P;
  const unsigned grid = (unsigned)adnm_cdiv(threads, kBlock), gridc = (unsigned)adnm_cdiv(B * H * P, kBlock);
  const double tokbytes = 4.0 * B * L * (2.0 * H * P + 2.0 * G * N + H);
#define SCAN_BWD(NN)                                                                                                                     \
  { ADNM_PROF("ssd_scan_chunk_grad", st, tokbytes); scan_chunk_grad_kernel<NN><<<grid, kBlock, 0, st>>>(a, (const float*)dy, lddy, dy_hstride, w.G_chunk); } \
  { /* the decays are recomputed by the state kernel into the workspace (cheap) */                                                       \
    ADNM_PROF("ssd_scan_chunk_state", st, tokbytes); scan_chunk_state_kernel<NN><<<grid, kBlock, 0, st>>>(a, w.S_chunk, w.decay); }       \
  { ADNM_PROF("ssd_scan_carry", st, 8.0 * B * H * NC * P * N); scan_carry_kernel<NN, true><<<gridc, kBlock, 0, st>>>(w.G_chunk, w.decay, w.E_in, (int)(B * H), (int)NC); } \
  { ADNM_PROF("ssd_scan_bwd", st, tokbytes * 2 + 8.0 * B * L * H * P * N);                                                                \
    scan_bwd_kernel<NN><<<grid, kBlock, 0, st>>>(a, (const float*)dy, lddy, dy_hstride, S_in, w.E_in, w.scratch, (float*)dx, lddx, dx_hstride, (float*)ddt_raw, ldddt, ddt_hstride, w.dBC_h, w.hpart); }
  if (N == 8) { SCAN_BWD(8) } else { SCAN_BWD(16) }
#undef SCAN_BWD
  const int64_t tot = B * L * 2 * G * N;
  scan_bc_fold_kernel<<<(unsigned)adnm_cdiv(tot, 256), 256, 0, st>>>(w.dBC_h, B * L, (int)H, (int)G, (int)N, (float*)dBm, lddb, (float*)dCm, lddc);
  scan_head_fold_kernel<<<(unsigned)adnm_cdiv(3 * H, 256), 256, 0, st>>>(w.hpart, (int)(B * NC), (int)H, dD, ddt_bias, dA_log);
  ADNM_CHECK_LAUNCH("ssd_scan_bwd");
  return ADNM_OK;
}
