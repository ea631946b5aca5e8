// The double-oracle level sampler's game solver (environments/nash_sampler.py:39-58 get_nash over
// util/projection.py:9-37 projection_simplex).
//
//  k_project_simplex  Euclidean projection of x[:nz] onto the unit simplex, one workgroup per row, without a sort:
//                     Newton's iteration on f(tau) = sum_j max(v_j - tau, 0) - 1 (Michelot's algorithm).  From
//                     tau = (sum_all v - 1) / nz it repeats tau = (sum_{v > tau} v - 1) / #{v > tau}; f is convex and
//                     piecewise linear, so the iterates rise monotonically to the root and the support set shrinks
//                     until it repeats -- then tau is the threshold of the reference's sorted-cumsum form, whose
//                     result is unique (no tie order enters).  Sums in f64 in a fixed order; out = max(v - tau, 0)
//                     rounded to f32 once.
//  k_nash<BP>         get_nash for one game per workgroup, every iteration inside the launch.  The workgroup has an x
//                     side and a y side of 2 BP threads each (BP = B rounded up to 8, 16, 32, 64, 128): two threads
//                     per strategy entry e, thread (e, h) holding in registers the 4-column chunks c = h (mod 2) of
//                     row e of M (x side) or of column e (y side).  An iteration is, on both sides at once,
//                       1. the matrix-vector product against the other side's strategy, read from LDS as 16-byte
//                          broadcasts (a wave reads two addresses 32 bytes apart: no bank conflict), the two halves
//                          added across the lane pair; v = x -+ lr g goes to LDS, -inf at index >= nz;
//                       2. the projection in its sort-free form: e is in the support iff sum_j max(v_j - v_e, 0) < 1
//                          (the reference's 1/k + v_(k) - cumsum_k/k > 0 rearranged), B/2 broadcast LDS reads per
//                          thread; k and sum_support v by a ballot and an f64 wave sum (and, with more than one wave
//                          per side, per-wave partials in LDS added in wave order);
//                       3. x' = max(v - tau, 0), tau = (sum_support v - 1) / k, into LDS for the other side, and
//                          into the thread's running sum.
//                     Everything is f64 (the f32 payoff is widened once, into registers; f64 VALU runs at the
//                     unpacked f32 rate here).  An f32 iterate does not hold 1e-6 against the float64 iteration: while
//                     a strategy drifts under a constant gradient every step adds the same rounding error of
//                     x + c, up to half an ulp, and 1000 steps of it came to 1e-5.
//                     x and y are double-buffered by iteration parity, so the only barrier between the sides is the
//                     one that ends an iteration; with more than one wave per side two more order the side's own
//                     exchanges.  No global access, no atomics: bit-identical from run to run.
#include "wave_dev.h"

namespace {

constexpr int kNashMaxB = 128;
constexpr int kNashMaxIters = 1000000;
constexpr int kProjMaxB = 8192;

// A DPP move of both halves of a double (patterns whose every source lane is valid, as dpp_u)
template <int CTRL>
TOUED_DEV double dpp_f64(double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = dpp_u<CTRL>((uint32_t)b), hi = dpp_u<CTRL>((uint32_t)(b >> 32));
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// wsum_dpp for doubles: the xor butterfly's additions in its order, every lane gets the sum, no LDS-crossbar permute
// but the xor-16 swizzle (six dependent ds_bpermute pairs were most of a small game's iteration).  All 64 lanes active.
TOUED_DEV double wave_sum_f64(double v) {
  v += dpp_f64<0xB1>(v);    // xor 1
  v += dpp_f64<0x4E>(v);    // xor 2
  v += dpp_f64<0x141>(v);   // row_half_mirror: the other quad of the 8
  v += dpp_f64<0x140>(v);   // row_mirror: the other 8 of the row
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_swizzle((int)(uint32_t)b, 0x401F);           // xor 16
  const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_swizzle((int)(uint32_t)(b >> 32), 0x401F);
  v += __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
  const uint64_t c = __builtin_bit_cast(uint64_t, v);
  const uint32_t l0 = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)c, 0);
  const uint32_t h0 = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(c >> 32), 0);
  const uint32_t l1 = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)c, 32);
  const uint32_t h1 = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(c >> 32), 32);
  return __builtin_bit_cast(double, ((uint64_t)h0 << 32) | l0) + __builtin_bit_cast(double, ((uint64_t)h1 << 32) | l1);
}

TOUED_DEV int wave_sum_i32(int v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

TOUED_DEV int clamp_nz(int n, int B) { return n < 1 ? 1 : (n > B ? B : n); }

// ------------------------------------------------------------------------------------------------ projection
// Block sum of (c, s), every thread gets both: wave butterflies, then the per-wave partials in wave order.  `buf`
// alternates between calls, so one barrier per call is enough (a wave can be at most one call ahead of another).
TOUED_DEV void block_sum(int& c, double& s, int buf, int (*pc)[16], double (*ps)[16], int lane, int wv, int nw) {
  c = wave_sum_i32(c);
  s = wave_sum_f64(s);
  if (lane == 0) { pc[buf][wv] = c; ps[buf][wv] = s; }
  __syncthreads();
  c = 0; s = 0.0;
  for (int w = 0; w < nw; ++w) { c += pc[buf][w]; s += ps[buf][w]; }
}

__global__ void __launch_bounds__(1024) k_project_simplex(const float* __restrict__ x, const int* __restrict__ nz,
                                                          int B, float* __restrict__ out) {
  __shared__ float sv[kProjMaxB];
  __shared__ int pc[2][16];
  __shared__ double ps[2][16];
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wv = tid >> 6, nw = nt >> 6;
  const size_t row = (size_t)blockIdx.x * (size_t)B;
  const int n = clamp_nz(nz[blockIdx.x], B);
  int c = 0;
  double s = 0.0;
  for (int j = tid; j < n; j += nt) {
    const float v = x[row + j];
    sv[j] = v;
    s += (double)v;
  }
  block_sum(c, s, 0, pc, ps, lane, wv, nw);   // its barrier also publishes sv
  int cnt = n;
  double tau = (s - 1.0) / (double)n;
  for (int step = 1;; ++step) {
    c = 0; s = 0.0;
    for (int j = tid; j < n; j += nt) {
      const float v = sv[j];
      if ((double)v > tau) { ++c; s += (double)v; }
    }
    block_sum(c, s, step & 1, pc, ps, lane, wv, nw);
    // the support repeats: tau is its threshold.  (c > cnt or c == 0 only by rounding at magnitudes where 1 is below
    // an ulp of the entries; tau stays the last one computed.)  cnt falls in every other case: at most n rounds.
    if (c >= cnt || c == 0) break;
    tau = (s - 1.0) / (double)c;
    cnt = c;
  }
  for (int j = tid; j < B; j += nt)
    out[row + j] = j < n ? (float)fmax((double)sv[j] - tau, 0.0) : 0.0f;
}

// ---------------------------------------------------------------------------------------------------- solver
// v of lane ^ 1
TOUED_DEV double pair_f64(double v) { return dpp_f64<0xB1>(v); }

template <int BP>
__global__ void __launch_bounds__((4 * BP < 128 ? 128 : 4 * BP))
k_nash(const float* __restrict__ payoff, const int* __restrict__ nxp, const int* __restrict__ nyp,
       const float* __restrict__ x0, const float* __restrict__ y0, int B, int iters, float lr,
       float* __restrict__ x_avg, float* __restrict__ y_avg, float* __restrict__ stats) {
  constexpr int NT = 4 * BP < 128 ? 128 : 4 * BP;
  constexpr int TS = NT / 2;     // threads of a side (a multiple of 64: a wave belongs to one side)
  constexpr int WS = TS / 64;    // waves of a side
  constexpr int NCH = BP / 8;    // 4-wide chunks of a thread
  __shared__ __align__(16) double cur[2][2][BP];   // x, y of iteration parity 0 / 1: iteration n reads [n & 1] and
                                                   // writes [~n & 1], so a side never overwrites what the other reads
  __shared__ __align__(16) double pre[2][BP];  // x - lr M y, y + lr x^T M before the projection; -inf at index >= nz
  __shared__ int pcnt[2][WS];
  __shared__ double psum[2][WS];
  __shared__ double prod[2][BP];               // M ybar, xbar^T M (the stats)

  const int tid = threadIdx.x, g = blockIdx.x;
  const int side = tid / TS, t = tid % TS, e = t >> 1, h = t & 1, wv = t >> 6, lane = tid & 63;
  const int nx = clamp_nz(nxp[g], B), ny = clamp_nz(nyp[g], B);
  const int nz = side ? ny : nx;
  const bool owner = h == 0 && e < BP;         // the thread that writes entry e
  const double NEG_INF = -(double)__builtin_inff();

  // this thread's part of row e (x side) or column e (y side); the inactive block and the padding are zeros
  const float* M = payoff + (size_t)g * (size_t)B * (size_t)B;
  double m[NCH * 4];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = (2 * c + h) * 4 + r;
      const int row = side ? j : e, col = side ? e : j;
      m[4 * c + r] = (row < nx && col < ny) ? (double)M[(size_t)row * B + col] : 0.0;
    }
  }
  double mine = e < B ? (double)(side ? y0 : x0)[(size_t)g * B + e] : 0.0;
  if (owner) cur[0][side][e] = mine;
  double acc = mine;
  const double slr = side ? (double)lr : -(double)lr;
  lds_barrier();

  for (int it = 0; it < iters; ++it) {
    // 1. g = M y (x side), x^T M (y side) on the old strategies
    const double2* oth = reinterpret_cast<const double2*>(cur[it & 1][side ^ 1]);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const double2 o0 = oth[2 * (2 * c + h)], o1 = oth[2 * (2 * c + h) + 1];
      a0 = fma(m[4 * c + 0], o0.x, a0);
      a1 = fma(m[4 * c + 1], o0.y, a1);
      a2 = fma(m[4 * c + 2], o1.x, a2);
      a3 = fma(m[4 * c + 3], o1.y, a3);
    }
    double p = (a0 + a1) + (a2 + a3);
    p += pair_f64(p);                            // the other half, lane ^ 1 (both lanes get the same sum)
    const double ve = e < nz ? fma(slr, p, mine) : NEG_INF;
    if (owner) pre[side][e] = ve;
    if constexpr (WS > 1) lds_barrier();
    else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // pre[side] stays inside the side's one wave

    // 2. e is in the support iff sum_j max(v_j - v_e, 0) < 1
    const double2* pv = reinterpret_cast<const double2*>(pre[side]);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const double2 q0 = pv[2 * (2 * c + h)], q1 = pv[2 * (2 * c + h) + 1];
      s0 += fmax(q0.x - ve, 0.0);
      s1 += fmax(q0.y - ve, 0.0);
      s2 += fmax(q1.x - ve, 0.0);
      s3 += fmax(q1.y - ve, 0.0);
    }
    double S = (s0 + s1) + (s2 + s3);
    S += pair_f64(S);
    const bool in = owner && e < nz && S < 1.0;
    int k = __popcll(__builtin_amdgcn_ballot_w64(in));
    double sm = wave_sum_f64(in ? ve : 0.0);
    if constexpr (WS > 1) {
      if (lane == 0) { pcnt[side][wv] = k; psum[side][wv] = sm; }
      lds_barrier();
      k = 0; sm = 0.0;
#pragma unroll
      for (int w = 0; w < WS; ++w) { k += pcnt[side][w]; sm += psum[side][w]; }
    }

    // 3. the new strategy
    const double tau = (sm - 1.0) / (double)k;
    mine = e < nz ? fmax(ve - tau, 0.0) : 0.0;
    acc += mine;
    if (owner) cur[(it + 1) & 1][side][e] = mine;
    lds_barrier();
  }

  // the means of the iters + 1 iterates, and from them (as rounded to f32) the value and the exploitability in f64
  const float avg = e < B ? (float)(acc / (double)(iters + 1)) : 0.0f;
  double (*fin)[BP] = cur[(iters + 1) & 1];    // the buffer that nobody reads any more
  if (owner) {
    fin[side][e] = (double)avg;
    if (e < B) (side ? y_avg : x_avg)[(size_t)g * B + e] = avg;
  }
  lds_barrier();
  double d = 0.0;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
#pragma unroll
    for (int r = 0; r < 4; ++r) d += m[4 * c + r] * fin[side ^ 1][(2 * c + h) * 4 + r];
  }
  d += pair_f64(d);
  if (owner) prod[side][e] = d;
  lds_barrier();
  if (tid == 0) {
    double value = 0.0, lo = prod[0][0], hi = prod[1][0];
    for (int i = 0; i < B; ++i) value += fin[0][i] * prod[0][i];
    for (int i = 1; i < nx; ++i) lo = fmin(lo, prod[0][i]);
    for (int j = 1; j < ny; ++j) hi = fmax(hi, prod[1][j]);
    stats[2 * (size_t)g] = (float)value;
    stats[2 * (size_t)g + 1] = (float)(hi - lo);
  }
}

template <int BP>
int launch_nash(const float* payoff, const int* nx, const int* ny, const float* x0, const float* y0, int G, int B,
                int iters, float lr, float* x_avg, float* y_avg, float* stats, hipStream_t stream) {
  constexpr int NT = 4 * BP < 128 ? 128 : 4 * BP;
  hipLaunchKernelGGL(k_nash<BP>, dim3(G), dim3(NT), 0, stream, payoff, nx, ny, x0, y0, B, iters, lr, x_avg, y_avg,
                     stats);
  TOUED_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" {

int toued_project_simplex(const float* x, const int* nz, int R, int B, float* out, hipStream_t stream) {
  TOUED_REQUIRE(R >= 0, "toued_project_simplex: R=%d must be >= 0", R);
  TOUED_REQUIRE(B >= 1 && B <= kProjMaxB, "toued_project_simplex: B=%d outside [1, %d]", B, kProjMaxB);
  if (R == 0) return 0;
  TOUED_REQUIRE(x != nullptr && nz != nullptr && out != nullptr, "toued_project_simplex: null x, nz or out");
  const int block = B <= 256 ? 64 : (B <= 2048 ? 256 : 1024);
  hipLaunchKernelGGL(k_project_simplex, dim3(R), dim3(block), 0, stream, x, nz, B, out);
  TOUED_CHECK_LAUNCH();
  return 0;
}

int toued_nash_fits(int B) { return B >= 1 && B <= kNashMaxB ? 1 : 0; }

int toued_nash_solve(const float* payoff, const int* nx, const int* ny, const float* x0, const float* y0, int G, int B,
                     int iters, float lr, float* x_avg, float* y_avg, float* stats, hipStream_t stream) {
  TOUED_REQUIRE(toued_nash_fits(B), "toued_nash_solve: B=%d outside [1, %d]", B, kNashMaxB);
  TOUED_REQUIRE(G >= 0, "toued_nash_solve: G=%d must be >= 0", G);
  TOUED_REQUIRE(iters >= 0 && iters <= kNashMaxIters, "toued_nash_solve: iters=%d outside [0, %d]", iters,
                kNashMaxIters);
  TOUED_REQUIRE(lr == lr && lr - lr == 0.0f, "toued_nash_solve: lr is not finite");
  if (G == 0) return 0;
  TOUED_REQUIRE(payoff != nullptr && nx != nullptr && ny != nullptr && x0 != nullptr && y0 != nullptr,
                "toued_nash_solve: null payoff, nx, ny, x0 or y0");
  TOUED_REQUIRE(x_avg != nullptr && y_avg != nullptr && stats != nullptr,
                "toued_nash_solve: null x_avg, y_avg or stats");
#define TOUED_NASH_LAUNCH(BP) \
  launch_nash<BP>(payoff, nx, ny, x0, y0, G, B, iters, lr, x_avg, y_avg, stats, stream)
  if (B <= 8) return TOUED_NASH_LAUNCH(8);
  if (B <= 16) return TOUED_NASH_LAUNCH(16);
  if (B <= 32) return TOUED_NASH_LAUNCH(32);
  if (B <= 64) return TOUED_NASH_LAUNCH(64);
  return TOUED_NASH_LAUNCH(128);
#undef TOUED_NASH_LAUNCH
}

}  // extern "C"
