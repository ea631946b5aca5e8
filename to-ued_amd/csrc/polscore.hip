// Policy PLR scores of a batch of eval trajectories (Prioritized Level Replay's policy entropy, least confidence and
// min margin, Jiang et al. 2021, Table 1) — HIP for gfx950.
//
// Per agent a, on the observation rows toued_rollout writes (tidx / ttime [N][T+1][W]; rows t < T enter, the end
// observation does not), with the actor table theta[a] [D][5]:
//   c   = (float)time * 0.001f;   l_j = theta[a][idx][j] + c * theta[a][D-1][j];   m = max_j l_j;   d_j = l_j - m
//   e_j = pexp_le0(d_j);   s = e_0 + ... + e_4;   p_j = e_j / s                    actor_probs5 (env_dev.h), its order
//   q   = e_0 d_0 + ... + e_4 d_4;   H = max(plog(s) - q / s, 0)                   the entropy -sum_j p_j log p_j
//   lc  = 1 - p_max;   mm = 1 - (p_max - p_2nd)                                    p_2nd: second entry of p sorted
//   entropy[a] = mean H / log 5,   least_conf[a] = mean lc,   min_margin[a] = mean mm     over the W * T pairs
// in f32 with one rounding per operation (this file is compiled with -ffp-contract=off), so the per-step terms are
// bit-identical to the numpy restatement and p is the distribution the rollout drew its action from.  8 bytes per
// (worker, step) are read once and nothing but the scores is written (plus the terms, when the caller asks).
//
//   * H: log p_j = d_j - log s, so -sum_j p_j log p_j = log s - (sum_j e_j d_j) / s: one log and one divide in place
//     of five logs, and no log of a probability that underflowed to 0 (e_j = 0 contributes e_j d_j = -0).
//   * p_max and p_2nd are the quotients of the two largest e_j: a correctly rounded division by one s is monotone, so
//     they are the bits of the two largest p_j, and the other three divisions are never made.
//   * One workgroup of 512 threads per agent, the agent's table staged once in dynamic LDS (D = 5409: 108 180 bytes,
//     above the 64 KB default: the host raises the kernel's limit).  The kernel is bound by vector arithmetic (about
//     290 instructions per pair), and a table of that size leaves room for one workgroup per CU only: 8 waves put two
//     on every SIMD, which a single wave cannot keep busy (measured: DESIGN.md section 6).
//   * The rows t < T of an agent are one contiguous block of T * W ints in each of tidx and ttime: it is walked flat,
//     in chunks of 2048 pairs, pair e = chunk * 2048 + i * 512 + tid, 4 per thread.  All 8 loads of a chunk are issued,
//     non-temporal, before the first use, and the next chunk's before the current chunk's arithmetic.  Nothing is
//     sequential: no barrier between the staging barrier and the final reduction, and W > 512 needs nothing special.
//   * Three f64 partial sums per thread, reduced and rounded once as trajscore_dev.h describes (the entropy is also
//     divided by log 5).
#include "trajscore_dev.h"

namespace {

using trajscore::block_reduce;
using trajscore::clamp_row;
using trajscore::trajscore_check;

constexpr int kPsThreads = 512;
constexpr int kPsPairs = 4;                          // (worker, step) pairs per thread and chunk
constexpr int kPsChunk = kPsThreads * kPsPairs;      // pairs per chunk
constexpr double kPsLog5 = 1.6094379124341003;       // log 5, the entropy of the uniform policy over 5 actions

// dynamic LDS: double red[3][threads]; float tab[D][5]
constexpr size_t kPsLdsMax = 150 * 1024;             // what the project's other kernels ask for at the most
constexpr size_t kPsRedBytes = 3 * kPsThreads * sizeof(double);
constexpr int kPsMaxD = (int)((kPsLdsMax - kPsRedBytes) / (5 * sizeof(float)));   // 7065 table rows
inline size_t polscore_lds_bytes(int D) { return kPsRedBytes + (size_t)D * 5 * sizeof(float); }

// plog on a sum of softmax exponentials (1 <= x <= 5, or NaN): the same value as plog(x) for every such x, with the
// tests for 0, negative, infinite and subnormal arguments dropped, so that a wave runs one straight-line sequence and
// the terms of a thread's pairs can be interleaved.
TOUED_DEV float plog_sum(float x) {
  const uint32_t bits = __float_as_uint(x);
  int e = (int)((bits >> 23) & 0xFFu) - 127;
  float m = __uint_as_float((bits & 0x7FFFFFu) | 0x3F800000u);
  const bool up = m > 1.41421356237f;
  m = up ? __fmul_rn(m, 0.5f) : m;
  e = up ? e + 1 : e;
  const float f = __fsub_rn(m, 1.0f);
  const float s = __fdiv_rn(f, __fadd_rn(2.0f, f));
  const float z = __fmul_rn(s, s);
  const float w = __fmul_rn(z, z);
  const float t1 = __fmul_rn(w, __fadd_rn(0.40000972152f, __fmul_rn(w, 0.24279078841f)));
  const float t2 = __fmul_rn(z, __fadd_rn(0.66666662693f, __fmul_rn(w, 0.28498786688f)));
  const float R = __fadd_rn(t2, t1);
  const float hfsq = __fmul_rn(__fmul_rn(0.5f, f), f);
  const float dk = (float)e;
  const float inner = __fadd_rn(__fmul_rn(s, __fadd_rn(hfsq, R)), __fmul_rn(dk, 1.428606765330187045e-06f));
  const float v = __fsub_rn(__fmul_rn(dk, 0.693145751953125f), __fsub_rn(__fsub_rn(hfsq, inner), f));
  return x != x ? x : v;
}

// The three per-step terms of one (worker, step) pair from the table in LDS; `last` is row D-1.
TOUED_DEV void policy_terms(const float* tab, const float* last, unsigned dmax, int idx, int tm, float& H, float& lc,
                            float& mm) {
  const unsigned i = clamp_row(idx, dmax);
  const float c = __fmul_rn((float)tm, 0.001f);
  float l[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) l[j] = __fadd_rn(tab[i * 5 + j], __fmul_rn(c, last[j]));
  float m = l[0];
#pragma unroll
  for (int j = 1; j < 5; ++j) m = fmaxf(m, l[j]);
  float d[5], e[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    d[j] = __fsub_rn(l[j], m);
    e[j] = pexp_le0(d[j]);
  }
  float s = e[0], q = __fmul_rn(e[0], d[0]);
  float hi = e[0], nx = -1.0f;       // the largest and the second largest e_j (two equal maxima: nx = hi)
#pragma unroll
  for (int j = 1; j < 5; ++j) {
    s = __fadd_rn(s, e[j]);
    q = __fadd_rn(q, __fmul_rn(e[j], d[j]));
    nx = fmaxf(nx, fminf(hi, e[j]));
    hi = fmaxf(hi, e[j]);
  }
  H = fmaxf(__fsub_rn(plog_sum(s), __fdiv_rn(q, s)), 0.0f);
  const float pmax = __fdiv_rn(hi, s), p2nd = __fdiv_rn(nx, s);
  lc = __fsub_rn(1.0f, pmax);
  mm = __fsub_rn(1.0f, __fsub_rn(pmax, p2nd));
}

__global__ void __launch_bounds__(kPsThreads) k_policy_scores(
    int W, int T, int D, const float* __restrict__ theta, const int* __restrict__ tidx,
    const int* __restrict__ ttime, float* __restrict__ entropy, float* __restrict__ least_conf,
    float* __restrict__ min_margin, float* __restrict__ steps) {
  extern __shared__ __align__(16) unsigned char smem[];
  double* red = reinterpret_cast<double*>(smem);
  float* tab = reinterpret_cast<float*>(smem + kPsRedBytes);

  const int a = blockIdx.x, tid = threadIdx.x;
  const unsigned TW = (unsigned)T * (unsigned)W;     // < 2^31 (checked by the host)
  const int* ti = tidx + (size_t)a * (T + 1) * W;
  const int* tt = ttime + (size_t)a * (T + 1) * W;
  // the raw trajectory of the chunk at c0 into registers, no branch between the loads: a pair past the end reads the
  // agent's first pair instead (in bounds, never used)
  int ni[kPsPairs], nt[kPsPairs];
  auto load = [&](unsigned c0) {
#pragma unroll
    for (int i = 0; i < kPsPairs; ++i) {
      const unsigned e = c0 + i * kPsThreads + tid;
      const unsigned off = e < TW ? e : 0u;
      ni[i] = __builtin_nontemporal_load(ti + off);
      nt[i] = __builtin_nontemporal_load(tt + off);
    }
  };
  load(0u);      // in flight across the staging of the table

  const float* tg = theta + (size_t)a * D * 5;
  const int n5 = D * 5;
  for (int i = tid; i < n5; i += kPsThreads) tab[i] = tg[i];
  const unsigned dmax = (unsigned)(D - 1);
  __syncthreads();
  float last[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) last[j] = tab[dmax * 5 + j];

  double sh = 0.0, sl = 0.0, sm = 0.0;
  float* st = steps != nullptr ? steps + (size_t)a * 3 * TW : nullptr;
  for (unsigned c0 = 0; c0 < TW; c0 += kPsChunk) {
    int ci[kPsPairs], ct[kPsPairs];
#pragma unroll
    for (int i = 0; i < kPsPairs; ++i) {
      ci[i] = ni[i];
      ct[i] = nt[i];
    }
    if (c0 + kPsChunk < TW) load(c0 + kPsChunk);   // in flight across the arithmetic below
    float H[kPsPairs], lc[kPsPairs], mm[kPsPairs];
#pragma unroll
    for (int i = 0; i < kPsPairs; ++i) policy_terms(tab, last, dmax, ci[i], ct[i], H[i], lc[i], mm[i]);
    // a pair past the end adds +0.0, which changes no bit of a sum that started at +0.0
#pragma unroll
    for (int i = 0; i < kPsPairs; ++i) {
      const bool in = c0 + i * kPsThreads + tid < TW;
      sh += in ? (double)H[i] : 0.0;
      sl += in ? (double)lc[i] : 0.0;
      sm += in ? (double)mm[i] : 0.0;
    }
    if (st != nullptr) {
#pragma unroll
      for (int i = 0; i < kPsPairs; ++i) {
        const unsigned e = c0 + i * kPsThreads + tid;
        if (e < TW) {
          st[e] = H[i];
          st[(size_t)TW + e] = lc[i];
          st[2 * (size_t)TW + e] = mm[i];
        }
      }
    }
  }

  red[tid] = sh;
  red[kPsThreads + tid] = sl;
  red[2 * kPsThreads + tid] = sm;
  block_reduce<kPsThreads, 3, false>(red, nullptr, tid);
  if (tid == 0) {
    const double cnt = (double)W * (double)T;
    if (entropy != nullptr) entropy[a] = (float)(red[0] / cnt / kPsLog5);
    if (least_conf != nullptr) least_conf[a] = (float)(red[kPsThreads] / cnt);
    if (min_margin != nullptr) min_margin[a] = (float)(red[2 * kPsThreads] / cnt);
  }
}

}  // namespace

extern "C" {

int toued_policy_scores(int N, int W, int T, int D, const float* theta, const int* tidx, const int* ttime,
                        float* entropy, float* least_conf, float* min_margin, float* steps, hipStream_t stream) {
  const int go = trajscore_check("toued_policy_scores", N, W, T, D, kPsMaxD, "an actor table", "rows");
  if (go <= 0) return go;
  TOUED_REQUIRE(theta && tidx && ttime, "toued_policy_scores: null input buffer");
  TOUED_REQUIRE(entropy || least_conf || min_margin, "toued_policy_scores: entropy, least_conf and min_margin are "
                "all null");
  static bool attr_set = false;
  if (!attr_set) {
    TOUED_REQUIRE(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_policy_scores),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPsLdsMax) == hipSuccess,
                  "toued_policy_scores: cannot raise the dynamic LDS limit");
    attr_set = true;
  }
  hipLaunchKernelGGL(k_policy_scores, dim3(N), dim3(kPsThreads), polscore_lds_bytes(D), stream, W, T, D, theta, tidx,
                     ttime, entropy, least_conf, min_margin, steps);
  TOUED_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
