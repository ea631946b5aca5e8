// Exact optimal return of tabular GridWorld levels (environments/gridworld/gridworld.py:253-323, vmapped by
// RolloutWrapper.optimal_return, environments/rollout.py:104-108) — HIP for gfx950.
//
// Finite-horizon dynamic programming over (time, position, object-existence): v_L = 0 and, for t = L-1 .. 0,
//   q(s, a) = r + (1 - p_term) * E[v_{t+1}(pos1, e')],   v_t(s) = max_a q(s, a)
// on the project's tabular state index s = pos + max_grid^2 * exists_mask (env_dev.h tab_index).
//
//   * One workgroup per level.  v_{t+1} and v_t are double-buffered in LDS as f64 (two tables of
//     S = max_grid^2 * 2^n_max entries: 87 KB at the largest tabular mode), so the H accumulated backups stay far
//     inside H * 2^-23 * max|v| of the float64 recursion; the outputs are rounded to f32 once.
//   * Built once per level before the time loop: the (cell, action) -> next cell | objects-there table (the A2C
//     chain's build_npt entries), the list of valid cells, the reward and 1 - p_term of every collected set, and the
//     respawn weights P[absent][R] = prod over the absent objects of (R_i ? p_respawn_i : 1 - p_respawn_i) for every R
//     inside `absent`.
//   * Only valid states are enumerated (valid cell x subsets of the level's n_objs objects): a small level padded into
//     a large mode's table costs what it contains.  Invalid states hold -inf in both buffers from the start and are
//     never read by a valid state's backup (a move stays on valid cells, unused objects never appear), so no
//     0 * (-inf) can form: a zero-weight outcome contributes an exact zero, as the reference's where(p > 0, v, 0).
//   * Work items are ordered existence-mask major: the lanes of a wave share `absent`, so they run the same number of
//     outcome terms and read neighbouring cells of one table slice; the masks are taken from the most absent objects to
//     the fewest, so a thread's items (a block size apart) mix heavy and light states.
//   * The outcome loop: per round two subsets' weights, read once for the five actions, and their ten values, read
//     independently, feed ten f64 fmas (32-bit LDS indices, no per-term test).
//   * One LDS-only barrier per time step; the only global traffic inside the loop is the optional v_all row store.
//   * Only the count of unmasked steps matters (v_t is zero for t >= max_steps_in_episode): H = min(max_steps,
//     max_rollout_len) backups give v_0, and the rows t >= max_steps of v_all are zero fills.
//
// k_policy_return is the same recursion for the expected return of a tabular agent's own policy,
// v_t(s) = sum_a pi_t(a|s) q(s, a), and k_policy_moments adds the variance of that return, u_t(s) = Var[G_t | s], in
// two f32 tables behind the setup's LDS.  The three kernels are built from the same parts; a further recursion on
// these tables is a backup function on top of outcome_loop and a kernel with its time loop:
//   optret_setup     the per-level tables                                     all three
//   work_item        work item -> (cell, existence mask)                      all three
//   outcome_loop     an item's next states and E[v'] (and E[u' + v'^2])       all three
//   step_end         a step's barrier, v_all (var_all) row stores, table swap  all three
//   write_start      v0 (var0) at the start state                             all three
//   softmax_backup   sum_a pi(a) q(s, a) (and the variance beside it)         k_policy_return, k_policy_moments
//   policy_items     a thread's items and their theta rows in registers       k_policy_return, k_policy_moments
// k_optimal_return's backup, the max over the actions, is written in the kernel.
//
// k_policy_occupancy is the forward counterpart of k_policy_return: the state occupancy d_t(s) of the policy, pushed
// from the start state through the same next-state, reward, keep and respawn tables (optret_setup, work_item,
// policy_items), with the two value tables read as u64 fixed-point mass.  It holds 1 - p_term to [0, 1], as the env's
// bernoulli(p_term) does; k_policy_return and k_policy_moments follow the reference's DP and do not clamp, so the
// return obtained from the occupancy equals theirs on the levels whose collected sets have sum p_terminate <= 1.
#include <type_traits>

#include "env_dev.h"

namespace {

constexpr size_t kOptretLdsMax = 150 * 1024;   // of the CU's 160 KB

// dynamic LDS: f64 va[S], vb[S], pw[4^n_max + 1], rsum[2^n_max], keepw[2^n_max]; int lev[LEVEL_WORDS];
// u16 nxt[G2 * 5]; u8 cells[G2], eord[2^n_max]
__host__ __device__ inline size_t optret_lds_bytes(int G2, int n_max) {
  const size_t S = (size_t)G2 << n_max;
  size_t b = (2 * S + ((size_t)1 << (2 * n_max)) + 1 + ((size_t)2 << n_max)) * sizeof(double) +
             LEVEL_WORDS * sizeof(int) + (size_t)G2 * 5 * sizeof(uint16_t) + (size_t)G2 + ((size_t)1 << n_max);
  return (b + 15) & ~(size_t)15;
}

// The per-level tables of both kernels, in dynamic LDS, and the level's scalars.
struct OptretSetup {
  double *va, *pw, *rsum, *keepw;
  const int* lev;
  const uint16_t* nxt;
  const uint8_t *cells, *eord;
  int G2, S, NE, used, ne, H, ncell;
};

// Builds the tables of level blockIdx.x (see the head of this file), fills both value tables with v_H and the rows
// t >= max_steps of v_all with zeros, and ends with a block barrier.
__device__ __forceinline__ OptretSetup optret_setup(unsigned char* smem, const int* __restrict__ levels, int max_grid,
                                                    int n_max, int L, float* __restrict__ v_all) {
  const int G2 = max_grid * max_grid;
  const int S = G2 << n_max;
  const int NE = 1 << n_max;
  double* va = reinterpret_cast<double*>(smem);
  double* vb = va + S;
  double* pw = vb + S;
  double* rsum = pw + NE * NE + 1;
  double* keepw = rsum + NE;
  int* lev = reinterpret_cast<int*>(keepw + NE);
  uint16_t* nxt = reinterpret_cast<uint16_t*>(lev + LEVEL_WORDS);
  uint8_t* cells = reinterpret_cast<uint8_t*>(nxt + G2 * 5);
  uint8_t* eord = cells + G2;
  __shared__ int s_ncell;

  const int tid = threadIdx.x, nt = blockDim.x;
  const int* glev = levels + (size_t)blockIdx.x * LEVEL_WORDS;
  // the level record, with the fields that index tables held to the mode's static bounds
  for (int i = tid; i < LEVEL_WORDS; i += nt) {
    int w = glev[i];
    if (i == L_GRID) w = w < 1 ? 1 : (w > max_grid ? max_grid : w);
    if (i == L_NOBJS) w = w < 0 ? 0 : (w > n_max ? n_max : w);
    if (i == L_START) w = w < 0 ? 0 : (w >= G2 ? G2 - 1 : w);
    lev[i] = w;
  }
  __syncthreads();
  const int g = lev[L_GRID], g2 = g * g;
  const int nobj = lev[L_NOBJS], used = (1 << nobj) - 1, ne = 1 << nobj;
  const int max_steps = lev[L_MAX_STEPS];
  const int H = max_steps < L ? (max_steps < 0 ? 0 : max_steps) : L;
  const float ninf = -__builtin_inff();

  // (cell, action) -> next cell | (objects placed there) << 8, for the level's valid cells
  for (int c = tid; c < G2 * 5; c += nt) {
    const int pos = c / 5, a = c - pos * 5;
    uint16_t e = 0;
    if (pos < g2 && !wall_at((const int*)lev, pos)) {
      const int p1 = next_pos((const int*)lev, pos, a);
      int m = 0;
      for (int o = 0; o < nobj; ++o)
        if (lev[L_STATIC + o] == p1) m |= 1 << o;
      e = (uint16_t)(p1 | (m << 8));
    }
    nxt[c] = e;
  }
  // reward and 1 - p_term of collecting the objects c (c inside used)
  for (int c = tid; c < ne; c += nt) {
    double rs = 0.0, pt = 0.0;
    for (int o = 0; o < nobj; ++o)
      if ((c >> o) & 1) {
        rs += (double)__int_as_float(lev[L_REW + o]);
        pt += (double)__int_as_float(lev[L_PTERM + o]);
      }
    rsum[c] = rs;
    keepw[c] = 1.0 - pt;
  }
  // respawn weights: pw[absent * NE + R], R inside absent inside used
  for (int i = tid; i < NE * NE; i += nt) {
    const int A = i >> n_max, R = i & (NE - 1);
    double p = 0.0;
    if (!(R & ~A) && !(A & ~used)) {
      p = 1.0;
      for (int o = 0; o < nobj; ++o)
        if ((A >> o) & 1) {
          const double pr = (double)__int_as_float(lev[L_PRESP + o]);
          p *= ((R >> o) & 1) ? pr : 1.0 - pr;
        }
    }
    pw[i] = p;
  }
  if (tid == 0) pw[NE * NE] = 0.0;
  if (tid == 0) {
    int n = 0;
    for (int pos = 0; pos < g2; ++pos)
      if (!wall_at((const int*)lev, pos)) cells[n++] = (uint8_t)pos;
    s_ncell = n;
  }
  // the level's existence masks by ascending count of present objects, i.e. from the most outcome terms (2^absent) to
  // the fewest: a thread's work items, a block size apart in this order, then mix heavy and light states
  if (tid == 64 % nt) {
    int n = 0;
    for (int pc = 0; pc <= nobj; ++pc)
      for (int e = 0; e < ne; ++e)
        if (__builtin_popcount(e) == pc) eord[n++] = (uint8_t)e;
  }
  // both tables: -inf at the invalid states for good, v_H = 0 at the valid ones
  for (int s = tid; s < S; s += nt) {
    const int pos = s % G2, e = s / G2;
    const bool valid = pos < g2 && !wall_at((const int*)lev, pos) && !(e & ~used);
    va[s] = vb[s] = valid ? 0.0 : (double)ninf;
  }
  // rows t >= max_steps of v_all are zero, invalid states included
  if (v_all != nullptr) {
    float* rows = v_all + ((size_t)blockIdx.x * L + H) * S;
    const size_t nz = (size_t)(L - H) * S;
    for (size_t i = tid; i < nz; i += nt) rows[i] = 0.0f;
  }
  __syncthreads();

  return OptretSetup{va, pw, rsum, keepw, lev, nxt, cells, eord, G2, S, NE, used, ne, H, s_ncell};
}

// Work item w (< ncell * ne) in the setup's order: its existence mask and cell.
__device__ __forceinline__ void work_item(const OptretSetup& T, int w, int& pos, int& e) {
  const int ei = w / T.ncell;
  e = T.eord[ei];
  pos = T.cells[w - ei * T.ncell];
}

// The outcomes of the five actions in state (pos, e), read from table `nxo`: col[a], the objects the move collects,
// ev[a] = E[v'] over the subsets R of the absent objects that respawn and, with VAR, ez[a] = E[u' + v'^2] with the
// next state's variance u' read as f32 from ua (one more LDS read and one more accumulation per outcome).
// after_cols() runs once col[] is known and before the loop: k_optimal_return's reads by col[] start there.  (As two
// helpers, next states and loop, with those reads between them, k_optimal_return measured 1 % slower on 4000 `all`
// levels.)
// The loop takes two subsets per round: one weight read serves the five actions, and the ten value reads of a round
// are independent.  Every value read is a valid state's (finite), so a zero weight gives a zero term without a test; a
// second subset that does not exist reads subset 0 with weight 0.
template <bool VAR, class AfterCols>
__device__ __forceinline__ void outcome_loop(const OptretSetup& T, const float* ua, int nxo, int pos, int e, int* col,
                                             double* ev, double* ez, AfterCols after_cols) {
  const double* va = T.va;
  const double* pw = T.pw;
  const int G2 = T.G2, NE = T.NE;
  const int absent = T.used & ~e;
  const double* pwa = pw + absent * NE;
  int base[5];            // index in table nxo of (next cell, e without col[a]); an outcome adds G2 * R
  double sv[5], sz[5];    // the sums, in registers whatever ev and ez point to
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    const uint32_t en = T.nxt[pos * 5 + a];
    col[a] = (int)(en >> 8) & e;
    base[a] = nxo + (int)(en & 0xFFu) + G2 * (e & ~col[a]);
  }
  after_cols();
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    sv[a] = 0.0;
    if constexpr (VAR) sz[a] = 0.0;
  }
  int R0 = 0;
  do {
    const int R1 = (R0 - absent) & absent;
    const double p0 = pwa[R0];
    const double p1 = pw[R1 != 0 ? absent * NE + R1 : NE * NE];   // pw[NE * NE] = 0
    const int o0 = G2 * R0, o1 = G2 * R1;
    double x0[5], x1[5];
    float y0[5], y1[5];
#pragma unroll
    for (int a = 0; a < 5; ++a) {
      x0[a] = va[base[a] + o0];
      x1[a] = va[base[a] + o1];
      if constexpr (VAR) {
        y0[a] = ua[base[a] + o0];
        y1[a] = ua[base[a] + o1];
      }
    }
    __builtin_amdgcn_sched_barrier(0);   // all the round's reads in flight before the first fma waits
#pragma unroll
    for (int a = 0; a < 5; ++a) {
      sv[a] = __builtin_fma(p1, x1[a], __builtin_fma(p0, x0[a], sv[a]));
      if constexpr (VAR) {
        const double z0 = __builtin_fma(x0[a], x0[a], (double)y0[a]);
        const double z1 = __builtin_fma(x1[a], x1[a], (double)y1[a]);
        sz[a] = __builtin_fma(p1, z1, __builtin_fma(p0, z0, sz[a]));
      }
    }
    R0 = R1 != 0 ? (R1 - absent) & absent : 0;
  } while (R0 != 0);
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    ev[a] = sv[a];
    if constexpr (VAR) ez[a] = sz[a];
  }
}

// Ends step t: one LDS-only barrier, the optional row t of v_all (var_all), and the tables swap.
template <bool VAR>
__device__ __forceinline__ void step_end(const OptretSetup& T, const float* ua, int L, int t, float* v_all,
                                         float* var_all, int& curo, int& nxo) {
  const double* va = T.va;
  const int S = T.S;
  const int tid = threadIdx.x, nt = blockDim.x;
  lds_barrier();
  if (v_all != nullptr) {
    float* out = v_all + ((size_t)blockIdx.x * L + t) * S;
    for (int s = tid; s < S; s += nt) out[s] = (float)va[curo + s];
  }
  if constexpr (VAR) {
    if (var_all != nullptr) {
      float* out = var_all + ((size_t)blockIdx.x * L + t) * S;
      for (int s = tid; s < S; s += nt) out[s] = ua[curo + s];
    }
  }
  const int sw = curo; curo = nxo; nxo = sw;
}

// After the last step table nxo holds v_0 (u_0): thread 0 writes them at the start state, 0 when H == 0
template <bool VAR>
__device__ __forceinline__ void write_start(const OptretSetup& T, const float* ua, int nxo, float* v0, float* var0) {
  if (threadIdx.x == 0) {
    const int si = nxo + T.lev[L_START] + T.G2 * T.used;
    v0[blockIdx.x] = T.H > 0 ? (float)T.va[si] : 0.0f;
    if constexpr (VAR) var0[blockIdx.x] = T.H > 0 ? ua[si] : 0.0f;
  }
}

__global__ void k_optimal_return(const int* __restrict__ levels, int max_grid, int n_max, int L,
                                 float* __restrict__ v0, float* __restrict__ v_all) {
  extern __shared__ __align__(16) unsigned char smem[];
  const OptretSetup T = optret_setup(smem, levels, max_grid, n_max, L, v_all);
  const int tid = threadIdx.x, nt = blockDim.x;
  const int nwork = T.ncell * T.ne;
  int curo = 0;    // v_t, written: table va (offset 0) or vb (offset S) of the 2S-entry array
  int nxo = T.S;   // v_{t+1}, read
  for (int t = T.H - 1; t >= 0; --t) {
    for (int w = tid; w < nwork; w += nt) {
      int pos, e;
      work_item(T, w, pos, e);
      int col[5];
      double r[5], keep[5], ev[5];
      outcome_loop<false>(T, nullptr, nxo, pos, e, col, ev, nullptr, [&] {
#pragma unroll
        for (int a = 0; a < 5; ++a) {
          r[a] = T.rsum[col[a]];
          keep[a] = T.keepw[col[a]];
        }
      });
      double best = (double)-__builtin_inff();
#pragma unroll
      for (int a = 0; a < 5; ++a) {
        const double q = r[a] + ev[a] * keep[a];
        best = q > best ? q : best;
      }
      T.va[curo + pos + T.G2 * e] = best;
    }
    step_end<false>(T, nullptr, L, t, v_all, nullptr, curo, nxo);
  }
  write_start<false>(T, nullptr, nxo, v0, nullptr);
}

// One policy backup: v_t(pos, e) = sum_a pi(a) q(s, a) into table `curo` of va, with the policy's f32 logits l[5] (as
// actor_probs5 forms them) and the outcome loop on table `nxo`.  The softmax is exp(l - max) / sum in f64; the argmax
// term is exp(0) = 1, so the sum is >= 1: huge logits give an exact one-hot policy and no NaN.
// With VAR, the return's variance beside its mean, by the same statements: u_t(pos, e) = Var[G_t | s] into table
// `curo` of ua.  With v', u' the next state's mean and variance, the second moment of r + cont * G' given (s, a) is
//   m2(s, a) = r^2 + c * (2 r E[v'] + E[u' + v'^2]),   c = 1 - p_term,
// and u_t(s) = sum_a pi(a) m2(s, a) - v_t(s)^2 (the law of total variance, nothing clipped: c < 0 is taken as the
// mean takes it).  Everything but u' is f64; u_t is rounded to f32 once.
template <bool VAR>
__device__ __forceinline__ void softmax_backup(const OptretSetup& T, float* ua, int nxo, int curo, int pos, int e,
                                               const float* l) {
  int col[5];
  double ev[5], ez[5];
  outcome_loop<VAR>(T, ua, nxo, pos, e, col, ev, ez, [] {});
  float m = l[0];
#pragma unroll
  for (int a = 1; a < 5; ++a) m = fmaxf(m, l[a]);
  double num = 0.0, den = 0.0, num2 = 0.0;
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    const double x = exp((double)l[a] - (double)m);
    const double r = T.rsum[col[a]], keep = T.keepw[col[a]];
    const double q = r + ev[a] * keep;
    den += x;
    num = __builtin_fma(x, q, num);
    if constexpr (VAR) {
      const double m2 = __builtin_fma(keep, __builtin_fma(r + r, ev[a], ez[a]), r * r);
      num2 = __builtin_fma(x, m2, num2);
    }
  }
  const double v = num / den;
  T.va[curo + pos + T.G2 * e] = v;
  if constexpr (VAR) ua[curo + pos + T.G2 * e] = (float)(num2 / den - v * v);
}

// Work item w belongs to thread w % blockDim at every step, so a thread reads the theta rows of its first ITEMS items
// once, before the time loop, and keeps them in registers (the kernels unroll their item loop over ITEMS, so the rows
// are not runtime-indexed): st[k] = pos | e << 8 of the thread's item k, -1 past the level's work, row[k] its logits
// row, and last = theta[D-1], the time feature's row.
template <int ITEMS>
__device__ __forceinline__ void policy_items(const OptretSetup& T, const float* th, int D, int nwork,
                                             float (&last)[5], int (&st)[ITEMS], float (&row)[ITEMS][5]) {
  const int tid = threadIdx.x, nt = blockDim.x;
#pragma unroll
  for (int a = 0; a < 5; ++a) last[a] = th[(size_t)(D - 1) * 5 + a];
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const int w = tid + k * nt;
    st[k] = -1;
#pragma unroll
    for (int a = 0; a < 5; ++a) row[k][a] = 0.0f;
    if (w < nwork) {
      int pos, e;
      work_item(T, w, pos, e);
      st[k] = pos | (e << 8);
      const float* r = th + (size_t)(pos + T.G2 * e) * 5;      // pos + G2 * e < S = D - 1
#pragma unroll
      for (int a = 0; a < 5; ++a) row[k][a] = r[a];
    }
  }
}

// Exact expected return of a tabular agent's own policy: k_optimal_return's recursion with
//   v_t(s) = sum_a pi_t(a|s) q(s, a),   pi_t(.|s) = softmax(theta[s] + fl(fl(t * 0.001) * theta[D-1]))
// in place of the max.  The logits are formed in f32 by actor_probs5's rounded operations; the softmax and the
// backup are f64.  One workgroup per (level, table) pair; theta rows in registers by policy_items.  Every mode's table
// has at most 6 items per thread and runs with MORE = false: theta is not read inside the time loop.  MORE = true
// serves larger tables, which no mode has: the items past the first ITEMS go through a plain loop that reads their
// rows from global memory at every step.
template <int ITEMS, bool MORE>
__global__ __launch_bounds__(1024) void k_policy_return(const int* __restrict__ levels,
                                                        const float* __restrict__ theta, int D, int max_grid,
                                                        int n_max, int L, float* __restrict__ v0,
                                                        float* __restrict__ v_all) {
  extern __shared__ __align__(16) unsigned char smem[];
  const OptretSetup T = optret_setup(smem, levels, max_grid, n_max, L, v_all);
  const int tid = threadIdx.x, nt = blockDim.x;
  const int nwork = T.ncell * T.ne;      // <= S; <= ITEMS * blockDim without MORE (the host's choice of ITEMS)
  const float* th = theta + (size_t)blockIdx.x * D * 5;
  float last[5], row[ITEMS][5];
  int st[ITEMS];
  policy_items(T, th, D, nwork, last, st, row);

  int curo = 0;    // v_t, written
  int nxo = T.S;   // v_{t+1}, read
  for (int t = T.H - 1; t >= 0; --t) {
    const float c = __fmul_rn((float)t, 0.001f);
    float tl[5];
#pragma unroll
    for (int a = 0; a < 5; ++a) tl[a] = __fmul_rn(c, last[a]);
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
      if (st[k] < 0) continue;
      float l[5];
#pragma unroll
      for (int a = 0; a < 5; ++a) l[a] = __fadd_rn(row[k][a], tl[a]);
      softmax_backup<false>(T, nullptr, nxo, curo, st[k] & 0xFF, st[k] >> 8, l);
    }
    if (MORE) {
      for (int w = tid + ITEMS * nt; w < nwork; w += nt) {
        int pos, e;
        work_item(T, w, pos, e);
        const float* r = th + (size_t)(pos + T.G2 * e) * 5;      // pos + G2 * e < S = D - 1
        float l[5];
#pragma unroll
        for (int a = 0; a < 5; ++a) l[a] = __fadd_rn(r[a], tl[a]);
        softmax_backup<false>(T, nullptr, nxo, curo, pos, e, l);
      }
    }
    step_end<false>(T, nullptr, L, t, v_all, nullptr, curo, nxo);
  }
  write_start<false>(T, nullptr, nxo, v0, nullptr);
}

// dynamic LDS of k_policy_moments: optret_setup's layout (a multiple of 16 bytes), then f32 ua[S], ub[S]
__host__ __device__ inline size_t polmom_lds_bytes(int G2, int n_max) {
  return optret_lds_bytes(G2, n_max) + 2 * ((size_t)G2 << n_max) * sizeof(float);
}

// Mean and variance of the first-episode return of a tabular agent's own policy: k_policy_return (its setup, work
// order, block size and, through softmax_backup, its mean arithmetic: v0 and v_all are bit-identical to its) with a
// second table pair for u_t(s) = Var[G_t | s].  The u tables are f32, double-buffered in LDS behind optret_setup's
// layout (two more f64 tables would not fit the largest mode), indexed like va; every step's arithmetic is f64 and
// the f32 store of u_t is the step's only rounding that the f64 recursion does not have.  Invalid states hold -inf in
// both u tables, as in va, and are never read by a valid state's backup.  A table that fits the LDS with the u tables
// has at most six items per thread, so there is no MORE.
template <int ITEMS>
__global__ __launch_bounds__(1024) void k_policy_moments(const int* __restrict__ levels,
                                                         const float* __restrict__ theta, int D, int max_grid,
                                                         int n_max, int L, float* __restrict__ v0,
                                                         float* __restrict__ var0, float* __restrict__ v_all,
                                                         float* __restrict__ var_all) {
  extern __shared__ __align__(16) unsigned char smem[];
  const OptretSetup T = optret_setup(smem, levels, max_grid, n_max, L, v_all);
  const int S = T.S;
  float* const ua = reinterpret_cast<float*>(smem + optret_lds_bytes(T.G2, n_max));
  const int tid = threadIdx.x, nt = blockDim.x;
  const int nwork = T.ncell * T.ne;      // <= S <= ITEMS * blockDim (the host's choice of ITEMS)

  // both u tables: u_H = 0 at the valid states, -inf at the invalid ones (va's fill); zero rows of var_all
  for (int s = tid; s < S; s += nt) ua[s] = ua[S + s] = (float)T.va[s];
  if (var_all != nullptr) {
    float* rows = var_all + ((size_t)blockIdx.x * L + T.H) * S;
    const size_t nz = (size_t)(L - T.H) * S;
    for (size_t i = tid; i < nz; i += nt) rows[i] = 0.0f;
  }
  float last[5], row[ITEMS][5];
  int st[ITEMS];
  policy_items(T, theta + (size_t)blockIdx.x * D * 5, D, nwork, last, st, row);
  __syncthreads();

  int curo = 0;    // v_t and u_t, written
  int nxo = S;     // v_{t+1} and u_{t+1}, read
  for (int t = T.H - 1; t >= 0; --t) {
    const float c = __fmul_rn((float)t, 0.001f);
    float tl[5];
#pragma unroll
    for (int a = 0; a < 5; ++a) tl[a] = __fmul_rn(c, last[a]);
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
      if (st[k] < 0) continue;
      // the item is made opaque per step: what derives from it (next cells, table offsets) is then formed here, not
      // hoisted out of the time loop for all ITEMS items at once (ITEMS = 4 and 6 spilled to scratch that way)
      int sk = st[k];
      asm volatile("" : "+v"(sk));
      float l[5];
#pragma unroll
      for (int a = 0; a < 5; ++a) l[a] = __fadd_rn(row[k][a], tl[a]);
      softmax_backup<true>(T, ua, nxo, curo, sk & 0xFF, sk >> 8, l);
    }
    step_end<true>(T, ua, L, t, v_all, var_all, curo, nxo);
  }
  write_start<true>(T, ua, nxo, v0, var0);
}

// Occupancy mass is held in fixed point, scaled by 2^62, in the setup's two tables read as u64: a state's mass at
// most 1 is at most 2^62, and a whole table sums to at most 2^62, far inside 64 bits.
constexpr double kOccOne = 4611686018427387904.0;           // 2^62
constexpr double kOccInv = 1.0 / 4611686018427387904.0;     // 2^-62, exact
// the eight summary columns as the block's sums (4-6 before their division by the length): a thread adds to ret,
// ret_abs and the three policy terms inside the time loop; its length (the sum of its items' visits) and alive_end are
// filled after it, and p_early_term is a block-wide fixed-point sum beside the collections
enum { OCC_RET = 0, OCC_LEN, OCC_PTERM, OCC_ALIVE, OCC_ENT, OCC_LC, OCC_MM, OCC_RABS, OCC_SUMS };
// The expected collections of an object are a block-wide fixed-point sum too, scaled by 2^48 (a step adds at most 1
// per object, so H < 2^15 steps fit 63 bits): collecting moves are rare, at most 5 * 2^(n_objs - 1) (state, action)
// pairs per object and step, so the sum is within H * 5 * 2^(n_objs - 1) * 2^-48 of the f64 one (2^-30 at the
// largest mode) and a thread keeps no register per object.
constexpr double kColOne = 281474976710656.0;               // 2^48
constexpr double kColInv = 1.0 / 281474976710656.0;

// One state's forward step: the mass m = d_t(pos, e) > 0 goes, for every action a and every subset R of the absent
// objects that respawns, as m pi(a) keep(col) pw[absent][R] into table `nxo` at (next cell, (e \ col) | R), truncated
// to a multiple of 2^-62 and added with a 64-bit integer LDS atomic: integer sums are exact in any order, so the
// tables do not depend on the order the waves run in.  The softmax is softmax_backup's (f64, from the f32 logits l);
// the entropy is log(sum x) - sum x_a d_a / sum x with d_a = l_a - max, so a zero probability adds an exact zero and
// huge logits give no NaN.  keep(col) is 1 - sum of the collected objects' p_terminate held to [0, 1], the env's own
// behaviour (a bernoulli(p) with p >= 1 always terminates); the backward kernels follow the reference's DP and do
// not clamp.
__device__ __forceinline__ void occupancy_step(const OptretSetup& T, unsigned long long* da, int nxo, int pos, int e,
                                               const float* l, double m, double (&acc)[OCC_SUMS],
                                               unsigned long long* colsum) {
  const int G2 = T.G2;
  // the largest logit's action i1 and the second-largest's i2 (another maximum, if there is one), found on the f32
  // logits: exp is monotone, so x[i1] = exp(0) = 1 is the largest x and x[i2] the second-largest
  int i1 = 0;
  float mx = l[0];
#pragma unroll
  for (int a = 1; a < 5; ++a)
    if (l[a] > mx) { mx = l[a]; i1 = a; }
  int i2 = i1 == 0 ? 1 : 0;
  float m2 = i1 == 0 ? l[1] : l[0];
#pragma unroll
  for (int a = 1; a < 5; ++a)
    if (a != i1 && l[a] > m2) { m2 = l[a]; i2 = a; }
  double x[5], den = 0.0, xd = 0.0, sec = 0.0;
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    const double d = (double)l[a] - (double)mx;
    x[a] = exp(d);
    den += x[a];
    xd += x[a] * d;
    sec = a == i2 ? x[a] : sec;
  }
  const double inv = 1.0 / den;
  acc[OCC_ENT] += m * (log(den) - xd * inv);
  acc[OCC_LC] += m * (1.0 - inv);
  acc[OCC_MM] += m * (1.0 - (inv - sec * inv));
  const int absent = T.used & ~e;
  const double* pwa = T.pw + absent * T.NE;
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    const uint32_t en = T.nxt[pos * 5 + a];
    const int col = (int)(en >> 8) & e;
    const double w = m * (x[a] * inv);
    double keep = 1.0;
    if (col != 0) {
      const double r = T.rsum[col], kw = T.keepw[col];
      keep = kw < 0.0 ? 0.0 : (kw > 1.0 ? 1.0 : kw);
      acc[OCC_RET] += w * r;
      acc[OCC_RABS] += w * fabs(r);
      const unsigned long long ft = (unsigned long long)(w * (1.0 - keep) * kOccOne);
      if (ft != 0) atomicAdd(colsum + TOUED_MAX_OBJS, ft);
      const unsigned long long f = (unsigned long long)(w * kColOne);
      for (int c = col; c != 0; c &= c - 1) atomicAdd(colsum + __builtin_ctz(c), f);
    }
    const double wk = w * keep;
    if (!(wk > 0.0)) continue;
    unsigned long long* dst = da + nxo + (int)(en & 0xFFu) + G2 * (e & ~col);   // an outcome adds G2 * R
    int R = 0;
    do {
      const unsigned long long f = (unsigned long long)(wk * pwa[R] * kOccOne);
      if (f != 0) atomicAdd(dst + G2 * R, f);
      R = (R - absent) & absent;
    } while (R != 0);
  }
}

// State occupancy of a tabular agent's own policy, the forward counterpart of k_policy_return:
//   d_0 = 1 at (start cell, all used objects present),   d_{t+1}(s') = sum_s d_t(s) sum_a pi_t(a|s) P(s' | s, a)
// for t = 0 .. H-1, d_t(s) = P(the first episode is still running at step t and is in state s).  k_policy_return's
// setup, work order, block size and theta rows in registers; the two LDS tables hold d_t and d_{t+1} as u64 fixed
// point (occupancy_step).  A thread reads only its own entries of the current table and clears each right after
// reading it, so the table is clean when it becomes the next step's target: one LDS barrier per step.  A state without
// mass does no work, so the early steps cost what the reachable front contains.  Results are bit-identical from run
// to run and do not depend on the other levels of the batch: the tables are integer sums, a thread's f64 sums run in
// its own fixed order, and they are combined once, by a fixed tree (wave butterflies, then the waves in order).
// Outputs (f32, one rounding each): summary[8] (toued.h), visits[s] = sum_t d_t(s) (0 at the invalid states),
// collected[o] = the expected collections of object o, and the optional rows occ_all[t] = d_t, stored from the table
// before the step clears it (one more barrier per step) with zero rows for t >= H.
template <int ITEMS>
__global__ __launch_bounds__(1024) void k_policy_occupancy(const int* __restrict__ levels,
                                                           const float* __restrict__ theta, int D, int max_grid,
                                                           int n_max, int L, float* __restrict__ summary,
                                                           float* __restrict__ visits, float* __restrict__ collected,
                                                           float* __restrict__ occ_all) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ double s_part[16][OCC_SUMS];      // a wave's sums; at most 16 waves
  __shared__ double s_tot[OCC_SUMS];
  __shared__ unsigned long long s_col[TOUED_MAX_OBJS + 1];      // collections; the early-termination mass
  const OptretSetup T = optret_setup(smem, levels, max_grid, n_max, L, occ_all);
  const int S = T.S, G2 = T.G2;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int nwork = T.ncell * T.ne;      // <= S <= ITEMS * blockDim (the host's choice of ITEMS)
  unsigned long long* const da = reinterpret_cast<unsigned long long*>(T.va);
  // both tables as fixed-point zeros (the setup's f64 fill has -inf at the invalid states), d_0 at the start state
  const int start = T.lev[L_START] + G2 * T.used;
  for (int s = tid; s < 2 * S; s += nt) da[s] = (s == start && T.H > 0) ? (1ull << 62) : 0ull;
  if (tid <= TOUED_MAX_OBJS) s_col[tid] = 0ull;
  float last[5], row[ITEMS][5];
  int st[ITEMS];
  policy_items(T, theta + (size_t)blockIdx.x * D * 5, D, nwork, last, st, row);
  __syncthreads();

  double acc[OCC_SUMS], vis[ITEMS];
#pragma unroll
  for (int i = 0; i < OCC_SUMS; ++i) acc[i] = 0.0;
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) vis[k] = 0.0;
  int curo = 0;    // d_t, read and cleared
  int nxo = S;     // d_{t+1}, added to
  for (int t = 0; t < T.H; ++t) {
    if (occ_all != nullptr) {
      float* out = occ_all + ((size_t)blockIdx.x * L + t) * S;
      for (int s = tid; s < S; s += nt) out[s] = (float)((double)da[curo + s] * kOccInv);
      lds_barrier();      // the row is read before its entries' owners clear them
    }
    const float c = __fmul_rn((float)t, 0.001f);
    float tl[5];
#pragma unroll
    for (int a = 0; a < 5; ++a) tl[a] = __fmul_rn(c, last[a]);
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
      if (st[k] < 0) continue;
      int sk = st[k];
      asm volatile("" : "+v"(sk));      // as in k_policy_moments: what derives from the item is formed per step
      const int pos = sk & 0xFF, e = sk >> 8;
      const int si = curo + pos + G2 * e;
      const unsigned long long u = da[si];
      if (u == 0) continue;
      da[si] = 0;
      const double m = (double)u * kOccInv;
      vis[k] += m;
      float l[5];
#pragma unroll
      for (int a = 0; a < 5; ++a) l[a] = __fadd_rn(row[k][a], tl[a]);
      occupancy_step(T, da, nxo, pos, e, l, m, acc, s_col);
    }
    lds_barrier();
    const int sw = curo; curo = nxo; nxo = sw;
  }
  // table curo holds d_H
#pragma unroll
  for (int k = 0; k < ITEMS; ++k)
    if (st[k] >= 0) {
      acc[OCC_ALIVE] += (double)da[curo + (st[k] & 0xFF) + G2 * (st[k] >> 8)] * kOccInv;
      acc[OCC_LEN] += vis[k];
    }

  if (visits != nullptr) {
    float* out = visits + (size_t)blockIdx.x * S;
    const int g = T.lev[L_GRID], g2 = g * g;
    for (int s = tid; s < S; s += nt) {      // the invalid states, which no thread owns
      const int pos = s % G2, e = s / G2;
      if (!(pos < g2 && !wall_at(T.lev, pos) && !(e & ~T.used))) out[s] = 0.0f;
    }
#pragma unroll
    for (int k = 0; k < ITEMS; ++k)
      if (st[k] >= 0) out[(st[k] & 0xFF) + G2 * (st[k] >> 8)] = (float)vis[k];
  }

  // the block's sums: a butterfly inside each wave, then the waves in order
#pragma unroll
  for (int i = 0; i < OCC_SUMS; ++i) {
    double v = acc[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((tid & 63) == 0) s_part[tid >> 6][i] = v;
  }
  __syncthreads();
  if (tid < OCC_SUMS) {
    double v = 0.0;
    for (int w = 0; w < (nt >> 6); ++w) v += s_part[w][tid];
    s_tot[tid] = v;
  }
  __syncthreads();
  if (tid < 8) {
    const double len = s_tot[OCC_LEN];
    double v = tid == OCC_PTERM ? (double)s_col[TOUED_MAX_OBJS] * kOccInv : s_tot[tid];
    if (tid == OCC_ENT) v = len > 0.0 ? v / (len * log(5.0)) : 0.0;
    if (tid == OCC_LC || tid == OCC_MM) v = len > 0.0 ? v / len : 0.0;
    summary[(size_t)blockIdx.x * 8 + tid] = (float)v;
  }
  if (collected != nullptr && tid < n_max)
    collected[(size_t)blockIdx.x * n_max + tid] = (float)((double)s_col[tid] * kColInv);
}

// Raises kernel K's dynamic-LDS limit on its first launch, then launches it: one workgroup of `block` threads per
// level.  `who` is the entry point, for the messages.
template <auto K, class... Args>
int optret_launch(const char* who, int n, int block, size_t lds, hipStream_t stream, Args... args) {
  static bool attr_set = false;
  if (!attr_set) {
    TOUED_REQUIRE(hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)kOptretLdsMax) == hipSuccess,
                  "%s: cannot raise the dynamic LDS limit", who);
    attr_set = true;
  }
  hipLaunchKernelGGL(K, dim3(n), dim3(block), lds, stream, args...);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) {      // TOUED_CHECK_LAUNCH under the entry point's name: -2, a launch failure
    toued::set_error("%s: launch failed: %s", who, hipGetErrorString(err));
    return -2;
  }
  return 0;
}

// launch(integral_constant<int, I>) for the fewest work items per thread I of 1, 2, 4, 6 that hold `items`
template <class Launch>
int by_items(int items, Launch launch) {
  if (items <= 1) return launch(std::integral_constant<int, 1>{});
  if (items <= 2) return launch(std::integral_constant<int, 2>{});
  if (items <= 4) return launch(std::integral_constant<int, 4>{});
  return launch(std::integral_constant<int, 6>{});      // every mode's table
}

// block size from the table size: one state per thread up to 1024 threads
int optret_block(int S) { return S <= 64 ? 64 : (S <= 256 ? 256 : (S <= 1024 ? 512 : 1024)); }

// The entry points' argument checks.  `who` is the entry point; D is null where there is no theta; lds_bytes is the
// kernel's dynamic LDS, returned in *lds.
int optret_check(const char* who, int tabular, int n, int max_rollout_len, int max_grid, int n_max, const int* D,
                 size_t (*lds_bytes)(int, int), size_t* lds) {
  TOUED_REQUIRE(tabular != 0, "%s: non-tabular environments are unsupported (%s)", who,
                D == nullptr ? "the reference raises NotImplementedError"
                             : "the agent is not a table over the environment's states");
  TOUED_REQUIRE(n >= 0 && max_rollout_len >= 0, "%s: n=%d max_rollout_len=%d must be >= 0", who, n, max_rollout_len);
  TOUED_REQUIRE(max_grid >= 1 && max_grid <= 16, "%s: max_grid=%d outside [1, 16]", who, max_grid);
  TOUED_REQUIRE(n_max >= 0 && n_max <= TOUED_MAX_OBJS, "%s: n_max=%d outside [0, %d]", who, n_max, TOUED_MAX_OBJS);
  const int G2 = max_grid * max_grid;
  const int S = G2 << n_max;
  TOUED_REQUIRE(D == nullptr || *D == S + 1, "%s: D=%d is not max_grid^2 * 2^n_max + 1 = %d", who, *D, S + 1);
  *lds = lds_bytes(G2, n_max);
  TOUED_REQUIRE(*lds <= kOptretLdsMax, "%s: max_grid=%d n_max=%d needs %zu bytes of LDS (limit %zu)", who, max_grid,
                n_max, *lds, kOptretLdsMax);
  return 0;
}

}  // namespace

extern "C" {

int toued_optimal_return(const int* levels, int n, int max_grid, int n_max, int tabular, int max_rollout_len,
                         float* v0, float* v_all, hipStream_t stream) {
  size_t lds;
  if (optret_check(__func__, tabular, n, max_rollout_len, max_grid, n_max, nullptr, optret_lds_bytes, &lds)) return -1;
  if (n == 0) return 0;
  const int block = optret_block((max_grid * max_grid) << n_max);
  return optret_launch<k_optimal_return>(__func__, n, block, lds, stream, levels, max_grid, n_max, max_rollout_len,
                                         v0, v_all);
}

int toued_policy_return(const int* levels, const float* theta, int n, int D, int max_grid, int n_max, int tabular,
                        int max_rollout_len, float* v0, float* v_all, hipStream_t stream) {
  const char* const who = __func__;
  size_t lds;
  if (optret_check(who, tabular, n, max_rollout_len, max_grid, n_max, &D, optret_lds_bytes, &lds)) return -1;
  if (n == 0) return 0;
  // the kernel is instantiated for the work items a thread can own at k_optimal_return's block size, and once more
  // for the tables past six items per thread
  const int S = D - 1, block = optret_block(S), items = (S + block - 1) / block;
  const auto launch = [&](auto I, auto more) {
    return optret_launch<k_policy_return<decltype(I)::value, decltype(more)::value>>(
        who, n, block, lds, stream, levels, theta, D, max_grid, n_max, max_rollout_len, v0, v_all);
  };
  if (items <= 6) return by_items(items, [&](auto I) { return launch(I, std::false_type{}); });      // every mode
  return launch(std::integral_constant<int, 4>{}, std::true_type{});
}

int toued_policy_return_moments(const int* levels, const float* theta, int n, int D, int max_grid, int n_max,
                                int tabular, int max_rollout_len, float* v0, float* var0, float* v_all,
                                float* var_all, hipStream_t stream) {
  // the f32 variance tables come on top of toued_policy_return's LDS: the limit on the table size is lower here
  const char* const who = __func__;
  size_t lds;
  if (optret_check(who, tabular, n, max_rollout_len, max_grid, n_max, &D, polmom_lds_bytes, &lds)) return -1;
  if (n == 0) return 0;
  // toued_policy_return's block size and items per thread; a table that fits the LDS has at most six
  const int S = D - 1, block = optret_block(S), items = (S + block - 1) / block;
  TOUED_REQUIRE(items <= 6, "%s: max_grid=%d n_max=%d has %d states per thread (limit 6)", who, max_grid, n_max,
                items);
  return by_items(items, [&](auto I) {
    return optret_launch<k_policy_moments<decltype(I)::value>>(who, n, block, lds, stream, levels, theta, D, max_grid,
                                                               n_max, max_rollout_len, v0, var0, v_all, var_all);
  });
}

int toued_policy_occupancy(const int* levels, const float* theta, int n, int D, int max_grid, int n_max, int tabular,
                           int max_rollout_len, float* summary, float* visits, float* collected, float* occ_all,
                           hipStream_t stream) {
  const char* const who = __func__;
  size_t lds;
  if (optret_check(who, tabular, n, max_rollout_len, max_grid, n_max, &D, optret_lds_bytes, &lds)) return -1;
  if (n == 0) return 0;
  TOUED_REQUIRE(summary != nullptr, "%s: summary is required", who);
  // toued_policy_return's LDS, block size and items per thread; every mode's table has at most six
  const int S = D - 1, block = optret_block(S), items = (S + block - 1) / block;
  TOUED_REQUIRE(items <= 6, "%s: max_grid=%d n_max=%d has %d states per thread (limit 6)", who, max_grid, n_max,
                items);
  return by_items(items, [&](auto I) {
    return optret_launch<k_policy_occupancy<decltype(I)::value>>(who, n, block, lds, stream, levels, theta, D,
                                                                 max_grid, n_max, max_rollout_len, summary, visits,
                                                                 collected, occ_all);
  });
}

}  // extern "C"
