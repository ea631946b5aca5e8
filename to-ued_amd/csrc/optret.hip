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
// k_policy_return (further down) is the same recursion for the expected return of a tabular agent's own policy,
// v_t(s) = sum_a pi_t(a|s) q(s, a), on the same setup (optret_setup).  k_policy_moments (after it) adds the variance
// of that return, u_t(s) = Var[G_t | s], in two f32 tables behind the setup's LDS.
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

__global__ void k_optimal_return(const int* __restrict__ levels, int max_grid, int n_max, int L,
                                 float* __restrict__ v0, float* __restrict__ v_all) {
  extern __shared__ __align__(16) unsigned char smem[];
  const OptretSetup T = optret_setup(smem, levels, max_grid, n_max, L, v_all);
  double* const va = T.va;
  const double *pw = T.pw, *rsum = T.rsum, *keepw = T.keepw;
  const int* lev = T.lev;
  const uint16_t* nxt = T.nxt;
  const uint8_t *cells = T.cells, *eord = T.eord;
  const int G2 = T.G2, S = T.S, NE = T.NE, used = T.used, ne = T.ne, H = T.H;
  const int tid = threadIdx.x, nt = blockDim.x;
  const float ninf = -__builtin_inff();

  const int ncell = T.ncell;
  const int nwork = ncell * ne;
  int curo = 0;    // v_t, written: table va (offset 0) or vb (offset S) of the 2S-entry array
  int nxo = S;     // v_{t+1}, read
  for (int t = H - 1; t >= 0; --t) {
    for (int w = tid; w < nwork; w += nt) {
      const int ei = w / ncell;
      const int e = eord[ei], pos = cells[w - ei * ncell];
      const int absent = used & ~e;
      const double* pwa = pw + absent * NE;
      int base[5];
      double r[5], keep[5], ev[5];
#pragma unroll
      for (int a = 0; a < 5; ++a) {
        const uint32_t en = nxt[pos * 5 + a];
        const int c = (int)(en >> 8) & e;
        base[a] = nxo + (int)(en & 0xFFu) + G2 * (e & ~c);
        r[a] = rsum[c];
        keep[a] = keepw[c];
        ev[a] = 0.0;
      }
      // the subsets R of `absent`, two per round: one weight read serves the five actions, and the ten value reads
      // of a round are independent.  Every value read is a valid state's (finite), so a zero weight gives a zero
      // term without a test; a second subset that does not exist reads subset 0 with weight 0.
      int R0 = 0;
      do {
        const int R1 = (R0 - absent) & absent;
        const double p0 = pwa[R0];
        const double p1 = pw[R1 != 0 ? absent * NE + R1 : NE * NE];   // pw[NE * NE] = 0
        const int o0 = G2 * R0, o1 = G2 * R1;
        double x0[5], x1[5];
#pragma unroll
        for (int a = 0; a < 5; ++a) { x0[a] = va[base[a] + o0]; x1[a] = va[base[a] + o1]; }
        __builtin_amdgcn_sched_barrier(0);   // all twelve reads in flight before the first fma waits
#pragma unroll
        for (int a = 0; a < 5; ++a) ev[a] = __builtin_fma(p1, x1[a], __builtin_fma(p0, x0[a], ev[a]));
        R0 = R1 != 0 ? (R1 - absent) & absent : 0;
      } while (R0 != 0);
      double best = (double)ninf;
#pragma unroll
      for (int a = 0; a < 5; ++a) {
        const double q = r[a] + ev[a] * keep[a];
        best = q > best ? q : best;
      }
      va[curo + pos + G2 * e] = best;
    }
    lds_barrier();
    if (v_all != nullptr) {
      float* row = v_all + ((size_t)blockIdx.x * L + t) * S;
      for (int s = tid; s < S; s += nt) row[s] = (float)va[curo + s];
    }
    const int sw = curo; curo = nxo; nxo = sw;
  }
  // table nxo now holds v_0 (v0 is 0 when H == 0, whatever the start cell)
  if (tid == 0) v0[blockIdx.x] = H > 0 ? (float)va[nxo + lev[L_START] + G2 * used] : 0.0f;
}

// One policy backup: v_t(pos, e) = sum_a pi(a) q(s, a) into table `curo`, with the policy's f32 logits l[5] (as
// actor_probs5 forms them) and k_optimal_return's outcome loop on table `nxo`.  The softmax is exp(l - max) / sum in
// f64; the argmax term is exp(0) = 1, so the sum is >= 1: huge logits give an exact one-hot policy and no NaN.
__device__ __forceinline__ void policy_backup(const OptretSetup& T, int nxo, int curo, int pos, int e,
                                              const float* l) {
  double* const va = T.va;
  const double* pw = T.pw;
  const int G2 = T.G2, NE = T.NE;
  const int absent = T.used & ~e;
  const double* pwa = pw + absent * NE;
  int base[5], col[5];
  double ev[5];
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    const uint32_t en = T.nxt[pos * 5 + a];
    col[a] = (int)(en >> 8) & e;
    base[a] = nxo + (int)(en & 0xFFu) + G2 * (e & ~col[a]);
    ev[a] = 0.0;
  }
  int R0 = 0;
  do {
    const int R1 = (R0 - absent) & absent;
    const double p0 = pwa[R0];
    const double p1 = pw[R1 != 0 ? absent * NE + R1 : NE * NE];   // pw[NE * NE] = 0
    const int o0 = G2 * R0, o1 = G2 * R1;
    double x0[5], x1[5];
#pragma unroll
    for (int a = 0; a < 5; ++a) { x0[a] = va[base[a] + o0]; x1[a] = va[base[a] + o1]; }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int a = 0; a < 5; ++a) ev[a] = __builtin_fma(p1, x1[a], __builtin_fma(p0, x0[a], ev[a]));
    R0 = R1 != 0 ? (R1 - absent) & absent : 0;
  } while (R0 != 0);
  float m = l[0];
#pragma unroll
  for (int a = 1; a < 5; ++a) m = fmaxf(m, l[a]);
  double num = 0.0, den = 0.0;
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    const double x = exp((double)l[a] - (double)m);
    const double q = T.rsum[col[a]] + ev[a] * T.keepw[col[a]];
    den += x;
    num = __builtin_fma(x, q, num);
  }
  va[curo + pos + G2 * e] = num / den;
}

// Exact expected return of a tabular agent's own policy: k_optimal_return's recursion with
//   v_t(s) = sum_a pi_t(a|s) q(s, a),   pi_t(.|s) = softmax(theta[s] + fl(fl(t * 0.001) * theta[D-1]))
// in place of the max.  The logits are formed in f32 by actor_probs5's two rounded operations; the softmax and the
// backup are f64.  One workgroup per (level, table) pair with the setup, work order and outcome loop above.  Work item
// w belongs to thread w % blockDim at every step, so a thread reads the theta rows of its first ITEMS items once,
// before the time loop, and keeps them in registers (the item loop is unrolled over ITEMS, so the rows are not
// runtime-indexed).  Every mode's table has at most 6 items per thread and runs with MORE = false: theta is not read
// inside the time loop.  MORE = true serves larger tables, which no mode has: the items past the first ITEMS go
// through a plain loop that reads their rows from global memory at every step.
template <int ITEMS, bool MORE>
__global__ __launch_bounds__(1024) void k_policy_return(const int* __restrict__ levels,
                                                        const float* __restrict__ theta, int D, int max_grid,
                                                        int n_max, int L, float* __restrict__ v0,
                                                        float* __restrict__ v_all) {
  extern __shared__ __align__(16) unsigned char smem[];
  const OptretSetup T = optret_setup(smem, levels, max_grid, n_max, L, v_all);
  const double* va = T.va;
  const int G2 = T.G2, S = T.S, H = T.H;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int ncell = T.ncell;
  const int nwork = ncell * T.ne;      // <= S; <= ITEMS * blockDim without MORE (the host's choice of ITEMS)

  const float* th = theta + (size_t)blockIdx.x * D * 5;
  float last[5];
#pragma unroll
  for (int a = 0; a < 5; ++a) last[a] = th[(size_t)(D - 1) * 5 + a];
  int st[ITEMS];          // pos | e << 8 of the thread's item k, -1 past the level's work
  float row[ITEMS][5];
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const int w = tid + k * nt;
    st[k] = -1;
#pragma unroll
    for (int a = 0; a < 5; ++a) row[k][a] = 0.0f;
    if (w < nwork) {
      const int ei = w / ncell;
      const int e = T.eord[ei], pos = T.cells[w - ei * ncell];
      st[k] = pos | (e << 8);
      const float* r = th + (size_t)(pos + G2 * e) * 5;      // pos + G2 * e < S = D - 1
#pragma unroll
      for (int a = 0; a < 5; ++a) row[k][a] = r[a];
    }
  }

  int curo = 0;    // v_t, written
  int nxo = S;     // v_{t+1}, read
  for (int t = H - 1; t >= 0; --t) {
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
      policy_backup(T, nxo, curo, st[k] & 0xFF, st[k] >> 8, l);
    }
    if (MORE) {
      for (int w = tid + ITEMS * nt; w < nwork; w += nt) {
        const int ei = w / ncell;
        const int e = T.eord[ei], pos = T.cells[w - ei * ncell];
        const float* r = th + (size_t)(pos + G2 * e) * 5;      // pos + G2 * e < S = D - 1
        float l[5];
#pragma unroll
        for (int a = 0; a < 5; ++a) l[a] = __fadd_rn(r[a], tl[a]);
        policy_backup(T, nxo, curo, pos, e, l);
      }
    }
    lds_barrier();
    if (v_all != nullptr) {
      float* out = v_all + ((size_t)blockIdx.x * L + t) * S;
      for (int s = tid; s < S; s += nt) out[s] = (float)va[curo + s];
    }
    const int sw = curo; curo = nxo; nxo = sw;
  }
  if (tid == 0) v0[blockIdx.x] = H > 0 ? (float)va[nxo + T.lev[L_START] + G2 * T.used] : 0.0f;
}

template <int ITEMS, bool MORE>
int launch_policy_return(int n, int block, size_t lds, hipStream_t stream, const int* levels, const float* theta, int D,
                         int max_grid, int n_max, int L, float* v0, float* v_all) {
  static bool attr_set = false;
  if (!attr_set) {
    TOUED_REQUIRE(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_policy_return<ITEMS, MORE>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)kOptretLdsMax) == hipSuccess,
                  "toued_policy_return: cannot raise the dynamic LDS limit");
    attr_set = true;
  }
  hipLaunchKernelGGL((k_policy_return<ITEMS, MORE>), dim3(n), dim3(block), lds, stream, levels, theta, D, max_grid,
                     n_max, L, v0, v_all);
  TOUED_CHECK_LAUNCH();
  return 0;
}

// dynamic LDS of k_policy_moments: optret_setup's layout (a multiple of 16 bytes), then f32 ua[S], ub[S]
__host__ __device__ inline size_t polmom_lds_bytes(int G2, int n_max) {
  return optret_lds_bytes(G2, n_max) + 2 * ((size_t)G2 << n_max) * sizeof(float);
}

// policy_backup with the return's variance beside its mean: v_t(pos, e) into table `curo` of va by policy_backup's
// arithmetic, operation for operation, and u_t(pos, e) = Var[G_t | s] into table `curo` of ua.  With v', u' the
// next state's mean and variance, the second moment of r + cont * G' given (s, a) is
//   m2(s, a) = r^2 + c * (2 r E[v'] + E[u' + v'^2]),   c = 1 - p_term,
// and u_t(s) = sum_a pi(a) m2(s, a) - v_t(s)^2 (the law of total variance, nothing clipped: c < 0 is taken as the
// mean takes it).  u' is read as f32 and everything else is f64; per outcome one more LDS read, u' + v'^2 and one
// more accumulation than the mean's.
__device__ __forceinline__ void moments_backup(const OptretSetup& T, float* ua, int nxo, int curo, int pos, int e,
                                               const float* l) {
  double* const va = T.va;
  const double* pw = T.pw;
  const int G2 = T.G2, NE = T.NE;
  const int absent = T.used & ~e;
  const double* pwa = pw + absent * NE;
  int base[5], col[5];
  double ev[5], ez[5];
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    const uint32_t en = T.nxt[pos * 5 + a];
    col[a] = (int)(en >> 8) & e;
    base[a] = nxo + (int)(en & 0xFFu) + G2 * (e & ~col[a]);
    ev[a] = 0.0;
    ez[a] = 0.0;
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
      y0[a] = ua[base[a] + o0];
      y1[a] = ua[base[a] + o1];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int a = 0; a < 5; ++a) {
      ev[a] = __builtin_fma(p1, x1[a], __builtin_fma(p0, x0[a], ev[a]));
      const double z0 = __builtin_fma(x0[a], x0[a], (double)y0[a]);
      const double z1 = __builtin_fma(x1[a], x1[a], (double)y1[a]);
      ez[a] = __builtin_fma(p1, z1, __builtin_fma(p0, z0, ez[a]));
    }
    R0 = R1 != 0 ? (R1 - absent) & absent : 0;
  } while (R0 != 0);
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
    const double m2 = __builtin_fma(keep, __builtin_fma(r + r, ev[a], ez[a]), r * r);
    num2 = __builtin_fma(x, m2, num2);
  }
  const double v = num / den;
  va[curo + pos + G2 * e] = v;
  ua[curo + pos + G2 * e] = (float)(num2 / den - v * v);
}

// Mean and variance of the first-episode return of a tabular agent's own policy: k_policy_return (its setup, work
// order, block size and mean arithmetic: v0 and v_all are bit-identical to its) with a second table pair for
// u_t(s) = Var[G_t | s], see moments_backup.  The u tables are f32, double-buffered in LDS behind optret_setup's
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
  const double* va = T.va;
  const int G2 = T.G2, S = T.S, H = T.H;
  float* const ua = reinterpret_cast<float*>(smem + optret_lds_bytes(G2, n_max));
  const int tid = threadIdx.x, nt = blockDim.x;
  const int ncell = T.ncell;
  const int nwork = ncell * T.ne;      // <= S <= ITEMS * blockDim (the host's choice of ITEMS)

  // both u tables: u_H = 0 at the valid states, -inf at the invalid ones (va's fill); zero rows of var_all
  for (int s = tid; s < S; s += nt) ua[s] = ua[S + s] = (float)va[s];
  if (var_all != nullptr) {
    float* rows = var_all + ((size_t)blockIdx.x * L + H) * S;
    const size_t nz = (size_t)(L - H) * S;
    for (size_t i = tid; i < nz; i += nt) rows[i] = 0.0f;
  }

  const float* th = theta + (size_t)blockIdx.x * D * 5;
  float last[5];
#pragma unroll
  for (int a = 0; a < 5; ++a) last[a] = th[(size_t)(D - 1) * 5 + a];
  int st[ITEMS];          // pos | e << 8 of the thread's item k, -1 past the level's work
  float row[ITEMS][5];
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const int w = tid + k * nt;
    st[k] = -1;
#pragma unroll
    for (int a = 0; a < 5; ++a) row[k][a] = 0.0f;
    if (w < nwork) {
      const int ei = w / ncell;
      const int e = T.eord[ei], pos = T.cells[w - ei * ncell];
      st[k] = pos | (e << 8);
      const float* r = th + (size_t)(pos + G2 * e) * 5;      // pos + G2 * e < S = D - 1
#pragma unroll
      for (int a = 0; a < 5; ++a) row[k][a] = r[a];
    }
  }
  __syncthreads();

  int curo = 0;    // v_t and u_t, written
  int nxo = S;     // v_{t+1} and u_{t+1}, read
  for (int t = H - 1; t >= 0; --t) {
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
      const int pos = sk & 0xFF, e = sk >> 8;
      float l[5];
#pragma unroll
      for (int a = 0; a < 5; ++a) l[a] = __fadd_rn(row[k][a], tl[a]);
      moments_backup(T, ua, nxo, curo, pos, e, l);
    }
    lds_barrier();
    if (v_all != nullptr) {
      float* out = v_all + ((size_t)blockIdx.x * L + t) * S;
      for (int s = tid; s < S; s += nt) out[s] = (float)va[curo + s];
    }
    if (var_all != nullptr) {
      float* out = var_all + ((size_t)blockIdx.x * L + t) * S;
      for (int s = tid; s < S; s += nt) out[s] = ua[curo + s];
    }
    const int sw = curo; curo = nxo; nxo = sw;
  }
  if (tid == 0) {
    const int si = nxo + T.lev[L_START] + G2 * T.used;
    v0[blockIdx.x] = H > 0 ? (float)va[si] : 0.0f;
    var0[blockIdx.x] = H > 0 ? ua[si] : 0.0f;
  }
}

template <int ITEMS>
int launch_policy_moments(int n, int block, size_t lds, hipStream_t stream, const int* levels, const float* theta,
                          int D, int max_grid, int n_max, int L, float* v0, float* var0, float* v_all,
                          float* var_all) {
  static bool attr_set = false;
  if (!attr_set) {
    TOUED_REQUIRE(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_policy_moments<ITEMS>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)kOptretLdsMax) == hipSuccess,
                  "toued_policy_return_moments: cannot raise the dynamic LDS limit");
    attr_set = true;
  }
  hipLaunchKernelGGL((k_policy_moments<ITEMS>), dim3(n), dim3(block), lds, stream, levels, theta, D, max_grid, n_max,
                     L, v0, var0, v_all, var_all);
  TOUED_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" {

int toued_optimal_return(const int* levels, int n, int max_grid, int n_max, int tabular, int max_rollout_len,
                         float* v0, float* v_all, hipStream_t stream) {
  TOUED_REQUIRE(tabular != 0, "toued_optimal_return: non-tabular environments are unsupported (the reference "
                "raises NotImplementedError)");
  TOUED_REQUIRE(n >= 0 && max_rollout_len >= 0, "toued_optimal_return: n=%d max_rollout_len=%d must be >= 0", n,
                max_rollout_len);
  TOUED_REQUIRE(max_grid >= 1 && max_grid <= 16, "toued_optimal_return: max_grid=%d outside [1, 16]", max_grid);
  TOUED_REQUIRE(n_max >= 0 && n_max <= TOUED_MAX_OBJS, "toued_optimal_return: n_max=%d outside [0, %d]", n_max,
                TOUED_MAX_OBJS);
  const int G2 = max_grid * max_grid;
  const size_t lds = optret_lds_bytes(G2, n_max);
  TOUED_REQUIRE(lds <= kOptretLdsMax, "toued_optimal_return: max_grid=%d n_max=%d needs %zu bytes of LDS (limit %zu)",
                max_grid, n_max, lds, kOptretLdsMax);
  if (n == 0) return 0;
  static bool attr_set = false;
  if (!attr_set) {
    TOUED_REQUIRE(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_optimal_return),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)kOptretLdsMax) == hipSuccess,
                  "toued_optimal_return: cannot raise the dynamic LDS limit");
    attr_set = true;
  }
  // block size from the table size: one state per thread up to 1024 threads
  const int S = G2 << n_max;
  const int block = S <= 64 ? 64 : (S <= 256 ? 256 : (S <= 1024 ? 512 : 1024));
  hipLaunchKernelGGL(k_optimal_return, dim3(n), dim3(block), lds, stream, levels, max_grid, n_max, max_rollout_len,
                     v0, v_all);
  TOUED_CHECK_LAUNCH();
  return 0;
}

int toued_policy_return(const int* levels, const float* theta, int n, int D, int max_grid, int n_max, int tabular,
                        int max_rollout_len, float* v0, float* v_all, hipStream_t stream) {
  TOUED_REQUIRE(tabular != 0, "toued_policy_return: non-tabular environments are unsupported (the agent is not a "
                "table over the environment's states)");
  TOUED_REQUIRE(n >= 0 && max_rollout_len >= 0, "toued_policy_return: n=%d max_rollout_len=%d must be >= 0", n,
                max_rollout_len);
  TOUED_REQUIRE(max_grid >= 1 && max_grid <= 16, "toued_policy_return: max_grid=%d outside [1, 16]", max_grid);
  TOUED_REQUIRE(n_max >= 0 && n_max <= TOUED_MAX_OBJS, "toued_policy_return: n_max=%d outside [0, %d]", n_max,
                TOUED_MAX_OBJS);
  const int G2 = max_grid * max_grid;
  const int S = G2 << n_max;
  TOUED_REQUIRE(D == S + 1, "toued_policy_return: D=%d is not max_grid^2 * 2^n_max + 1 = %d", D, S + 1);
  const size_t lds = optret_lds_bytes(G2, n_max);
  TOUED_REQUIRE(lds <= kOptretLdsMax, "toued_policy_return: max_grid=%d n_max=%d needs %zu bytes of LDS (limit %zu)",
                max_grid, n_max, lds, kOptretLdsMax);
  if (n == 0) return 0;
  // k_optimal_return's block size; the kernel is instantiated for the work items a thread can then own, and once
  // more for the tables past six items per thread
  const int block = S <= 64 ? 64 : (S <= 256 ? 256 : (S <= 1024 ? 512 : 1024));
  const int items = (S + block - 1) / block;
#define TOUED_POLRET_LAUNCH(I, MORE) \
  launch_policy_return<I, MORE>(n, block, lds, stream, levels, theta, D, max_grid, n_max, max_rollout_len, v0, v_all)
  if (items <= 1) return TOUED_POLRET_LAUNCH(1, false);
  if (items <= 2) return TOUED_POLRET_LAUNCH(2, false);
  if (items <= 4) return TOUED_POLRET_LAUNCH(4, false);
  if (items <= 6) return TOUED_POLRET_LAUNCH(6, false);      // every mode's table
  return TOUED_POLRET_LAUNCH(4, true);
#undef TOUED_POLRET_LAUNCH
}

int toued_policy_return_moments(const int* levels, const float* theta, int n, int D, int max_grid, int n_max,
                                int tabular, int max_rollout_len, float* v0, float* var0, float* v_all,
                                float* var_all, hipStream_t stream) {
  TOUED_REQUIRE(tabular != 0, "toued_policy_return_moments: non-tabular environments are unsupported (the agent is "
                "not a table over the environment's states)");
  TOUED_REQUIRE(n >= 0 && max_rollout_len >= 0, "toued_policy_return_moments: n=%d max_rollout_len=%d must be >= 0",
                n, max_rollout_len);
  TOUED_REQUIRE(max_grid >= 1 && max_grid <= 16, "toued_policy_return_moments: max_grid=%d outside [1, 16]",
                max_grid);
  TOUED_REQUIRE(n_max >= 0 && n_max <= TOUED_MAX_OBJS, "toued_policy_return_moments: n_max=%d outside [0, %d]", n_max,
                TOUED_MAX_OBJS);
  const int G2 = max_grid * max_grid;
  const int S = G2 << n_max;
  TOUED_REQUIRE(D == S + 1, "toued_policy_return_moments: D=%d is not max_grid^2 * 2^n_max + 1 = %d", D, S + 1);
  // the f32 variance tables come on top of toued_policy_return's LDS: the limit on the table size is lower here
  const size_t lds = polmom_lds_bytes(G2, n_max);
  TOUED_REQUIRE(lds <= kOptretLdsMax,
                "toued_policy_return_moments: max_grid=%d n_max=%d needs %zu bytes of LDS (limit %zu)", max_grid,
                n_max, lds, kOptretLdsMax);
  if (n == 0) return 0;
  // toued_policy_return's block size and items per thread; a table that fits the LDS has at most six
  const int block = S <= 64 ? 64 : (S <= 256 ? 256 : (S <= 1024 ? 512 : 1024));
  const int items = (S + block - 1) / block;
  TOUED_REQUIRE(items <= 6, "toued_policy_return_moments: max_grid=%d n_max=%d has %d states per thread (limit 6)",
                max_grid, n_max, items);
#define TOUED_POLMOM_LAUNCH(I)                                                                                     \
  launch_policy_moments<I>(n, block, lds, stream, levels, theta, D, max_grid, n_max, max_rollout_len, v0, var0, \
                           v_all, var_all)
  if (items <= 1) return TOUED_POLMOM_LAUNCH(1);
  if (items <= 2) return TOUED_POLMOM_LAUNCH(2);
  if (items <= 4) return TOUED_POLMOM_LAUNCH(4);
  return TOUED_POLMOM_LAUNCH(6);
#undef TOUED_POLMOM_LAUNCH
}

}  // extern "C"
