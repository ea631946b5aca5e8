// What the PLR score kernels that walk a batch of eval trajectories share (vscore.hip, maxmc.hip, polscore.hip).
//
// The trajectory layout is toued_rollout's: tidx / ttime [N][T+1][W], trew / tdone [N][T][W].  One workgroup per
// agent; the agent's table row(s) are staged in LDS once and gathered from there.  The two critic kernels
// (k_value_loss_scores, k_max_mc_scores) share one scheme:
//   * 256 threads.  Only a short recurrence per worker is sequential.  Time is walked in chunks of at most 2048
//     (worker, step) pairs, 8 per thread, whole rows of up to 256 workers each (W = 64: 32 steps).  For a chunk every
//     thread turns its pairs into what the recurrence needs and stages that in LDS; then thread w runs worker w's
//     chain over the chunk's steps from LDS (chain4), its state carried from chunk to chunk in registers, so the order
//     of operations is the sequential walk's.
//   * The next chunk's 13 bytes per pair are loaded into registers (tile_load) before the chain of the current
//     one, and the barriers of a chunk wait for LDS only (lds_barrier), so those loads stay in flight across the
//     chain; the waves that have no worker (W < 256) go on to gather the next chunk meanwhile.  Where the load is
//     issued is the kernel's business: it differs with the direction of time.
//   * W > 256: the workers are taken in tiles of 256, one full time walk per tile.
// All three keep their sums in f64 per thread (f32 -> f64 is exact), in the order of the thread's pairs, and reduce
// them over the workgroup by a fixed tree in LDS (block_reduce), to be divided by (double)W * T and rounded to f32
// once: no atomics, the same bits on every run, and a function of agent a's rows only.
#pragma once
#include <array>
#include <tuple>

#include "common.h"

namespace trajscore {

constexpr int kThreads = 256;                    // the critic kernels' workgroup (k_policy_scores has its own 512 / 4)
constexpr int kPairs = 8;                        // (worker, step) pairs per thread and chunk
constexpr int kChunk = kThreads * kPairs;        // pairs per chunk
constexpr int kMaxD = 8192;                      // critic row entries that fit beside the chunk buffers

// An index outside the row is held to it (no trajectory of toued_rollout has one); dmax = D - 1.
TOUED_DEV unsigned clamp_row(int idx, unsigned dmax) { return (unsigned)idx < dmax ? (unsigned)idx : dmax; }

// The agent's critic row in LDS and the value critic of k_eval_loss on it.
struct CriticRow {
  const float* vrow;
  unsigned dmax;
  float vlast;
  TOUED_DEV float operator()(int idx, int tm) const {
    return vrow[clamp_row(idx, dmax)] + ((float)tm * 0.001f) * vlast;
  }
};

// Stages vg[0 .. D) into vrow (every thread of the workgroup calls it; it holds a __syncthreads()).
TOUED_DEV CriticRow stage_critic_row(float* vrow, const float* __restrict__ vg, int D, int tid) {
  for (int i = tid; i < D; i += kThreads) vrow[i] = vg[i];
  __syncthreads();
  return CriticRow{vrow, (unsigned)(D - 1), vrow[D - 1]};
}

// One tile's raw trajectory, a chunk at a time, in registers the kernel declares.  Pair e = i * 256 + tid of a chunk
// is (step lo + e / Wt, worker w0 + e % Wt), rel[i] elements past the chunk's (lo, worker 0): the same for every chunk
// of the tile.  Offsets are unsigned: a pair that a chunk uses has e / Wt < rows <= T, so its rel is below W * T < 2^31
// and no chunk ever relied on a negative one; a pair no chunk uses may wrap, defined and unread.
TOUED_DEV void tile_rel(unsigned (&rel)[kPairs], int W, int w0, int Wt, int tid) {
#pragma unroll
  for (int i = 0; i < kPairs; ++i) {
    const unsigned e = i * kThreads + tid, j = e / Wt;
    rel[i] = j * (unsigned)W + w0 + (e - j * Wt);
  }
}

// steps [lo, lo + rows) of the agent's rows (tidx, ttime at ob; trew, tdone at sb) into ri, rt, rr, rd, no branch
// between the loads: a pair past the chunk's end reads the chunk's first worker instead (in bounds, never used)
TOUED_DEV void tile_load(const int* tidx, const int* ttime, const float* trew, const uint8_t* tdone, size_t ob,
                         size_t sb, int W, int w0, int Wt, int tid, const unsigned (&rel)[kPairs], int lo,
                         int rows, int (&ri)[kPairs], int (&rt)[kPairs], float (&rr)[kPairs], uint8_t (&rd)[kPairs]) {
  const int n = rows * Wt;
  const size_t base = (size_t)lo * W;
#pragma unroll
  for (int i = 0; i < kPairs; ++i) {
    const size_t off = base + (i * kThreads + tid < n ? rel[i] : (unsigned)w0);
    ri[i] = __builtin_nontemporal_load(tidx + ob + off);
    rt[i] = __builtin_nontemporal_load(ttime + ob + off);
    rr[i] = __builtin_nontemporal_load(trew + sb + off);
    rd[i] = __builtin_nontemporal_load(tdone + sb + off);
  }
}

// One worker's chain over the `rows` steps of a chunk, first step first (FWD) or last step first: step(j, read(j)...)
// for every j.  Four steps' LDS reads are issued ahead of their four links of the chain, one `read` after the other.
template <bool FWD, class Step, class... Read>
TOUED_DEV void chain4(int rows, Step step, Read... read) {
  int j = FWD ? 0 : rows;   // FWD: the steps done, else the steps left
  auto at = [&](int i) { return FWD ? j + i : j - 1 - i; };
  auto quad = [&](auto rd) { return std::array<decltype(rd(0)), 4>{rd(at(0)), rd(at(1)), rd(at(2)), rd(at(3))}; };
  for (; FWD ? j + 4 <= rows : j >= 4; j += FWD ? 4 : -4) {
    const auto q = std::make_tuple(quad(read)...);
#pragma unroll
    for (int i = 0; i < 4; ++i) std::apply([&](const auto&... x) { step(at(i), x[i]...); }, q);
  }
  for (; FWD ? j < rows : j >= 1; j += FWD ? 1 : -1) step(at(0), read(at(0))...);
}

// The workgroup's fixed reduction tree over K f64 sums per thread, and with MAX an f32 maximum.  Thread tid has put
// its sums in red[k * THREADS + tid] (static or dynamic LDS) and its maximum in redm[tid] (unused without MAX); the
// results are red[k * THREADS] and redm[0], valid for every thread on return.
template <int THREADS, int K, bool MAX>
TOUED_DEV void block_reduce(double* red, float* redm, int tid) {
  __syncthreads();
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int k = 0; k < K; ++k) red[k * THREADS + tid] += red[k * THREADS + tid + s];
      if (MAX) redm[tid] = fmaxf(redm[tid], redm[tid + s]);
    }
    __syncthreads();
  }
}

// The entry points' argument check: 1 to go on, 0 when there is nothing to do (N == 0: before any pointer is looked
// at), -1 with the error set.  The table that has to fit is `what`, of at most maxD `unit`.
inline int trajscore_check(const char* name, int N, int W, int T, int D, int maxD, const char* what,
                           const char* unit) {
  TOUED_REQUIRE(N >= 0 && W >= 1 && T >= 1 && D >= 2, "%s: N=%d W=%d T=%d D=%d (need N >= 0, W >= 1, T >= 1, D >= 2)",
                name, N, W, T, D);
  TOUED_REQUIRE((long)W * T < (1L << 31), "%s: W=%d x T=%d steps per agent, limit 2^31", name, W, T);
  TOUED_REQUIRE(D <= maxD, "%s: D=%d, %s of more than %d %s does not fit in LDS", name, D, what, maxD, unit);
  return N != 0;
}

}  // namespace trajscore
