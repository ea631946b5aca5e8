// Episode statistics of a batch of train trajectories, carried across the update boundaries of a lifetime (the
// sampled learning curve of the meta-test, toued/evaluate.py) — HIP for gfx950.
//
// Per agent a and worker w (the layout, the chunked walk and the reduction: trajscore_dev.h), first step first:
//   run_ret = run_ret + r_t  (f32, one rounding);  run_len = run_len + 1
//   on done_t: the episode (run_ret, run_len) is recorded and both are cleared
// run_ret / run_len [N][W] come in as the carry of the call before (zero at the start of a lifetime) and go out as
// the carry of the next: episodes do not end where a train rollout ends.  Per agent, added to stats[a][0..6):
//   episodes recorded, sum of their returns, sum of their squared returns, sum of their lengths, sum of all rewards,
//   steps (W * T).
// The f32 running sum in time order is the contract: run_ret and run_len are bit-identical to the sequential
// restatement, and a call on T1 + T2 steps leaves the carry of a call on T1 steps followed by one on T2 steps.
//
//   * 5 bytes per (worker, step) are read once: trew and tdone, no observation.
//   * For a chunk every thread adds its pairs' rewards to its f64 reward sum and stages (r, done) in LDS; then thread
//     w runs worker w's chain from LDS, carrying run_ret and run_len in registers.  The staging buffers are double: a
//     chunk needs one barrier, and the next chunk's loads are in flight across the chain.
//   * The sums are f64 per thread (f32 -> f64 and the square of an f32 in f64 are exact), the counts integers, reduced
//     by block_reduce's fixed tree: no atomics, the same bits on every run, a function of agent a's rows only.
#include "trajscore_dev.h"

namespace {

using namespace trajscore;

constexpr int kCols = 6;   // stats columns
constexpr int kSums = 5;   // of which reduced over the workgroup (steps is W * T)

// steps [lo, lo + rows) of the agent's trew / tdone rows (at sb) into rr, rd: tile_load without the observations
TOUED_DEV void tile_load_rd(const float* trew, const uint8_t* tdone, size_t sb, int W, int w0, int Wt, int tid,
                            const unsigned (&rel)[kPairs], int lo, int rows, float (&rr)[kPairs],
                            uint8_t (&rd)[kPairs]) {
  const int n = rows * Wt;
  const size_t base = sb + (size_t)lo * W;
#pragma unroll
  for (int i = 0; i < kPairs; ++i) {
    const size_t off = base + (i * kThreads + tid < n ? rel[i] : (unsigned)w0);
    rr[i] = __builtin_nontemporal_load(trew + off);
    rd[i] = __builtin_nontemporal_load(tdone + off);
  }
}

__global__ void __launch_bounds__(kThreads) k_episode_stats(
    int W, int T, const float* __restrict__ trew, const uint8_t* __restrict__ tdone, float* __restrict__ run_ret,
    int* __restrict__ run_len, double* __restrict__ stats) {
  __shared__ __align__(16) float rbuf[2 * kChunk];
  __shared__ __align__(16) uint8_t dbuf[2 * kChunk];
  __shared__ double red[kSums * kThreads];

  const int a = blockIdx.x, tid = threadIdx.x;
  const size_t sb = (size_t)a * T * W;

  double s_ret = 0.0, s_sq = 0.0, s_rew = 0.0;
  long long s_len = 0;
  int s_eps = 0;
  for (int w0 = 0; w0 < W; w0 += kThreads) {
    const int Wt = W - w0 < kThreads ? W - w0 : kThreads;
    const int C = kChunk / Wt;           // steps per chunk (>= 8)
    unsigned rel[kPairs];
    float rr[kPairs];
    uint8_t rd[kPairs];
    tile_rel(rel, W, w0, Wt, tid);
    int lo = 0, rows = T < C ? T : C, cur = 0;
    tile_load_rd(trew, tdone, sb, W, w0, Wt, tid, rel, lo, rows, rr, rd);
    float ret = 0.0f;
    int len = 0;
    if (tid < Wt) {
      ret = run_ret[(size_t)a * W + w0 + tid];
      len = run_len[(size_t)a * W + w0 + tid];
    }
    for (;;) {
      const int n = rows * Wt;
      float* rb = rbuf + cur * kChunk;
      uint8_t* db = dbuf + cur * kChunk;
      // entries past the chunk's end (e >= n) of rb and db are written too, and read by nobody
#pragma unroll
      for (int i = 0; i < kPairs; ++i) {
        const int e = i * kThreads + tid;
        if (e < n) s_rew += (double)rr[i];
        rb[e] = rr[i];
        db[e] = rd[i];
      }
      const int srows = rows;
      lo += rows;
      const bool more = lo < T;
      if (more) {
        rows = T - lo < C ? T - lo : C;
        tile_load_rd(trew, tdone, sb, W, w0, Wt, tid, rel, lo, rows, rr, rd);   // in flight across the walk below
      }
      // the chunk's (r, done) are in LDS.  The next chunk is staged in the other buffer, whose last readers (the walk
      // of the chunk before this one) had finished when they arrived at this barrier
      lds_barrier();
      if (tid < Wt) {
        const float* r = rb + tid;
        const uint8_t* d = db + tid;
        chain4<true>(srows, [&](int, float rv, uint8_t dv) {
          ret = ret + rv;
          len = len + 1;
          if (dv) {
            s_eps += 1;
            s_ret += (double)ret;
            s_sq += (double)ret * (double)ret;
            s_len += len;
            ret = 0.0f;
            len = 0;
          }
        }, [&](int j) { return r[j * Wt]; }, [&](int j) { return d[j * Wt]; });
      }
      if (!more) break;
      cur ^= 1;
    }
    if (tid < Wt) {
      run_ret[(size_t)a * W + w0 + tid] = ret;
      run_len[(size_t)a * W + w0 + tid] = len;
    }
    lds_barrier();   // this tile's last reads of rbuf and dbuf before the next tile's writes
  }

  // the counts are integers below 2^53: exact in f64, in any order
  red[0 * kThreads + tid] = (double)s_eps;
  red[1 * kThreads + tid] = s_ret;
  red[2 * kThreads + tid] = s_sq;
  red[3 * kThreads + tid] = (double)s_len;
  red[4 * kThreads + tid] = s_rew;
  block_reduce<kThreads, kSums, false>(red, nullptr, tid);
  if (tid < kCols) {
    const double add = tid < kSums ? red[tid * kThreads] : (double)W * (double)T;
    stats[(size_t)a * kCols + tid] += add;
  }
}

}  // namespace

extern "C" {

int toued_episode_stats(int N, int W, int T, const float* trew, const uint8_t* tdone, float* run_ret, int* run_len,
                        double* stats, hipStream_t stream) {
  TOUED_REQUIRE(N >= 0 && W >= 1 && T >= 1, "toued_episode_stats: N=%d W=%d T=%d (need N >= 0, W >= 1, T >= 1)", N, W,
                T);
  TOUED_REQUIRE((long)W * T < (1L << 31), "toued_episode_stats: W=%d x T=%d steps per agent, limit 2^31", W, T);
  if (N == 0) return 0;
  TOUED_REQUIRE(trew && tdone, "toued_episode_stats: null input buffer");
  TOUED_REQUIRE(run_ret && run_len && stats, "toued_episode_stats: null run_ret, run_len or stats");
  hipLaunchKernelGGL(k_episode_stats, dim3(N), dim3(kThreads), 0, stream, W, T, trew, tdone, run_ret, run_len, stats);
  TOUED_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
