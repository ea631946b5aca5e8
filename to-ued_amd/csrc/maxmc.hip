// MaxMC PLR score of a batch of eval trajectories (the maximum Monte Carlo regret estimate of Jiang et al. 2021,
// "Replay-Guided Adversarial Environment Design") — HIP for gfx950.
//
// Per agent a, on the trajectory layout toued_rollout writes (tidx / ttime [N][T+1][W], trew / tdone [N][T][W]):
//   v        = vcrit[a][idx] + ((float)time * 0.001f) * vcrit[a][D-1]      the value critic of k_value_loss_scores
//   per worker, forward in time:  cum = cum + disc * r;  disc = disc * gamma;  on done: best = max(best, cum),
//                                 cum = 0, disc = 1;  after the last step an unfinished episode's cum counts too
//   wmax[a][w] = best,   rmax_out[a] = max(rmax_in[a], max_w wmax[a][w]),
//   score[a]   = rmax_out[a] - mean over (w, t < T) of v
// in f32 with separate roundings (this file is compiled with -ffp-contract=off), so wmax and rmax_out are bit-identical
// to the sequential restatement.  13 bytes per (worker, step) are read once and nothing but the outputs is written.
//
//   * One workgroup of 256 threads per agent.  The agent's critic row is staged in LDS once and the value gather
//     reads it from there (k_value_loss_scores' layout and limits).
//   * Only the returns' three-operation recurrence is sequential.  Time is walked forward in chunks of at most 2048
//     (worker, step) pairs, 8 per thread, whole rows of up to 256 workers each (W = 64: 32 steps).  For a chunk every
//     thread gathers the values of its pairs into its f64 partial sum and stages (r, done) in LDS; then thread w runs
//     worker w's chain over the chunk's steps from LDS.  cum, disc, best and open are carried from chunk to chunk in
//     registers, so the order of operations is the sequential walk's.
//   * The staging buffers are double: a chunk needs one barrier (LDS only, lds_barrier), between its staging and its
//     scan.  The next chunk's 13 bytes per pair are loaded into registers before the scan of the current one and stay
//     in flight across it; the waves that have no worker to scan (W < 256) go on to gather the next chunk meanwhile.
//   * W > 256: the workers are taken in tiles of 256, one full time walk per tile.
//   * The value sum is kept in f64 per thread (f32 -> f64 is exact), in the order of the thread's pairs, reduced over
//     the 256 threads by a fixed tree in LDS, divided by (double)W * T, taken from (double)rmax_out and rounded to f32
//     once: no atomics, the same bits on every run, and a function of agent a's rows only.
#include "common.h"

namespace {

constexpr int kMcThreads = 256;
constexpr int kMcPairs = 8;                          // (worker, step) pairs per thread and chunk
constexpr int kMcChunk = kMcThreads * kMcPairs;      // pairs per chunk
constexpr int kMcMaxD = 8192;                        // critic row entries (k_value_loss_scores' limit)

// dynamic LDS: float rbuf[2][chunk]; float vrow[D rounded up to 4]; uint8_t dbuf[2][chunk]
inline size_t maxmc_lds_bytes(int D) {
  return 2 * (size_t)kMcChunk * (sizeof(float) + sizeof(uint8_t)) + (((size_t)D + 3) & ~(size_t)3) * sizeof(float);
}

// One worker's walk over the `rows` steps of a chunk, first step first: r[j * Wt], d[j * Wt] of step j.  Four steps'
// LDS reads are issued ahead of their four links of the chain.
TOUED_DEV void walk_chunk(const float* r, const uint8_t* d, int Wt, int rows, float gamma, float& cum, float& disc,
                          float& best, bool& open) {
  auto step = [&](float rv, uint8_t dv) {
    cum = cum + disc * rv;
    disc = disc * gamma;
    open = dv == 0;
    if (dv) {
      best = fmaxf(best, cum);
      cum = 0.0f;
      disc = 1.0f;
    }
  };
  int j = 0;
  for (; j + 4 <= rows; j += 4) {
    const float r0 = r[j * Wt], r1 = r[(j + 1) * Wt], r2 = r[(j + 2) * Wt], r3 = r[(j + 3) * Wt];
    const uint8_t d0 = d[j * Wt], d1 = d[(j + 1) * Wt], d2 = d[(j + 2) * Wt], d3 = d[(j + 3) * Wt];
    step(r0, d0);
    step(r1, d1);
    step(r2, d2);
    step(r3, d3);
  }
  for (; j < rows; ++j) step(r[j * Wt], d[j * Wt]);
}

__global__ void __launch_bounds__(kMcThreads) k_max_mc_scores(
    int W, int T, int D, const float* __restrict__ vcrit, const int* __restrict__ tidx,
    const int* __restrict__ ttime, const float* __restrict__ trew, const uint8_t* __restrict__ tdone, float gamma,
    const float* __restrict__ rmax_in, float* __restrict__ score, float* __restrict__ rmax_out,
    float* __restrict__ wmax) {
  extern __shared__ __align__(16) unsigned char smem[];
  float* rbuf = reinterpret_cast<float*>(smem);
  float* vrow = rbuf + 2 * kMcChunk;
  uint8_t* dbuf = reinterpret_cast<uint8_t*>(vrow + ((D + 3) & ~3));
  __shared__ double red[kMcThreads];
  __shared__ float redm[kMcThreads];

  const int a = blockIdx.x, tid = threadIdx.x;
  const float* vg = vcrit + (size_t)a * D;
  for (int i = tid; i < D; i += kMcThreads) vrow[i] = vg[i];
  const size_t ob = (size_t)a * (T + 1) * W, sb = (size_t)a * T * W;
  const unsigned dmax = (unsigned)(D - 1);
  __syncthreads();
  const float vlast = vrow[D - 1];
  // an index outside the row is held to it (no trajectory of toued_rollout has one)
  auto value = [&](int idx, int tm) {
    const unsigned i = (unsigned)idx < dmax ? (unsigned)idx : dmax;
    return vrow[i] + ((float)tm * 0.001f) * vlast;
  };

  double sv = 0.0;
  float lvl = -__builtin_inff();
  for (int w0 = 0; w0 < W; w0 += kMcThreads) {
    const int Wt = W - w0 < kMcThreads ? W - w0 : kMcThreads;
    const int C = kMcChunk / Wt;           // steps per chunk (>= 8)
    // pair e = i * 256 + tid of a chunk is (step lo + e / Wt, worker w0 + e % Wt), rel[i] elements past the chunk's
    // (lo, worker 0): the same for every chunk of the tile (a pair no chunk uses may wrap: unsigned)
    unsigned rel[kMcPairs];
#pragma unroll
    for (int i = 0; i < kMcPairs; ++i) {
      const unsigned e = i * kMcThreads + tid, j = e / Wt;
      rel[i] = j * (unsigned)W + w0 + (e - j * Wt);
    }
    int ri[kMcPairs], rt[kMcPairs];
    float rr[kMcPairs];
    uint8_t rd[kMcPairs];
    // the raw trajectory of steps [lo, lo + rows) into registers, no branch between the loads: a pair past the
    // chunk's end reads the chunk's first worker instead (in bounds, never used)
    auto load = [&](int lo, int rows) {
      const int n = rows * Wt;
      const size_t base = (size_t)lo * W;
#pragma unroll
      for (int i = 0; i < kMcPairs; ++i) {
        const size_t off = base + (i * kMcThreads + tid < n ? rel[i] : (unsigned)w0);
        ri[i] = __builtin_nontemporal_load(tidx + ob + off);
        rt[i] = __builtin_nontemporal_load(ttime + ob + off);
        rr[i] = __builtin_nontemporal_load(trew + sb + off);
        rd[i] = __builtin_nontemporal_load(tdone + sb + off);
      }
    };
    int lo = 0, rows = T < C ? T : C, cur = 0;
    load(lo, rows);
    float cum = 0.0f, disc = 1.0f, best = -__builtin_inff();
    bool open = false;
    for (;;) {
      const int n = rows * Wt;
      float* rb = rbuf + cur * kMcChunk;
      uint8_t* db = dbuf + cur * kMcChunk;
      // entries past the chunk's end (e >= n) of rb and db are written too, and read by nobody
#pragma unroll
      for (int i = 0; i < kMcPairs; ++i) {
        const int e = i * kMcThreads + tid;
        const float v = value(ri[i], rt[i]);
        if (e < n) sv += (double)v;
        rb[e] = rr[i];
        db[e] = rd[i];
      }
      const int srows = rows;
      lo += rows;
      const bool more = lo < T;
      if (more) {
        rows = T - lo < C ? T - lo : C;
        load(lo, rows);   // in flight across the walk below
      }
      // the chunk's (r, done) are in LDS.  The next chunk is staged in the other buffer, whose last readers (the walk
      // of the chunk before this one) had finished when they arrived at this barrier
      lds_barrier();
      if (tid < Wt) walk_chunk(rb + tid, db + tid, Wt, srows, gamma, cum, disc, best, open);
      if (!more) break;
      cur ^= 1;
    }
    if (tid < Wt) {
      if (open) best = fmaxf(best, cum);   // the unfinished last episode: a truncated return
      lvl = fmaxf(lvl, best);
      if (wmax != nullptr) wmax[(size_t)a * W + w0 + tid] = best;
    }
    lds_barrier();   // this tile's last reads of rbuf and dbuf before the next tile's writes
  }

  red[tid] = sv;
  redm[tid] = lvl;
  __syncthreads();
  for (int s = kMcThreads / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[tid] += red[tid + s];
      redm[tid] = fmaxf(redm[tid], redm[tid + s]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float prior = rmax_in != nullptr ? rmax_in[a] : -__builtin_inff();
    const float rm = fmaxf(prior, redm[0]);
    rmax_out[a] = rm;
    score[a] = (float)((double)rm - red[0] / ((double)W * (double)T));
  }
}

}  // namespace

extern "C" {

int toued_max_mc_scores(int N, int W, int T, int D, const float* vcrit, const int* tidx, const int* ttime,
                        const float* trew, const uint8_t* tdone, float gamma, const float* rmax_in, float* score,
                        float* rmax_out, float* wmax, hipStream_t stream) {
  TOUED_REQUIRE(N >= 0 && W >= 1 && T >= 1 && D >= 2, "toued_max_mc_scores: N=%d W=%d T=%d D=%d (need N >= 0, "
                "W >= 1, T >= 1, D >= 2)", N, W, T, D);
  TOUED_REQUIRE((long)W * T < (1L << 31), "toued_max_mc_scores: W=%d x T=%d steps per agent, limit 2^31", W, T);
  TOUED_REQUIRE(D <= kMcMaxD, "toued_max_mc_scores: D=%d, a critic row of more than %d entries does not fit in LDS",
                D, kMcMaxD);
  if (N == 0) return 0;
  TOUED_REQUIRE(vcrit && tidx && ttime && trew && tdone, "toued_max_mc_scores: null input buffer");
  TOUED_REQUIRE(score && rmax_out, "toued_max_mc_scores: null score or rmax_out");
  hipLaunchKernelGGL(k_max_mc_scores, dim3(N), dim3(kMcThreads), maxmc_lds_bytes(D), stream, W, T, D, vcrit, tidx,
                     ttime, trew, tdone, gamma, rmax_in, score, rmax_out, wmax);
  TOUED_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
