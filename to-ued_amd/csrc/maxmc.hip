// MaxMC PLR score of a batch of eval trajectories (the maximum Monte Carlo regret estimate of Jiang et al. 2021,
// "Replay-Guided Adversarial Environment Design") — HIP for gfx950.
//
// Per agent a (the layout, the chunked walk and the reduction: trajscore_dev.h):
//   v        = vcrit[a][idx] + ((float)time * 0.001f) * vcrit[a][D-1]      the value critic of k_value_loss_scores
//   per worker, forward in time:  cum = cum + disc * r;  disc = disc * gamma;  on done: best = max(best, cum),
//                                 cum = 0, disc = 1;  after the last step an unfinished episode's cum counts too
//   wmax[a][w] = best,   rmax_out[a] = max(rmax_in[a], max_w wmax[a][w]),
//   score[a]   = rmax_out[a] - mean over (w, t < T) of v
// in f32 with separate roundings (this file is compiled with -ffp-contract=off), so wmax and rmax_out are bit-identical
// to the sequential restatement.  13 bytes per (worker, step) are read once and nothing but the outputs is written.
//
//   * Only the returns' three-operation recurrence is sequential.  Time is walked forward.  For a chunk every thread
//     gathers the values of its pairs into its f64 partial sum and stages (r, done) in LDS; then thread w runs worker
//     w's chain from LDS, carrying cum, disc, best and open.
//   * The staging buffers are double: a chunk needs one barrier, between its staging and its walk.
//   * The mean of v is taken from (double)rmax_out before the one rounding to f32.
#include "trajscore_dev.h"

namespace {

using namespace trajscore;

// dynamic LDS: float rbuf[2][chunk]; float vrow[D rounded up to 4]; uint8_t dbuf[2][chunk]
inline size_t maxmc_lds_bytes(int D) {
  return 2 * (size_t)kChunk * (sizeof(float) + sizeof(uint8_t)) + (((size_t)D + 3) & ~(size_t)3) * sizeof(float);
}

// One worker's walk over the `rows` steps of a chunk, first step first: r[j * Wt], d[j * Wt] of step j
TOUED_DEV void walk_chunk(const float* r, const uint8_t* d, int Wt, int rows, float gamma, float& cum, float& disc,
                          float& best, bool& open) {
  chain4<true>(rows, [&](int, float rv, uint8_t dv) {
    cum = cum + disc * rv;
    disc = disc * gamma;
    open = dv == 0;
    if (dv) {
      best = fmaxf(best, cum);
      cum = 0.0f;
      disc = 1.0f;
    }
  }, [&](int j) { return r[j * Wt]; }, [&](int j) { return d[j * Wt]; });
}

__global__ void __launch_bounds__(kThreads) k_max_mc_scores(
    int W, int T, int D, const float* __restrict__ vcrit, const int* __restrict__ tidx,
    const int* __restrict__ ttime, const float* __restrict__ trew, const uint8_t* __restrict__ tdone, float gamma,
    const float* __restrict__ rmax_in, float* __restrict__ score, float* __restrict__ rmax_out,
    float* __restrict__ wmax) {
  extern __shared__ __align__(16) unsigned char smem[];
  float* rbuf = reinterpret_cast<float*>(smem);
  float* vrow = rbuf + 2 * kChunk;
  uint8_t* dbuf = reinterpret_cast<uint8_t*>(vrow + ((D + 3) & ~3));
  __shared__ double red[kThreads];
  __shared__ float redm[kThreads];

  const int a = blockIdx.x, tid = threadIdx.x;
  const size_t ob = (size_t)a * (T + 1) * W, sb = (size_t)a * T * W;
  const CriticRow value = stage_critic_row(vrow, vcrit + (size_t)a * D, D, tid);

  double sv = 0.0;
  float lvl = -__builtin_inff();
  for (int w0 = 0; w0 < W; w0 += kThreads) {
    const int Wt = W - w0 < kThreads ? W - w0 : kThreads;
    const int C = kChunk / Wt;           // steps per chunk (>= 8)
    unsigned rel[kPairs];
    int ri[kPairs], rt[kPairs];
    float rr[kPairs];
    uint8_t rd[kPairs];
    tile_rel(rel, W, w0, Wt, tid);
    auto load = [&](int lo, int rows) {
      tile_load(tidx, ttime, trew, tdone, ob, sb, W, w0, Wt, tid, rel, lo, rows, ri, rt, rr, rd);
    };
    int lo = 0, rows = T < C ? T : C, cur = 0;
    load(lo, rows);
    float cum = 0.0f, disc = 1.0f, best = -__builtin_inff();
    bool open = false;
    for (;;) {
      const int n = rows * Wt;
      float* rb = rbuf + cur * kChunk;
      uint8_t* db = dbuf + cur * kChunk;
      // entries past the chunk's end (e >= n) of rb and db are written too, and read by nobody
#pragma unroll
      for (int i = 0; i < kPairs; ++i) {
        const int e = i * kThreads + tid;
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
  block_reduce<kThreads, 1, true>(red, redm, tid);
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
  const int go = trajscore_check("toued_max_mc_scores", N, W, T, D, kMaxD, "a critic row", "entries");
  if (go <= 0) return go;
  TOUED_REQUIRE(vcrit && tidx && ttime && trew && tdone, "toued_max_mc_scores: null input buffer");
  TOUED_REQUIRE(score && rmax_out, "toued_max_mc_scores: null score or rmax_out");
  hipLaunchKernelGGL(k_max_mc_scores, dim3(N), dim3(kThreads), maxmc_lds_bytes(D), stream, W, T, D, vcrit, tidx,
                     ttime, trew, tdone, gamma, rmax_in, score, rmax_out, wmax);
  TOUED_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
