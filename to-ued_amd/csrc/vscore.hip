// Value-loss PLR scores of a batch of eval trajectories (Prioritized Level Replay's positive value loss and L1 value
// loss) — HIP for gfx950.
//
// Per agent a (the layout, the chunked walk and the reduction: trajscore_dev.h):
//   v     = vcrit[a][idx] + ((float)time * 0.001f) * vcrit[a][D-1]        the value critic of k_eval_loss
//   delta = r + (gamma * v[t+1] * nd - v[t]);   g = delta + gamma_lambda * nd * g        the scan of k_gae
//   pvl[a] = mean over (w, t) of max(g, 0),   l1[a] = mean of |g|
// in f32 with separate roundings (this file is compiled with -ffp-contract=off), so g is bit-identical to toued_gae
// on the gathered values.  13 bytes per (worker, step) are read once and nothing but the two scores is written
// (plus g, when the caller asks for it).
//
//   * Only g's two-operation recurrence is sequential.  Time is walked from the end.  For a chunk every thread
//     gathers the values of its pairs into LDS, then -- once the chunk's values are all there -- forms delta and
//     gamma_lambda * nd of its pairs, both independent of g, into LDS; then thread w runs worker w's scan: one LDS
//     read, one multiply and one add per step on the chain.  Two barriers per chunk.
//   * v[t+1] of a chunk's last row is the first row of the chunk before it (later in time): it is handed on through
//     a two-slot row in LDS instead of being gathered twice.
#include "trajscore_dev.h"

namespace {

using namespace trajscore;

// dynamic LDS: float2 dc[chunk] (delta, gamma_lambda * nd); float vbuf[chunk]; float vtop[2][threads]; float vrow[D]
inline size_t vscore_lds_bytes(int D) {
  return (size_t)kChunk * (sizeof(float2) + sizeof(float)) + 2 * kThreads * sizeof(float) +
         (((size_t)D + 3) & ~(size_t)3) * sizeof(float);
}

// One worker's scan over the `rows` steps of a chunk, last step first: x[j * Wt] = (delta, gamma_lambda * nd) of step j
template <bool ADV>
TOUED_DEV void scan_chunk(const float2* x, int Wt, int rows, float& g, double& spos, double& sabs, float* ag, int W) {
  chain4<false>(rows, [&](int j, float2 dcv) {
    g = dcv.x + dcv.y * g;
    spos += (double)fmaxf(g, 0.0f);
    sabs += (double)fabsf(g);
    if (ADV) __builtin_nontemporal_store(g, ag + (size_t)j * W);
  }, [&](int j) { return x[j * Wt]; });
}

__global__ void __launch_bounds__(kThreads) k_value_loss_scores(
    int W, int T, int D, const float* __restrict__ vcrit, const int* __restrict__ tidx,
    const int* __restrict__ ttime, const float* __restrict__ trew, const uint8_t* __restrict__ tdone, float gamma,
    float gl, float* __restrict__ pvl, float* __restrict__ l1, float* __restrict__ adv) {
  extern __shared__ __align__(16) unsigned char smem[];
  float2* dc = reinterpret_cast<float2*>(smem);
  float* vbuf = reinterpret_cast<float*>(dc + kChunk);
  float* vtop = vbuf + kChunk;
  float* vrow = vtop + 2 * kThreads;
  __shared__ double red[2 * kThreads];

  const int a = blockIdx.x, tid = threadIdx.x;
  const size_t ob = (size_t)a * (T + 1) * W, sb = (size_t)a * T * W;
  const CriticRow value = stage_critic_row(vrow, vcrit + (size_t)a * D, D, tid);

  double spos = 0.0, sabs = 0.0;
  for (int w0 = 0; w0 < W; w0 += kThreads) {
    const int Wt = W - w0 < kThreads ? W - w0 : kThreads;
    const int C = kChunk / Wt;           // steps per chunk (>= 8)
    if (tid < Wt) {
      const size_t o = ob + (size_t)T * W + w0 + tid;
      vtop[tid] = value(tidx[o], ttime[o]);
    }
    unsigned rel[kPairs];
    int ri[kPairs], rt[kPairs];
    float rr[kPairs];
    uint8_t rd[kPairs];
    tile_rel(rel, W, w0, Wt, tid);
    auto load = [&](int lo, int rows) {
      tile_load(tidx, ttime, trew, tdone, ob, sb, W, w0, Wt, tid, rel, lo, rows, ri, rt, rr, rd);
    };
    int cur = 0;
    int lo = T > C ? T - C : 0, rows = T - lo;
    load(lo, rows);
    float g = 0.0f;
    for (;;) {
      const int n = rows * Wt;
      float v[kPairs];
      // entries past the chunk's end (e >= n) of vbuf and dc are written too, and read by nobody
#pragma unroll
      for (int i = 0; i < kPairs; ++i) {
        v[i] = value(ri[i], rt[i]);
        vbuf[i * kThreads + tid] = v[i];
      }
      lds_barrier();   // the chunk's values (and the row handed on) are in LDS; the scan before has read dc
#pragma unroll
      for (int i = 0; i < kPairs; ++i) {
        const int e = i * kThreads + tid;
        // v[t+1]: the next row of the chunk, or for the chunk's last row the row handed on (vtop follows vbuf)
        const int en = e + Wt < n ? e + Wt : (e < n ? kChunk + cur * kThreads + (e + Wt - n) : 0);
        const float vn = vbuf[en];
        const float nd = rd[i] ? 0.0f : 1.0f;
        const float delta = rr[i] + (gamma * vn * nd - v[i]);
        dc[e] = make_float2(delta, gl * nd);
      }
      if (tid < Wt) vtop[(cur ^ 1) * kThreads + tid] = v[0];   // row lo: v[t+1] of the next chunk's last row
      const int slo = lo, srows = rows;
      const bool more = lo > 0;
      if (more) {
        rows = lo > C ? C : lo;
        lo -= rows;
        load(lo, rows);   // in flight across the scan below
      }
      lds_barrier();   // delta and gamma_lambda * nd of the chunk are in LDS
      if (tid < Wt) {
        float* ag = adv != nullptr ? adv + sb + (size_t)slo * W + w0 + tid : nullptr;
        if (adv != nullptr) scan_chunk<true>(dc + tid, Wt, srows, g, spos, sabs, ag, W);
        else scan_chunk<false>(dc + tid, Wt, srows, g, spos, sabs, ag, W);
      }
      if (!more) break;
      cur ^= 1;
    }
    lds_barrier();   // this tile's last reads of vtop and dc before the next tile's writes
  }

  red[tid] = spos;
  red[kThreads + tid] = sabs;
  block_reduce<kThreads, 2, false>(red, nullptr, tid);
  if (tid == 0) {
    const double cnt = (double)W * (double)T;
    if (pvl != nullptr) pvl[a] = (float)(red[0] / cnt);
    if (l1 != nullptr) l1[a] = (float)(red[kThreads] / cnt);
  }
}

}  // namespace

extern "C" {

int toued_value_loss_scores(int N, int W, int T, int D, const float* vcrit, const int* tidx, const int* ttime,
                            const float* trew, const uint8_t* tdone, float gamma, float gamma_lambda, float* pvl,
                            float* l1, float* adv, hipStream_t stream) {
  const int go = trajscore_check("toued_value_loss_scores", N, W, T, D, kMaxD, "a critic row", "entries");
  if (go <= 0) return go;
  TOUED_REQUIRE(vcrit && tidx && ttime && trew && tdone, "toued_value_loss_scores: null input buffer");
  TOUED_REQUIRE(pvl || l1, "toued_value_loss_scores: pvl and l1 are both null");
  hipLaunchKernelGGL(k_value_loss_scores, dim3(N), dim3(kThreads), vscore_lds_bytes(D), stream, W, T, D, vcrit,
                     tidx, ttime, trew, tdone, gamma, gamma_lambda, pvl, l1, adv);
  TOUED_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
