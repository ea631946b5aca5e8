// Value-loss PLR scores of a batch of eval trajectories (Prioritized Level Replay's positive value loss and L1 value
// loss) — HIP for gfx950.
//
// Per agent a, on the trajectory layout toued_rollout writes (tidx / ttime [N][T+1][W], trew / tdone [N][T][W]):
//   v     = vcrit[a][idx] + ((float)time * 0.001f) * vcrit[a][D-1]        the value critic of k_eval_loss
//   delta = r + (gamma * v[t+1] * nd - v[t]);   g = delta + gamma_lambda * nd * g        the scan of k_gae
//   pvl[a] = mean over (w, t) of max(g, 0),   l1[a] = mean of |g|
// in f32 with separate roundings (this file is compiled with -ffp-contract=off), so g is bit-identical to toued_gae
// on the gathered values.  13 bytes per (worker, step) are read once and nothing but the two scores is written
// (plus g, when the caller asks for it).
//
//   * One workgroup of 256 threads per agent.  The agent's critic row is staged in LDS once (at most 21.6 KB, the
//     `tabular` mode) and the value gather reads it from there.
//   * Only g's two-operation recurrence is sequential.  Time is walked from the end in chunks of at most 2048
//     (worker, step) pairs, 8 per thread, whole rows of up to 256 workers each (W = 64: 32 steps).  For a chunk every
//     thread gathers the values of its pairs into LDS, then -- once the chunk's values are all there -- forms delta and
//     gamma_lambda * nd of its pairs, both independent of g, into LDS; then thread w runs worker w's scan over the
//     chunk's steps, one LDS read, one multiply and one add per step on the chain.  g is carried from chunk to chunk in
//     a register, so the order of operations is the sequential scan's.
//   * The next chunk's 13 bytes per pair are loaded into registers before the scan of the current one, and the two
//     barriers of a chunk wait for LDS only (lds_barrier), so those loads stay in flight across the scan; the waves
//     that have no worker to scan (W < 256) go on to gather the next chunk meanwhile.
//   * v[t+1] of a chunk's last row is the first row of the chunk before it (later in time): it is handed on through
//     a two-slot row in LDS instead of being gathered twice.
//   * W > 256: the workers are taken in tiles of 256, one full time walk per tile.
//   * The two sums are kept in f64 per thread (f32 -> f64 is exact), in the order of the thread's scan, reduced over
//     the 256 threads by a fixed tree in LDS, divided by (double)W * T and rounded to f32 once: no atomics, the same
//     bits on every run, and a function of agent a's rows only.
#include "common.h"

namespace {

constexpr int kVsThreads = 256;
constexpr int kVsPairs = 8;                          // (worker, step) pairs per thread and chunk
constexpr int kVsChunk = kVsThreads * kVsPairs;      // pairs per chunk
constexpr int kVsMaxD = 8192;                        // critic row entries that fit beside the chunk buffers

// dynamic LDS: float2 dc[chunk] (delta, gamma_lambda * nd); float vbuf[chunk]; float vtop[2][threads]; float vrow[D]
inline size_t vscore_lds_bytes(int D) {
  return (size_t)kVsChunk * (sizeof(float2) + sizeof(float)) + 2 * kVsThreads * sizeof(float) +
         (((size_t)D + 3) & ~(size_t)3) * sizeof(float);
}

// One worker's scan over the `rows` steps of a chunk, last step first: x[j * Wt] = (delta, gamma_lambda * nd) of step
// j.  Four steps' LDS reads are issued ahead of their four links of the chain.
template <bool ADV>
TOUED_DEV void scan_chunk(const float2* x, int Wt, int rows, float& g, double& spos, double& sabs, float* ag, int W) {
  auto step = [&](float2 dcv, int j) {
    g = dcv.x + dcv.y * g;
    spos += (double)fmaxf(g, 0.0f);
    sabs += (double)fabsf(g);
    if (ADV) __builtin_nontemporal_store(g, ag + (size_t)j * W);
  };
  int j = rows;
  for (; j >= 4; j -= 4) {
    const float2 x0 = x[(j - 1) * Wt], x1 = x[(j - 2) * Wt], x2 = x[(j - 3) * Wt], x3 = x[(j - 4) * Wt];
    step(x0, j - 1);
    step(x1, j - 2);
    step(x2, j - 3);
    step(x3, j - 4);
  }
  for (; j >= 1; --j) step(x[(j - 1) * Wt], j - 1);
}

__global__ void __launch_bounds__(kVsThreads) k_value_loss_scores(
    int W, int T, int D, const float* __restrict__ vcrit, const int* __restrict__ tidx,
    const int* __restrict__ ttime, const float* __restrict__ trew, const uint8_t* __restrict__ tdone, float gamma,
    float gl, float* __restrict__ pvl, float* __restrict__ l1, float* __restrict__ adv) {
  extern __shared__ __align__(16) unsigned char smem[];
  float2* dc = reinterpret_cast<float2*>(smem);
  float* vbuf = reinterpret_cast<float*>(dc + kVsChunk);
  float* vtop = vbuf + kVsChunk;
  float* vrow = vtop + 2 * kVsThreads;
  __shared__ double red[2][kVsThreads];

  const int a = blockIdx.x, tid = threadIdx.x;
  const float* vg = vcrit + (size_t)a * D;
  for (int i = tid; i < D; i += kVsThreads) vrow[i] = vg[i];
  const size_t ob = (size_t)a * (T + 1) * W, sb = (size_t)a * T * W;
  const unsigned dmax = (unsigned)(D - 1);
  __syncthreads();
  const float vlast = vrow[D - 1];
  // an index outside the row is held to it (no trajectory of toued_rollout has one)
  auto value = [&](int idx, int tm) {
    const unsigned i = (unsigned)idx < dmax ? (unsigned)idx : dmax;
    return vrow[i] + ((float)tm * 0.001f) * vlast;
  };

  double spos = 0.0, sabs = 0.0;
  for (int w0 = 0; w0 < W; w0 += kVsThreads) {
    const int Wt = W - w0 < kVsThreads ? W - w0 : kVsThreads;
    const int C = kVsChunk / Wt;           // steps per chunk (>= 8)
    if (tid < Wt) {
      const size_t o = ob + (size_t)T * W + w0 + tid;
      vtop[tid] = value(tidx[o], ttime[o]);
    }
    // pair e = i * 256 + tid of a chunk is (step lo + e / Wt, worker w0 + e % Wt), rel[i] floats past the chunk's
    // (lo, worker 0): the same for every chunk of the tile
    int rel[kVsPairs];
#pragma unroll
    for (int i = 0; i < kVsPairs; ++i) {
      const int e = i * kVsThreads + tid, j = e / Wt;
      rel[i] = j * W + w0 + (e - j * Wt);
    }
    int cur = 0;
    int ri[kVsPairs], rt[kVsPairs];
    float rr[kVsPairs];
    uint8_t rd[kVsPairs];
    // the raw trajectory of steps [lo, lo + rows) into registers, no branch between the loads: a pair past the
    // chunk's end reads the chunk's first worker instead (in bounds, never used)
    auto load = [&](int lo, int rows) {
      const int n = rows * Wt;
      const size_t base = (size_t)lo * W;
#pragma unroll
      for (int i = 0; i < kVsPairs; ++i) {
        const size_t off = base + (i * kVsThreads + tid < n ? rel[i] : w0);
        ri[i] = __builtin_nontemporal_load(tidx + ob + off);
        rt[i] = __builtin_nontemporal_load(ttime + ob + off);
        rr[i] = __builtin_nontemporal_load(trew + sb + off);
        rd[i] = __builtin_nontemporal_load(tdone + sb + off);
      }
    };
    int lo = T > C ? T - C : 0, rows = T - lo;
    load(lo, rows);
    float g = 0.0f;
    for (;;) {
      const int n = rows * Wt;
      float v[kVsPairs];
      // entries past the chunk's end (e >= n) of vbuf and dc are written too, and read by nobody
#pragma unroll
      for (int i = 0; i < kVsPairs; ++i) {
        v[i] = value(ri[i], rt[i]);
        vbuf[i * kVsThreads + tid] = v[i];
      }
      lds_barrier();   // the chunk's values (and the row handed on) are in LDS; the scan before has read dc
#pragma unroll
      for (int i = 0; i < kVsPairs; ++i) {
        const int e = i * kVsThreads + tid;
        // v[t+1]: the next row of the chunk, or for the chunk's last row the row handed on (vtop follows vbuf)
        const int en = e + Wt < n ? e + Wt : (e < n ? kVsChunk + cur * kVsThreads + (e + Wt - n) : 0);
        const float vn = vbuf[en];
        const float nd = rd[i] ? 0.0f : 1.0f;
        const float delta = rr[i] + (gamma * vn * nd - v[i]);
        dc[e] = make_float2(delta, gl * nd);
      }
      if (tid < Wt) vtop[(cur ^ 1) * kVsThreads + tid] = v[0];   // row lo: v[t+1] of the next chunk's last row
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

  red[0][tid] = spos;
  red[1][tid] = sabs;
  __syncthreads();
  for (int s = kVsThreads / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] += red[0][tid + s];
      red[1][tid] += red[1][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double cnt = (double)W * (double)T;
    if (pvl != nullptr) pvl[a] = (float)(red[0][0] / cnt);
    if (l1 != nullptr) l1[a] = (float)(red[1][0] / cnt);
  }
}

}  // namespace

extern "C" {

int toued_value_loss_scores(int N, int W, int T, int D, const float* vcrit, const int* tidx, const int* ttime,
                            const float* trew, const uint8_t* tdone, float gamma, float gamma_lambda, float* pvl,
                            float* l1, float* adv, hipStream_t stream) {
  TOUED_REQUIRE(N >= 0 && W >= 1 && T >= 1 && D >= 2, "toued_value_loss_scores: N=%d W=%d T=%d D=%d (need N >= 0, "
                "W >= 1, T >= 1, D >= 2)", N, W, T, D);
  TOUED_REQUIRE((long)W * T < (1L << 31), "toued_value_loss_scores: W=%d x T=%d steps per agent, limit 2^31", W, T);
  TOUED_REQUIRE(D <= kVsMaxD, "toued_value_loss_scores: D=%d, a critic row of more than %d entries does not fit in "
                "LDS", D, kVsMaxD);
  if (N == 0) return 0;
  TOUED_REQUIRE(vcrit && tidx && ttime && trew && tdone, "toued_value_loss_scores: null input buffer");
  TOUED_REQUIRE(pvl || l1, "toued_value_loss_scores: pvl and l1 are both null");
  hipLaunchKernelGGL(k_value_loss_scores, dim3(N), dim3(kVsThreads), vscore_lds_bytes(D), stream, W, T, D, vcrit,
                     tidx, ttime, trew, tdone, gamma, gamma_lambda, pvl, l1, adv);
  TOUED_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
