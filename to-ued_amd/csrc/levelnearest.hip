// Level distance (toued_level_nearest): for each of n query levels the nearest of b corpus levels, which one it is,
// and the sum of the distances -- the duplicate test of the level editor's filter (DCD's level store, jaxued's
// duplicate_check) and the diversity of a level buffer.  Not in the reference.
//
// The canonical record of a packed level is 54 words, exactly what the env and the agent's lifetime read: the six
// scalars (words 0..5; the lifetime reads as 0 without include_lifetime), the five per-object fields of the eight
// slots (words 8..47, a slot i >= clamp(n_objs, 0, 8) reads as 0) and the eight wall words (words 48..55, keeping the
// bits of the cells c < g^2, g = clamp(grid_size, 0, 16); cell c is bit c & 31 of word c >> 5).  Canonical word w is
// source word w (w < 6) or w + 2.  d(a, b) = popcount(walls_a ^ walls_b) + the number of the 46 other canonical words
// that differ: an integer in [0, 302], a Hamming metric on the canonical coordinates, 0 exactly for equal records.
//
// One query per lane, its canonical record in 54 VGPRs; kThreads queries per workgroup.  The corpus goes through LDS
// a tile of kTile canonical records at a time (canonicalised on load, one word per thread and step, so the global
// reads run along the rows); the inner loop reads a record at a wave-uniform address (a broadcast, 14 128-bit reads)
// and compares it with the lane's query: compare-and-add for 46 words, xor and popcount for 8.  Word 54 of a staged
// record is the entry's own eligibility (inside the corpus and corpus_mask set), so a masked entry costs one uniform
// branch.  gridDim.y splits the corpus (n = 512 alone is two workgroups); the parts meet in global memory through
// atomicMin on the key (d << 16) | j -- d <= 302 and j < 65536, so the key is a positive int32 and its minimum is the
// least distance at the lowest index -- and atomicAdd on the sum and the count.  All three are order-independent
// integer operations: results are bit-identical from run to run.  k_nearest_init sets the outputs before, and
// k_nearest_finish splits the key into nn_dist and nn_idx after, on the same stream.  No host synchronisation, no
// floating point.
#include "common.h"
#include <limits.h>

namespace {

constexpr int kThreads = 256;       // queries per workgroup
constexpr int kTile = 64;           // corpus records per LDS tile
constexpr int kCanon = 54;          // canonical words
constexpr int kPlain = 46;          // of them compared for equality (the rest are wall bits)
constexpr int kStride = 56;         // LDS words per record: 54, the eligibility word, one pad (16-byte rows)
constexpr int kTargetBlocks = 1024; // workgroups aimed at when splitting the corpus (256 CUs x 4)
constexpr int kMaxCorpus = 65536;   // j < 2^16 in the key; dist_sum <= 65536 * 302 < 2^31

static_assert(L_OBJ_IDS == 8 && L_PRESP + TOUED_MAX_OBJS == L_WALLS && L_WALLS + 8 == kCanon + 2,
              "canonical word w >= 6 is source word w + 2");
static_assert((kStride * 4) % 16 == 0 && kStride > kCanon, "128-bit LDS rows with room for the eligibility word");

// Canonical value of source word src (0..5, 8..55) holding v, in a level with n_objs held to nobj and g^2 = g2.
TOUED_DEV int canon_word(int src, int v, int nobj, int g2, int include_lifetime) {
  if (src < L_OBJ_IDS) return (src == L_LIFETIME && !include_lifetime) ? 0 : v;
  if (src < L_WALLS) return ((src - L_OBJ_IDS) & (TOUED_MAX_OBJS - 1)) < nobj ? v : 0;
  const int rem = g2 - 32 * (src - L_WALLS);      // cells of this word inside the grid
  const uint32_t keep = rem <= 0 ? 0u : (rem >= 32 ? 0xFFFFFFFFu : (1u << rem) - 1u);
  return (int)((uint32_t)v & keep);
}
TOUED_DEV int held_nobjs(int v) { return v < 0 ? 0 : (v > TOUED_MAX_OBJS ? TOUED_MAX_OBJS : v); }
TOUED_DEV int held_g2(int g) {
  g = g < 0 ? 0 : (g > 16 ? 16 : g);
  return g * g;
}

__global__ void __launch_bounds__(kThreads) k_nearest_init(int n, int* __restrict__ nn_dist, int* __restrict__ nn_idx,
                                                           int* __restrict__ dist_sum, int* __restrict__ count) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  nn_dist[i] = INT_MAX;
  nn_idx[i] = -1;
  dist_sum[i] = 0;
  count[i] = 0;
}

__global__ void __launch_bounds__(kThreads) k_nearest_finish(int n, int* __restrict__ nn_dist,
                                                             int* __restrict__ nn_idx) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int key = nn_dist[i];
  if (key == INT_MAX) return;       // nothing eligible: INT_MAX and -1 stand
  nn_dist[i] = key >> 16;
  nn_idx[i] = key & 0xFFFF;
}

__global__ void __launch_bounds__(kThreads) k_level_nearest(const int* __restrict__ queries, int n,
                                                            const int* __restrict__ corpus, int b,
                                                            const uint8_t* __restrict__ corpus_mask, int eligible,
                                                            int include_lifetime, int tiles_per_part,
                                                            int* __restrict__ nn_key, int* __restrict__ dist_sum,
                                                            int* __restrict__ count) {
  __shared__ __attribute__((aligned(16))) int tile[kTile * kStride];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < n;

  // the lane's query, canonical, in registers (a lane past n holds zeros and writes nothing)
  int q[kCanon];
  {
    const int* __restrict__ row = queries + (size_t)(live ? i : 0) * LEVEL_WORDS;
    const int nobj = held_nobjs(row[L_NOBJS]), g2 = held_g2(row[L_GRID]);
#pragma unroll
    for (int w = 0; w < kCanon; ++w) {
      const int src = w < 6 ? w : w + 2;
      q[w] = canon_word(src, row[src], nobj, g2, include_lifetime);
    }
  }

  int best = INT_MAX, sum = 0, cnt = 0;
  const int n_tiles = (b + kTile - 1) / kTile;
  const int t0 = blockIdx.y * tiles_per_part;
  const int t1 = min(t0 + tiles_per_part, n_tiles);
  for (int t = t0; t < t1; ++t) {
    const int j0 = t * kTile;
    if (t != t0) __syncthreads();                 // the waves are done with the tile before
    // stage: record e's word w at tile[e * kStride + w], w = 54 its eligibility; an entry past the corpus is staged
    // as zeros without reading anything
    for (int x = threadIdx.x; x < kTile * (kCanon + 1); x += kThreads) {
      const int e = x / (kCanon + 1), w = x - e * (kCanon + 1);
      const int j = j0 + e;
      int v = 0;
      if (j < b) {
        const int* __restrict__ row = corpus + (size_t)j * LEVEL_WORDS;
        if (w == kCanon) {
          v = corpus_mask == nullptr ? 1 : (corpus_mask[j] != 0 ? 1 : 0);
        } else {
          const int src = w < 6 ? w : w + 2;
          v = canon_word(src, row[src], held_nobjs(row[L_NOBJS]), held_g2(row[L_GRID]), include_lifetime);
        }
      }
      tile[e * kStride + w] = v;
    }
    __syncthreads();
    for (int e = 0; e < kTile; ++e) {
      if (tile[e * kStride + kCanon] == 0) continue;   // masked out or past the corpus: uniform over the workgroup
      const int4* __restrict__ c4 = reinterpret_cast<const int4*>(tile + e * kStride);   // wave-uniform address
      int c[kStride];
#pragma unroll
      for (int k = 0; k < kStride / 4; ++k) {
        const int4 v = c4[k];
        c[4 * k] = v.x;
        c[4 * k + 1] = v.y;
        c[4 * k + 2] = v.z;
        c[4 * k + 3] = v.w;
      }
      int d = 0;
#pragma unroll
      for (int w = 0; w < kPlain; ++w) d += (q[w] != c[w]) ? 1 : 0;
#pragma unroll
      for (int w = kPlain; w < kCanon; ++w) d += __builtin_popcount((uint32_t)(q[w] ^ c[w]));
      const int j = j0 + e;
      const bool ok = eligible == 0 || (eligible == 1 ? j != i : j < i);
      const int key = (d << 16) | j;
      best = (ok && key < best) ? key : best;
      sum += ok ? d : 0;
      cnt += ok ? 1 : 0;
    }
  }
  if (live && cnt > 0) {
    atomicMin(nn_key + i, best);
    atomicAdd(dist_sum + i, sum);
    atomicAdd(count + i, cnt);
  }
}

}  // namespace

extern "C" {

int toued_level_nearest(const int* queries, int n, const int* corpus, int b, const uint8_t* corpus_mask, int eligible,
                        int include_lifetime, int* nn_dist, int* nn_idx, int* dist_sum, int* count,
                        hipStream_t stream) {
  TOUED_REQUIRE(n >= 0, "toued_level_nearest: n=%d must be >= 0", n);
  TOUED_REQUIRE(b >= 0 && b <= kMaxCorpus, "toued_level_nearest: b=%d outside [0, %d] (dist_sum is an int32)", b,
                kMaxCorpus);
  TOUED_REQUIRE(eligible >= 0 && eligible <= 2, "toued_level_nearest: eligible=%d outside [0, 2]", eligible);
  if (n == 0) return 0;
  TOUED_REQUIRE(nn_dist != nullptr && nn_idx != nullptr && dist_sum != nullptr && count != nullptr,
                "toued_level_nearest: nn_dist, nn_idx, dist_sum and count must not be NULL (n=%d)", n);
  TOUED_REQUIRE(b == 0 || (queries != nullptr && corpus != nullptr),
                "toued_level_nearest: queries and corpus must not be NULL (n=%d, b=%d)", n, b);
  const int xblocks = (n + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(k_nearest_init, dim3(xblocks), dim3(kThreads), 0, stream, n, nn_dist, nn_idx, dist_sum, count);
  TOUED_CHECK_LAUNCH();
  if (b == 0) return 0;
  const int n_tiles = (b + kTile - 1) / kTile;
  int parts = kTargetBlocks / xblocks;
  parts = parts < 1 ? 1 : (parts > n_tiles ? n_tiles : parts);
  const int tiles_per_part = (n_tiles + parts - 1) / parts;
  parts = (n_tiles + tiles_per_part - 1) / tiles_per_part;
  hipLaunchKernelGGL(k_level_nearest, dim3(xblocks, parts), dim3(kThreads), 0, stream, queries, n, corpus, b,
                     corpus_mask, eligible, include_lifetime != 0 ? 1 : 0, tiles_per_part, nn_dist, dist_sum, count);
  TOUED_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_nearest_finish, dim3(xblocks), dim3(kThreads), 0, stream, n, nn_dist, nn_idx);
  TOUED_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
