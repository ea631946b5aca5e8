// Level reachability statistics (toued_level_stats): which cells of a level the agent can ever stand on, how far
// they are from the start, and whether a positive reward lies within the episode's horizon.  ACCEL's complexity
// metrics (Parker-Holder et al. 2022: shortest path to the goal, number of walls) and the solvability test of the
// level editor's filter.  Not in the reference.
//
// R is the closure of {start} under the environment's own move, next_pos (env_dev.h): a cell c < g^2 whose wall bit
// is clear joins R when a member p of R, p < g^2, moves onto it, i.e. p = c - g (down), p = c + g (up; c + g < g^2),
// p = c - 1 (right; c is not in column 0) or p = c + 1 (left; c is not in column g - 1).  The start is in R whatever
// its own wall bit says (the env puts the agent there); wall bits at cells >= g^2 are never read; a row's last cell
// and the next row's first are not neighbours.  A start cell >= g^2 (a malformed row) stays alone: next_pos is only
// followed inside the grid.
//
// One wave64 per level, kWaves waves per workgroup, no LDS.  The level's 256 cells are four 64-bit words; cell c is
// bit c & 63 of word c >> 6 and belongs to lane c & 63.  The wall words come straight from the record, the other cell
// sets (inside the grid, column 0, column g - 1) are ballots of per-lane predicates, and the reached set is four
// wave-uniform 64-bit words: a round shifts the 256-bit set by +-1 and +-g in scalar registers, masks it with the
// free and column sets and ORs it in; each lane stamps the round number on the cells of its own that the round added
// (the distance map, in registers).  The loop ends when a round adds nothing: at most g^2 - 1 rounds add a cell, so
// 256 bounds it.  No global access inside the loop.
#include "common.h"

namespace {

constexpr int kWaves = 4;            // waves (levels) per workgroup
constexpr int kStatWords = 16;       // TOUED_LSTAT_WORDS
enum { ST_CELLS = 0, ST_N_WALLS, ST_N_REACH, ST_ECC, ST_N_OBJ_REACH, ST_N_POS_REACH, ST_NEAREST_POS, ST_SOLVABLE,
       ST_OBJ_DIST = 8 };

static_assert(ST_OBJ_DIST + TOUED_MAX_OBJS == kStatWords, "one OBJ_DIST word per object");

struct Set256 {
  uint64_t w[4];
};

// cells c with c - s in x (1 <= s <= 63)
TOUED_DEV Set256 shl256(const Set256& x, int s) {
  Set256 r;
  r.w[0] = x.w[0] << s;
#pragma unroll
  for (int k = 1; k < 4; ++k) r.w[k] = (x.w[k] << s) | (x.w[k - 1] >> (64 - s));
  return r;
}
// cells c with c + s in x
TOUED_DEV Set256 shr256(const Set256& x, int s) {
  Set256 r;
#pragma unroll
  for (int k = 0; k < 3; ++k) r.w[k] = (x.w[k] >> s) | (x.w[k + 1] << (64 - s));
  r.w[3] = x.w[3] >> s;
  return r;
}

__global__ void __launch_bounds__(64 * kWaves) k_level_stats(const int* __restrict__ levels, int n, int max_grid,
                                                             int max_n_objs, int* __restrict__ stats,
                                                             int* __restrict__ dist) {
  const int lane = threadIdx.x & 63;
  // wave-uniform by construction: made so for the compiler, which then keeps the record and the sets in SGPRs
  const int lvl = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
  if (lvl >= n) return;
  const int* __restrict__ lev = levels + (size_t)lvl * LEVEL_WORDS;
  const int G2 = max_grid * max_grid;
  // the fields that index anything, held to the mode's static bounds as optret_setup holds them
  int g = lev[L_GRID];
  g = g < 1 ? 1 : (g > max_grid ? max_grid : g);
  int nobj = lev[L_NOBJS];
  nobj = nobj < 0 ? 0 : (nobj > max_n_objs ? max_n_objs : nobj);
  int start = lev[L_START];
  start = start < 0 ? 0 : (start >= G2 ? G2 - 1 : start);
  const int g2 = g * g;
  const int max_steps = lev[L_MAX_STEPS];
  const bool randresp = lev[L_RANDRESP] != 0;

  Set256 wall, grid, col0, colN;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    wall.w[k] = (uint64_t)(uint32_t)lev[L_WALLS + 2 * k] | ((uint64_t)(uint32_t)lev[L_WALLS + 2 * k + 1] << 32);
    const int c = lane + 64 * k, col = c % g;
    grid.w[k] = __ballot(c < g2);
    col0.w[k] = __ballot(col == 0);
    colN.w[k] = __ballot(col == g - 1);
  }
  Set256 reach, free_;
  int n_walls = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    free_.w[k] = grid.w[k] & ~wall.w[k];
    n_walls += __builtin_popcountll(grid.w[k] & wall.w[k]);
    reach.w[k] = (start >> 6) == k ? (uint64_t)1 << (start & 63) : (uint64_t)0;
  }
  int d[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) d[k] = (lane + 64 * k == start && start < g2) ? 0 : -1;

  int ecc = 0;
  for (int r = 1; r <= 256; ++r) {
    Set256 src, dn, up, rt, lf;
#pragma unroll
    for (int k = 0; k < 4; ++k) src.w[k] = reach.w[k] & grid.w[k];
    dn = shl256(src, g);
    up = shr256(src, g);
    rt = shl256(src, 1);
    lf = shr256(src, 1);
    uint64_t any = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint64_t nw = (dn.w[k] | up.w[k] | (rt.w[k] & ~col0.w[k]) | (lf.w[k] & ~colN.w[k])) & free_.w[k] &
                          ~reach.w[k];
      reach.w[k] |= nw;
      any |= nw;
      if ((nw >> lane) & 1) d[k] = r;
    }
    if (any == 0) break;
    ecc = r;
  }

  int n_reach = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) n_reach += __builtin_popcountll(reach.w[k]);

  // the objects: static cells (wave-uniform), their distance read from the lane that owns the cell
  int od[TOUED_MAX_OBJS];
  int n_obj_reach = 0, n_pos_reach = 0, nearest = -1;
#pragma unroll
  for (int i = 0; i < TOUED_MAX_OBJS; ++i) {
    const int cell = lev[L_STATIC + i];
    const bool in = i < nobj && !randresp && cell >= 0 && cell < g2;
    const int c = in ? cell : 0;                 // c < g2 <= 256: a valid word and lane whatever the record holds
    const int kk = c >> 6;
    int dk = d[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) dk = kk == k ? d[k] : dk;
    const int dc = __builtin_amdgcn_readlane(dk, c & 63);
    const int di = in ? dc : -1;
    od[i] = di;
    const bool pos = __int_as_float(lev[L_REW + i]) > 0.0f;
    if (di >= 0) {
      ++n_obj_reach;
      if (pos) {
        ++n_pos_reach;
        nearest = (nearest < 0 || di < nearest) ? di : nearest;
      }
    }
  }
  int solvable = (nearest >= 0 && (nearest > 1 ? nearest : 1) <= max_steps) ? 1 : 0;
  if (randresp) solvable = -1;

  // lane j < 16 writes word j: one 64-byte store per level
  const int head[ST_OBJ_DIST] = {g2, n_walls, n_reach, ecc, n_obj_reach, n_pos_reach, nearest, solvable};
  int word = 0;
#pragma unroll
  for (int j = 0; j < ST_OBJ_DIST; ++j) {
    word = lane == j ? head[j] : word;
    word = lane == ST_OBJ_DIST + j ? od[j] : word;
  }
  if (lane < kStatWords) stats[(size_t)lvl * kStatWords + lane] = word;
  if (dist != nullptr) {
    int* drow = dist + (size_t)lvl * G2;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (lane + 64 * k < G2) drow[lane + 64 * k] = d[k];
  }
}

}  // namespace

extern "C" {

int toued_level_stats(const int* levels, int n, int max_grid, int max_n_objs, int* stats, int* dist,
                      hipStream_t stream) {
  TOUED_REQUIRE(n >= 0, "toued_level_stats: n=%d must be >= 0", n);
  TOUED_REQUIRE(max_grid >= 1 && max_grid <= 16, "toued_level_stats: max_grid=%d: max_grid^2 outside [1, 256]",
                max_grid);
  TOUED_REQUIRE(max_n_objs >= 0 && max_n_objs <= TOUED_MAX_OBJS, "toued_level_stats: max_n_objs %d outside [0, %d]",
                max_n_objs, TOUED_MAX_OBJS);
  if (n == 0) return 0;
  TOUED_REQUIRE(levels != nullptr && stats != nullptr, "toued_level_stats: levels and stats must not be NULL (n=%d)",
                n);
  hipLaunchKernelGGL(k_level_stats, dim3((n + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, stream, levels, n,
                     max_grid, max_n_objs, stats, dist);
  TOUED_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
