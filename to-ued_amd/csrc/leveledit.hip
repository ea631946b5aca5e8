// Device level editor: ACCEL (Parker-Holder et al. 2022) for the PLR buffer.  Not in the reference.
//
// A reset slot's replacement level is, with probability p_edit, a few small edits of a high-scoring buffer level (its
// parent, toued_plr_parent_ids) in place of the generator's fresh draw.  One lane per level, as in the generator: the
// work is a short key chain and a handful of words of a 320-byte record, and n is the reset count (<= the buffer).
// The editable fields (start, object cells, wall bitmap, per-type rewards) live in registers; every indexed access is
// an unrolled compare-and-select over the field's fixed size, so a cell or an id outside its range touches nothing.
//
// Key schedule of row j (keys[j] is the generator key of the slot; the generator ran on it, unchanged):
//   ek = fold_in(keys[j], 0x45444954); ek_use, ek_edit = split(ek); use = uniform(ek_use) < p_edit
//   per edit, whatever it ends up doing: rng, k_op = split(rng); rng, k_cell = split(rng); rng, k_obj = split(rng);
//   rng, k_val = split(rng)  (rng starts as ek_edit)
#include "common.h"

namespace {

constexpr uint32_t kEditFold = 0x45444954u;   // "EDIT"
enum { OP_WALLS = 0, OP_OBJECTS = 1, OP_START = 2, OP_REWARDS = 3 };

struct EditLevel {
  int start;
  int cell[TOUED_MAX_OBJS];     // static object cells, all max_n_objs of them
  uint32_t walls[8];
  float trew[TOUED_MAX_TYPES];
};

TOUED_DEV bool wall_at(const EditLevel& l, int c) {
  bool w = false;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if ((c >> 5) == k) w = (l.walls[k] >> (c & 31)) & 1u;
  return w;
}

// the start cell or any of the max_n_objs static object cells
TOUED_DEV bool occupied(const EditLevel& l, int max_n_objs, int c) {
  bool occ = c == l.start;
#pragma unroll
  for (int i = 0; i < TOUED_MAX_OBJS; ++i) occ = occ || (i < max_n_objs && l.cell[i] == c);
  return occ;
}

__global__ void __launch_bounds__(64) k_level_edit(const int* __restrict__ buffer_levels,
                                                   const int* __restrict__ parent_ids,
                                                   const uint32_t* __restrict__ keys, int n, int max_n_objs,
                                                   int max_n_types, float p_edit, int num_edits, int ops_mask,
                                                   float reward_delta, int* __restrict__ levels,
                                                   uint8_t* __restrict__ edited_out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint2 ek = threefry(keys[2 * j], keys[2 * j + 1], 0u, kEditFold);
  uint2 ek_use, rng;
  split2(ek, ek_use, rng);
  const bool use = uniform_from_bits(bits1(ek_use), 0.0f, 1.0f) < p_edit;
  const int pid = parent_ids[j];
  if (!use || pid < 0) {
    if (edited_out) edited_out[j] = 0;
    return;
  }
  const int* par = buffer_levels + (size_t)pid * LEVEL_WORDS;
  int* row = levels + (size_t)j * LEVEL_WORDS;
  const int grid = par[L_GRID], n_objs = par[L_NOBJS];
  int ids[TOUED_MAX_OBJS];
  EditLevel l;
  l.start = par[L_START];
#pragma unroll
  for (int i = 0; i < TOUED_MAX_OBJS; ++i) {
    l.cell[i] = par[L_STATIC + i];
    const int id = par[L_OBJ_IDS + i];
    ids[i] = id < 0 ? id + max_n_types : id;      // as pack_levels resolves it
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) l.walls[k] = (uint32_t)par[L_WALLS + k];
#pragma unroll
  for (int t = 0; t < TOUED_MAX_TYPES; ++t) l.trew[t] = __int_as_float(par[L_TREW + t]);

  const int n_enabled = __builtin_popcount((unsigned)ops_mask);
  bool rew_edited = false;
  for (int e = 0; e < num_edits; ++e) {
    uint2 k_op, k_cell, k_obj, k_val;
    split2(rng, rng, k_op);
    split2(rng, rng, k_cell);
    split2(rng, rng, k_obj);
    split2(rng, rng, k_val);
    int nth = randint0(k_op, (uint32_t)n_enabled), op = 0;
#pragma unroll
    for (int b = 3; b >= 0; --b)      // the nth set bit of ops_mask, ascending
      if (((ops_mask >> b) & 1) && __builtin_popcount((unsigned)ops_mask & ((1u << b) - 1u)) == nth) op = b;
    const int c = randint0(k_cell, (uint32_t)(grid * grid));
    const int o = randint0(k_obj, (uint32_t)(n_objs > 1 ? n_objs : 1));
    const float dv = uniform_from_bits(bits1(k_val), -reward_delta, reward_delta);
    const bool occ = occupied(l, max_n_objs, c), wall = wall_at(l, c);
    if (op == OP_WALLS) {
      if (!occ) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if ((c >> 5) == k) l.walls[k] ^= 1u << (c & 31);
      }
    } else if (op == OP_OBJECTS) {
      if (n_objs > 0 && !wall && !occ) {
#pragma unroll
        for (int i = 0; i < TOUED_MAX_OBJS; ++i)
          if (i == o) l.cell[i] = c;
      }
    } else if (op == OP_START) {
      if (!wall && !occ) l.start = c;
    } else if (n_objs > 0) {
      int t = -1;
#pragma unroll
      for (int i = 0; i < TOUED_MAX_OBJS; ++i)
        if (i == o) t = ids[i];
      const float lo = t == 0 ? 0.0f : -1.0f;
      rew_edited = true;
#pragma unroll
      for (int k = 0; k < TOUED_MAX_TYPES; ++k)
        if (k == t && k < max_n_types) l.trew[k] = fminf(fmaxf(__fadd_rn(l.trew[k], dv), lo), 1.0f);
    }
  }

  const int slot = row[L_BUFID];
  for (int w = 0; w < LEVEL_WORDS; ++w) row[w] = par[w];     // the inherited fields, and the fields edited below
  row[L_BUFID] = slot;
  row[L_START] = l.start;
#pragma unroll
  for (int i = 0; i < TOUED_MAX_OBJS; ++i) {
    if (i < max_n_objs) {
      row[L_STATIC + i] = l.cell[i];
      float r = 0.0f;
#pragma unroll
      for (int k = 0; k < TOUED_MAX_TYPES; ++k)
        if (k == ids[i] && k < max_n_types) r = l.trew[k];
      if (rew_edited) row[L_REW + i] = __float_as_int(r);     // re-resolved through obj_ids from the per-type table
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) row[L_WALLS + k] = (int)l.walls[k];
#pragma unroll
  for (int t = 0; t < TOUED_MAX_TYPES; ++t)
    if (t < max_n_types) row[L_TREW + t] = __float_as_int(l.trew[t]);
  if (edited_out) edited_out[j] = 1;
}

}  // namespace

extern "C" {

int toued_level_edit(const int* buffer_levels, const int* parent_ids, const uint32_t* keys, int n, int max_n_objs,
                     int max_n_types, float p_edit, int num_edits, int ops_mask, float reward_delta,
                     int* levels_inout, uint8_t* edited_out, hipStream_t stream) {
  TOUED_REQUIRE(n >= 0 && num_edits >= 0, "toued_level_edit: n=%d num_edits=%d", n, num_edits);
  TOUED_REQUIRE(ops_mask >= 1 && ops_mask <= 15, "toued_level_edit: ops_mask %d outside [1, 15]", ops_mask);
  TOUED_REQUIRE(p_edit >= 0.0f && p_edit <= 1.0f, "toued_level_edit: p_edit %g outside [0, 1]", (double)p_edit);
  TOUED_REQUIRE(max_n_objs >= 0 && max_n_objs <= TOUED_MAX_OBJS, "toued_level_edit: max_n_objs %d outside [0, %d]",
                max_n_objs, TOUED_MAX_OBJS);
  TOUED_REQUIRE(max_n_types >= 1 && max_n_types <= TOUED_MAX_TYPES,
                "toued_level_edit: max_n_types %d outside [1, %d]", max_n_types, TOUED_MAX_TYPES);
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_level_edit, dim3((n + 63) / 64), dim3(64), 0, stream, buffer_levels, parent_ids, keys, n,
                     max_n_objs, max_n_types, p_edit, num_edits, ops_mask, reward_delta, levels_inout, edited_out);
  TOUED_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
