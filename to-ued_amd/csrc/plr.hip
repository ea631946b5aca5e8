// Prioritised level replay buffer logic (environments/level_sampler.py:169-234, 331-408) — HIP for gfx950.
//
// The buffer (B <= 8192 levels) is small, so each operation is ONE workgroup of 1024 threads that
// keeps its sort keys in LDS: a bitonic sort of 64-bit (order-preserving float bits, index) keys is a
// stable argsort with jax's comparator (lax.sort canonicalises -0 -> +0 and NaN, ties by index).
//
//   k_plr_reset_ids  _reset_lowest_scoring (:338-341): argsort(where(active, inf, where(new, -inf, score)))[:N]
//   k_plr_sample     _replay_from_buffer (:363-385, rank or proportional), _sample_random_from_buffer
//                    (:396-407), and the replay/random selection (:212-227): bernoulli count, the
//                    n_replayable guard, permutation(use_replay), where(use, replay, random)
//   k_plr_sample_prio k_plr_sample with Prioritized Level Replay's replay distribution (not in the reference): the
//                    rank-weighted score part (rank_sampled) and the staleness mixture; the same stages otherwise
//   k_plr_parent_ids the level editor's parents (not in the reference): the scored slots that this round does not
//                    reset, highest score first, dealt round-robin to the reset slots
#include "common.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kMaxSort = 8192;

// Order-preserving map of a float to uint32 after jax's canonicalisation.
TOUED_DEV uint32_t sort_key(float x) {
  if (x == 0.0f) x = 0.0f;
  uint32_t b = __float_as_uint(x);
  if (x != x) b = 0x7FC00000u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// Ascending bitonic sort of s[0..P) (P a power of two), whole block participates.
TOUED_DEV void bitonic(uint64_t* s, int P) {
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < (P >> 1); i += blockDim.x) {
        const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));
        const int hi = lo + j;
        const bool asc = (lo & k) == 0;
        const uint64_t a = s[lo], b = s[hi];
        if ((a > b) == asc) { s[lo] = b; s[hi] = a; }
      }
      __syncthreads();
    }
  }
}

TOUED_DEV int pow2_ceil(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

TOUED_DEV void fill_keys(uint64_t* s, int B, int P, const float* key_of) {
  for (int i = threadIdx.x; i < P; i += blockDim.x)
    s[i] = (i < B) ? (((uint64_t)sort_key(key_of[i]) << 32) | (uint32_t)i) : ~0ull;
}

TOUED_DEV int block_count(bool v, int* red) {
  int c = __builtin_popcountll(__ballot(v));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  int s = 0;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += red[i];
  return s;
}

// -gumbel(key, (B,))[i] - log(p)   (random.choice replace=False, p given: Gumbel top-k)
TOUED_DEV float gumbel_key(uint2 key, int B, int i, float p) {
  const float tiny = 1.17549435e-38f;
  const float u = uniform_from_bits(random_bits_at(key, (uint32_t)B, (uint32_t)i), tiny, 1.0f);
  const float g = -plog(-plog(u));
  return __fsub_rn(-g, plog(p));
}

}  // namespace

__global__ void __launch_bounds__(kThreads) k_plr_reset_ids(int B, int N, const float* __restrict__ score,
                                                            const uint8_t* __restrict__ active,
                                                            const uint8_t* __restrict__ fresh, int* __restrict__ ids) {
  __shared__ uint64_t s[kMaxSort];
  __shared__ float f[kMaxSort];
  const int P = pow2_ceil(B);
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    float x = fresh[i] ? -__builtin_inff() : score[i];
    f[i] = active[i] ? __builtin_inff() : x;
  }
  __syncthreads();
  fill_keys(s, B, P, f);
  bitonic(s, P);
  for (int i = threadIdx.x; i < N; i += blockDim.x) ids[i] = (int)(uint32_t)s[i];
}

namespace {

// ---- the stages of the sample kernels (k_plr_sample, k_plr_sample_prio).  s[kMaxSort], f[kMaxSort] and red[16] are
// the caller's LDS; every stage is entered and left by the whole block.

// Number of slots that cannot be replayed (new or active).
TOUED_DEV int count_invalid(int B, const uint8_t* active, const uint8_t* fresh, int* red) {
  int n_invalid = 0;
  for (int base = 0; base < B; base += blockDim.x) {
    const int i = base + threadIdx.x;
    n_invalid += block_count(i < B && (fresh[i] || active[i]), red);
  }
  return n_invalid;
}

// f[i] = uniform_p ? 1 : f[i] / (f[0] + f[1] + ... in index order) (level_sampler.py:366-372).
TOUED_DEV void normalise(float* f, int B, bool uniform_p, float* total) {
  __syncthreads();
  if (threadIdx.x == 0) {
    float acc = 0.0f;
    for (int i = 0; i < B; ++i) acc = __fadd_rn(acc, f[i]);
    *total = acc;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < B; i += blockDim.x) f[i] = uniform_p ? 1.0f : __fdiv_rn(f[i], *total);
  __syncthreads();
}

// Replay ids from the distribution in f (level_sampler.py:373-385): Gumbel top-k with the second key of
// split(replay_rng), or flip(argsort(p))[:N].  f is overwritten.
TOUED_DEV void replay_pick(uint64_t* s, float* f, int B, int P, int N, uint2 k_rep, bool gumbel, int* rep) {
  const int tid = threadIdx.x;
  if (gumbel) {
    uint2 k0, k1;
    split2(k_rep, k0, k1);
    for (int i = tid; i < B; i += blockDim.x) f[i] = gumbel_key(k1, B, i, f[i]);
    __syncthreads();
    fill_keys(s, B, P, f);
    bitonic(s, P);
    for (int i = tid; i < N; i += blockDim.x) rep[i] = (int)(uint32_t)s[i];
  } else {
    fill_keys(s, B, P, f);
    bitonic(s, P);
    for (int i = tid; i < N; i += blockDim.x) rep[i] = (int)(uint32_t)s[B - 1 - i];  // flip(argsort(p))[:N]
  }
  __syncthreads();
}

// Random new levels (level_sampler.py:396-407).
TOUED_DEV void random_new_ids(uint64_t* s, float* f, int* red, int B, int P, int N, const uint8_t* active,
                              const uint8_t* fresh, uint2 k_rnd, int* rnd) {
  const int tid = threadIdx.x;
  int n_new = 0;
  for (int base = 0; base < B; base += blockDim.x) {
    const int i = base + tid;
    n_new += block_count(i < B && fresh[i] && !active[i], red);
  }
  for (int i = tid; i < B; i += blockDim.x) {
    const float p = __fdiv_rn((fresh[i] && !active[i]) ? 1.0f : 0.0f, (float)n_new);
    f[i] = gumbel_key(k_rnd, B, i, p);
  }
  __syncthreads();
  fill_keys(s, B, P, f);
  bitonic(s, P);
  for (int i = tid; i < N; i += blockDim.x) rnd[i] = (int)(uint32_t)s[i];
  __syncthreads();
}

// Replay / random selection (level_sampler.py:212-227).  Thread i reads back the rep[i] and rnd[i] it wrote itself.
// The block size is read once: left as blockDim.x in the loops of this inlined stage, the shuffle rounds re-derived it
// from the dispatch packet with three dependent loads (+0.5 us per call at B = 4000, N = 512).
TOUED_DEV void select_ids(uint64_t* s, float* f, int* red, int B, int N, int n_invalid, uint2 k_sel, float p_replay,
                          int* chosen, const int* rep, const int* rnd, int* use_out) {
  const int tid = threadIdx.x, nt = blockDim.x;
  uint2 rng1, k_bern, rng2, k_perm;
  split2(k_sel, rng1, k_bern);
  split2(rng1, rng2, k_perm);
  int n_rep = 0;
  for (int base = 0; base < N; base += nt) {
    const int i = base + tid;
    bool b = false;
    if (i < N) b = uniform_from_bits(random_bits_at(k_bern, (uint32_t)N, (uint32_t)i), 0.0f, 1.0f) < p_replay;
    n_rep += block_count(b, red);
  }
  const bool replayable = (B - n_invalid) >= N;
  // permutation(k_perm, use) = jax _shuffle: per round (key, sub) = split(key), stable sort by
  // random_bits(sub, (N,)); ceil(3 ln N / ln(2^32-1)) rounds (1 for N <= ~1.6k).
  int* cur = reinterpret_cast<int*>(f);
  for (int i = tid; i < N; i += nt) cur[i] = i;
  const int rounds = N > 1 ? (int)ceil(3.0 * log((double)N) / log(4294967295.0)) : 0;
  const int PN = pow2_ceil(N);
  uint2 kk = k_perm;
  for (int r = 0; r < rounds; ++r) {
    uint2 knext, ksub;
    split2(kk, knext, ksub);
    kk = knext;
    for (int i = tid; i < PN; i += nt)
      s[i] = (i < N) ? (((uint64_t)random_bits_at(ksub, (uint32_t)N, (uint32_t)i) << 32) | (uint32_t)i) : ~0ull;
    bitonic(s, PN);
    for (int i = tid; i < N; i += nt) s[i] = (uint64_t)(uint32_t)cur[(uint32_t)s[i]];
    __syncthreads();
    for (int i = tid; i < N; i += nt) cur[i] = (int)(uint32_t)s[i];
    __syncthreads();
  }
  for (int i = tid; i < N; i += nt) {
    const bool u = (cur[i] < n_rep) && replayable;
    use_out[i] = u ? 1 : 0;
    chosen[i] = u ? rep[i] : rnd[i];
  }
  (void)rng2;
}

}  // namespace

// keys: [3][2] = replay_rng, random_rng, select_rng (the sampler's rng after split(rng, 3)).
// out: chosen[N], replay[N], random[N], use[N] (int32).
__global__ void __launch_bounds__(kThreads) k_plr_sample(int B, int N, const float* __restrict__ score,
                                                         const uint8_t* __restrict__ active,
                                                         const uint8_t* __restrict__ fresh,
                                                         const uint32_t* __restrict__ keys, int proportional,
                                                         float temperature, float p_replay, int* __restrict__ chosen,
                                                         int* __restrict__ rep, int* __restrict__ rnd,
                                                         int* __restrict__ use_out) {
  __shared__ uint64_t s[kMaxSort];
  __shared__ float f[kMaxSort];
  __shared__ int red[16];
  __shared__ float total;
  const int P = pow2_ceil(B);
  const int tid = threadIdx.x;
  // ---- replay (level_sampler.py:363-385)
  for (int i = tid; i < B; i += blockDim.x) {
    const bool inv = fresh[i] || active[i];
    f[i] = inv ? 0.0f : pexp(__fdiv_rn(score[i], temperature));
  }
  const int n_invalid = count_invalid(B, active, fresh, red);
  normalise(f, B, (B - n_invalid) < N, &total);
  replay_pick(s, f, B, P, N, make_uint2(keys[0], keys[1]), proportional != 0, rep);
  random_new_ids(s, f, red, B, P, N, active, fresh, make_uint2(keys[2], keys[3]), rnd);
  select_ids(s, f, red, B, N, n_invalid, make_uint2(keys[4], keys[5]), p_replay, chosen, rep, rnd, use_out);
}

// k_plr_sample with PLR's replay distribution (Jiang et al. 2021, section 3; not in the reference): the score part is
// the softmax above (transform 0 and 1) or rank^(-1/T) over the stable descending-score ranks of the valid slots
// (transform 2), mixed with the staleness part (now - stamp, normalised) by rho; the valid slots' probabilities are
// floored at the smallest normal float where the rank weights or the mixture can underflow, so that a valid slot's
// Gumbel key stays finite and sorts before every invalid slot's +inf.  The random-new draw and the selection are
// k_plr_sample's.  p_out[B] (may be null) receives the distribution.
__global__ void __launch_bounds__(kThreads) k_plr_sample_prio(
    int B, int N, const float* __restrict__ score, const uint8_t* __restrict__ active,
    const uint8_t* __restrict__ fresh, const int* __restrict__ stamp, int now, const uint32_t* __restrict__ keys,
    int transform, float temperature, float rho, float p_replay, int* __restrict__ chosen, int* __restrict__ rep,
    int* __restrict__ rnd, int* __restrict__ use_out, float* __restrict__ p_out) {
  __shared__ uint64_t s[kMaxSort];
  __shared__ float f[kMaxSort];
  __shared__ int red[16];
  __shared__ float total;
  __shared__ unsigned long long age_sum;
  const int P = pow2_ceil(B);
  const int tid = threadIdx.x;
  const float tiny = 1.17549435e-38f;
  if (tid == 0) age_sum = 0ull;
  const int n_invalid = count_invalid(B, active, fresh, red);
  const int n_valid = B - n_invalid;
  const bool uniform_p = n_valid < N;
  // ---- score part
  if (transform == 2) {
    for (int i = tid; i < B; i += blockDim.x) f[i] = (fresh[i] || active[i]) ? __builtin_inff() : -score[i];
    __syncthreads();
    fill_keys(s, B, P, f);
    bitonic(s, P);
    for (int j = tid; j < B; j += blockDim.x) {      // slot s[j] has rank j + 1
      const int i = (int)(uint32_t)s[j];
      const bool inv = fresh[i] || active[i];
      f[i] = inv ? 0.0f : pexp(__fdiv_rn(-plog((float)(j + 1)), temperature));
    }
  } else {
    for (int i = tid; i < B; i += blockDim.x) {
      const bool inv = fresh[i] || active[i];
      f[i] = inv ? 0.0f : pexp(__fdiv_rn(score[i], temperature));
    }
  }
  normalise(f, B, uniform_p, &total);
  // ---- staleness part, mixture and floor
  if (!uniform_p && (rho > 0.0f || transform == 2)) {
    long long A = 0;
    if (rho > 0.0f) {
      long long part = 0;
      for (int i = tid; i < B; i += blockDim.x) {
        const long long a = (long long)now - (long long)stamp[i];
        if (!(fresh[i] || active[i]) && a > 0) part += a;
      }
      atomicAdd(&age_sum, (unsigned long long)part);     // integer sum: exact in any order
      __syncthreads();
      A = (long long)age_sum;
    }
    for (int i = tid; i < B; i += blockDim.x) {
      const bool inv = fresh[i] || active[i];
      float p = f[i];
      if (rho > 0.0f) {
        const long long d = (long long)now - (long long)stamp[i];
        const long long a = (inv || d < 0) ? 0 : d;
        const float pc = A > 0 ? __fdiv_rn((float)a, (float)A) : (inv ? 0.0f : __fdiv_rn(1.0f, (float)n_valid));
        p = __fadd_rn(__fmul_rn(__fsub_rn(1.0f, rho), p), __fmul_rn(rho, pc));
      }
      f[i] = inv ? 0.0f : (p < tiny ? tiny : p);
    }
    __syncthreads();
  }
  if (p_out != nullptr)
    for (int i = tid; i < B; i += blockDim.x) p_out[i] = f[i];
  replay_pick(s, f, B, P, N, make_uint2(keys[0], keys[1]), transform != 0, rep);
  random_new_ids(s, f, red, B, P, N, active, fresh, make_uint2(keys[2], keys[3]), rnd);
  select_ids(s, f, red, B, N, n_invalid, make_uint2(keys[4], keys[5]), p_replay, chosen, rep, rnd, use_out);
}

// parent_ids[j] = order[j % n_elig] with order = argsort(where(eligible, -score, +inf)), eligible = !fresh and not
// among reset_ids[0..N); -1 when nothing is eligible.  A reset id outside [0, B) excludes nothing.
__global__ void __launch_bounds__(kThreads) k_plr_parent_ids(int B, int N, const float* __restrict__ score,
                                                             const uint8_t* __restrict__ fresh,
                                                             const int* __restrict__ reset_ids,
                                                             int* __restrict__ parent_ids) {
  __shared__ uint64_t s[kMaxSort];
  __shared__ float f[kMaxSort];
  __shared__ uint8_t elig[kMaxSort];
  __shared__ int red[16];
  const int P = pow2_ceil(B);
  const int tid = threadIdx.x;
  for (int i = tid; i < B; i += blockDim.x) elig[i] = fresh[i] ? 0 : 1;
  __syncthreads();
  for (int j = tid; j < N; j += blockDim.x) {
    const int r = reset_ids[j];
    if (r >= 0 && r < B) elig[r] = 0;     // duplicates store the same byte
  }
  __syncthreads();
  int n_elig = 0;
  for (int base = 0; base < B; base += blockDim.x) {
    const int i = base + tid;
    n_elig += block_count(i < B && elig[i], red);
  }
  for (int i = tid; i < B; i += blockDim.x) f[i] = elig[i] ? -score[i] : __builtin_inff();
  __syncthreads();
  fill_keys(s, B, P, f);
  bitonic(s, P);
  for (int j = tid; j < N; j += blockDim.x) parent_ids[j] = n_elig ? (int)(uint32_t)s[j % n_elig] : -1;
}

extern "C" {

int toued_plr_reset_ids(int B, int N, const float* score, const uint8_t* active, const uint8_t* fresh, int* ids,
                        hipStream_t stream) {
  TOUED_REQUIRE(B > 0 && B <= kMaxSort && N >= 0 && N <= B, "toued_plr_reset_ids: need 0 <= N <= B <= %d",
                kMaxSort);
  if (N == 0) return 0;
  hipLaunchKernelGGL(k_plr_reset_ids, dim3(1), dim3(kThreads), 0, stream, B, N, score, active, fresh, ids);
  TOUED_CHECK_LAUNCH();
  return 0;
}

int toued_plr_sample(int B, int N, const float* score, const uint8_t* active, const uint8_t* fresh,
                     const uint32_t* keys, int proportional, float temperature, float p_replay, int* chosen,
                     int* rep, int* rnd, int* use_out, hipStream_t stream) {
  TOUED_REQUIRE(B > 0 && B <= kMaxSort && N >= 0 && N <= B, "toued_plr_sample: need 0 <= N <= B <= %d", kMaxSort);
  TOUED_REQUIRE(temperature > 0.0f, "toued_plr_sample: temperature must be > 0");
  if (N == 0) return 0;
  hipLaunchKernelGGL(k_plr_sample, dim3(1), dim3(kThreads), 0, stream, B, N, score, active, fresh, keys,
                     proportional, temperature, p_replay, chosen, rep, rnd, use_out);
  TOUED_CHECK_LAUNCH();
  return 0;
}

int toued_plr_sample_prio(int B, int N, const float* score, const uint8_t* active, const uint8_t* fresh,
                          const int* stamp, int now, const uint32_t* keys, int transform, float temperature,
                          float staleness_coeff, float p_replay, int* chosen, int* rep, int* rnd, int* use_out,
                          float* p_out, hipStream_t stream) {
  TOUED_REQUIRE(B > 0 && B <= kMaxSort && N >= 0 && N <= B, "toued_plr_sample_prio: need 0 <= N <= B <= %d",
                kMaxSort);
  TOUED_REQUIRE(temperature > 0.0f, "toued_plr_sample_prio: temperature must be > 0");
  TOUED_REQUIRE(transform >= 0 && transform <= 2,
                "toued_plr_sample_prio: transform must be 0 (rank), 1 (proportional) or 2 (rank_sampled), got %d",
                transform);
  TOUED_REQUIRE(staleness_coeff >= 0.0f && staleness_coeff <= 1.0f,
                "toued_plr_sample_prio: staleness_coeff must be in [0, 1]");
  TOUED_REQUIRE(stamp != nullptr || staleness_coeff == 0.0f,
                "toued_plr_sample_prio: staleness_coeff > 0 needs the slots' stamps");
  if (N == 0) return 0;
  hipLaunchKernelGGL(k_plr_sample_prio, dim3(1), dim3(kThreads), 0, stream, B, N, score, active, fresh, stamp, now,
                     keys, transform, temperature, staleness_coeff, p_replay, chosen, rep, rnd, use_out, p_out);
  TOUED_CHECK_LAUNCH();
  return 0;
}

int toued_plr_parent_ids(int B, int N, const float* score, const uint8_t* fresh, const int* reset_ids,
                         int* parent_ids, hipStream_t stream) {
  TOUED_REQUIRE(B > 0 && B <= kMaxSort && N >= 0 && N <= B, "toued_plr_parent_ids: need 0 <= N <= B <= %d",
                kMaxSort);
  if (N == 0) return 0;
  hipLaunchKernelGGL(k_plr_parent_ids, dim3(1), dim3(kThreads), 0, stream, B, N, score, fresh, reset_ids,
                     parent_ids);
  TOUED_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
