// Whole-episode rollout of the two-agent pursuit-evasion tag game
// (envs/multiagent.py, BatchedPursuitTag) for the co-evolution engine.
//
// One 256-thread workgroup per game b plays up to n_steps env steps in one
// launch: per step it runs agent 0's and agent 1's MLP (each on member row b
// of that policy's own blob: mlp_layers on bf16 rows, mlp_layers_f32 on fp32
// rows, one kernel body templated on the weight element type), steps the game
// and does the engine's bookkeeping (reward and step totals, fp64 observation
// moments).
// The game state lives in LDS between steps; it is read from global memory at
// launch and written back at the end, so a rollout may be cut into several
// launches with salt_base continuing. A game that ends leaves the step loop:
// the condition is block-uniform, so no barrier is ever divergent.
//
// Only what PursuitTag needs: two agents, 8 observations each, the first two
// outputs of each net are the action. Anything else is an argument error.
#include "mlp_core.h"

#define TAG_OB 8        // own p, own v, other p, other v
#define TAG_AC 2
#define TAG_ARENA 5.0f  // BatchedPursuitTag.ARENA
// game slab behind the mlp carve: fp64 ob_sum[2][8], ob_sumsq[2][8], then
// float p[2][2], v[2][2], act[2][2], rew[2], steps, pad[3]
#define TAG_SLAB_BYTES (2 * 2 * TAG_OB * 8 + 16 * 4)
// the pair kernel's dynamic LDS: four activation buffers and two 256x8
// partial slabs (= 2 * mlp_lds_bytes), then one game slab per member
#define TAG_PAIR_LDS_BYTES(maxdim) (2 * mlp_lds_bytes(maxdim) + 2 * TAG_SLAB_BYTES)

struct TagPolicy {
  const void* weights;  // member rows of the kernel's weight type, row_stride apart
  const float* obmean;
  const float* obstd;
  const float* ac_std_dev;
  int64_t row_stride;
  float ob_clip;
  MlpShape sh;
};

// Agent i's forward on the pre-step state: writes its two raw actions to
// act[2i], act[2i+1]. Ends on a barrier, so bufA/bufB are free afterwards.
template <typename WT>
__device__ __forceinline__ void tag_agent_forward(
    const TagPolicy& P, int i, int b, const float* st, float* act, float* bufA,
    float* bufB, float* partial, float mean_k, float std_k, uint64_t seed,
    int act_final, int noiseless_from, int tid) {
  if (tid < TAG_OB) {
    // st = p[2][2] v[2][2]: own p, own v, other p, other v
    const int who = (tid & 4) ? 1 - i : i;
    const float ob = st[((tid >> 1) & 1) * 4 + who * 2 + (tid & 1)];
    bufA[tid] = fclampf((ob - mean_k) / std_k, -P.ob_clip, P.ob_clip);
  }
  __syncthreads();
  const WT* wb = reinterpret_cast<const WT*>(P.weights) + (int64_t)b * P.row_stride;
  const float* out;
  if constexpr (sizeof(WT) == 4)
    out = mlp_layers_f32(wb, P.sh, bufA, bufB, partial, tid, 256, act_final);
  else
    out = mlp_layers(wb, P.sh, bufA, bufB, partial, tid, 256, act_final);
  if (tid < TAG_AC) {
    const int A = P.sh.dims[P.sh.n_layers];
    const float ac_std = P.ac_std_dev ? *P.ac_std_dev : 0.0f;
    float a = out[tid];
    if (ac_std != 0.0f && b < noiseless_from)
      a += ac_std * es_actnoise(seed, (uint64_t)b * A + tid);
    act[i * 2 + tid] = a;
  }
  __syncthreads();
}

template <typename WT>
__global__ void __launch_bounds__(256)
tag_episode_kernel(float* __restrict__ p_g, float* __restrict__ v_g,
                   float* __restrict__ alive_g, float* __restrict__ steps_g,
                   float* __restrict__ rew_g, double* __restrict__ obsum_g,
                   double* __restrict__ obsq_g, TagPolicy P0, TagPolicy P1, int lds_maxdim,
                   const uint64_t* __restrict__ seed_dev, uint64_t salt_base, int n_steps,
                   int act_final, int noiseless_from) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* bufA = reinterpret_cast<float*>(smem);
  float* bufB = bufA + lds_maxdim;
  float* partial = bufB + lds_maxdim;
  double* obsum = reinterpret_cast<double*>(partial + 256 * 8);
  double* obsq = obsum + 2 * TAG_OB;
  float* st = reinterpret_cast<float*>(obsq + 2 * TAG_OB);  // p[2][2] v[2][2]
  float* act = st + 8;
  float* rew = act + 4;
  float* steps = rew + 2;
  const int b = blockIdx.x;
  const int tid = threadIdx.x;

  if (tid < 4) {
    st[tid] = p_g[(int64_t)b * 4 + tid];
    st[4 + tid] = v_g[(int64_t)b * 4 + tid];
  }
  if (tid < 2 * TAG_OB) {
    obsum[tid] = obsum_g[(int64_t)b * 2 * TAG_OB + tid];
    obsq[tid] = obsq_g[(int64_t)b * 2 * TAG_OB + tid];
  }
  if (tid < 2) rew[tid] = rew_g[(int64_t)b * 2 + tid];
  if (tid == 0) steps[0] = steps_g[b];
  bool alive = alive_g[b] != 0.0f;
  // launch invariants of the threads that build the observations
  float mean0 = 0.0f, std0 = 1.0f, mean1 = 0.0f, std1 = 1.0f;
  if (tid < TAG_OB) {
    mean0 = P0.obmean[tid];
    std0 = P0.obstd[tid];
    mean1 = P1.obmean[tid];
    std1 = P1.obstd[tid];
  }
  const uint64_t seed0 = seed_dev ? *seed_dev : 0;
  __syncthreads();

  for (int t = 0; t < n_steps && alive; ++t) {
    // the key of es_mlp_fwd at salt (t+1)*2 + i: the per-step engine's draw
    const uint64_t seed = seed0 + (salt_base + (uint64_t)t + 1) * 2;
    tag_agent_forward<WT>(P0, 0, b, st, act, bufA, bufB, partial, mean0, std0, seed,
                          act_final, noiseless_from, tid);
    tag_agent_forward<WT>(P1, 1, b, st, act, bufA, bufB, partial, mean1, std1, seed + 1,
                          act_final, noiseless_from, tid);
    {
      // BatchedPursuitTag.step, op for op in fp32
#pragma clang fp contract(off)
      if (tid < 4) {
        const float a = fclampf(act[tid], -1.0f, 1.0f);
        const float vn = 0.8f * st[4 + tid] + a * 0.1f * 5.0f;
        st[4 + tid] = vn;
        st[tid] = fclampf(st[tid] + vn * 0.1f, -TAG_ARENA, TAG_ARENA);
      }
      __syncthreads();
      const float dx = st[0] - st[2], dy = st[1] - st[3];
      const float d = sqrtf(dx * dx + dy * dy);
      const bool caught = d < 0.3f;
      const float bonus = caught ? 10.0f : 0.0f;
      if (tid == 0) {
        rew[0] += -d + bonus;
        rew[1] += d - bonus;
        steps[0] += 1.0f;
      }
      if (tid < 2 * TAG_OB) {
        // post-step observation of agent tid / 8, the terminal one included
        const int i = tid >> 3, k = tid & 7;
        const int who = (k & 4) ? 1 - i : i;
        const double ob = (double)st[((k >> 1) & 1) * 4 + who * 2 + (k & 1)];
        obsum[tid] += ob;
        obsq[tid] += ob * ob;
      }
      alive = !caught;
    }
    // the next step's first LDS write (bufA) is to another region, and every
    // write to st/act/rew sits behind one of its barriers
  }

  __syncthreads();
  if (tid < 4) {
    p_g[(int64_t)b * 4 + tid] = st[tid];
    v_g[(int64_t)b * 4 + tid] = st[4 + tid];
  }
  if (tid < 2 * TAG_OB) {
    obsum_g[(int64_t)b * 2 * TAG_OB + tid] = obsum[tid];
    obsq_g[(int64_t)b * 2 * TAG_OB + tid] = obsq[tid];
  }
  if (tid < 2) rew_g[(int64_t)b * 2 + tid] = rew[tid];
  if (tid == 0) {
    steps_g[b] = steps[0];
    alive_g[b] = alive ? 1.0f : 0.0f;
  }
}

// f32: the rows are float32 and a layer is quad-tiled only where its 16-B
// loads are aligned for THIS policy's stride (mlp_shape_vec_f32).
static inline int tag_policy_init(TagPolicy* P, bool f32, const void* weights,
                                  const void* obmean, const void* obstd,
                                  const void* ac_std_dev, const int32_t* dims_host,
                                  int32_t ndims, int64_t row_stride, float ob_clip) {
  int rc = mlp_shape_init(&P->sh, dims_host, ndims, row_stride);
  if (rc) return rc;
  if (f32) mlp_shape_vec_f32(&P->sh, row_stride);
  if (P->sh.dims[0] != TAG_OB) return -110;
  if (P->sh.dims[P->sh.n_layers] < TAG_AC) return -111;
  P->weights = weights;
  P->obmean = (const float*)obmean;
  P->obstd = (const float*)obstd;
  P->ac_std_dev = (const float*)ac_std_dev;
  P->row_stride = row_stride;
  P->ob_clip = ob_clip;
  return 0;
}

static inline int tag_launch(bool f32, void* p, void* v, void* alive, void* steps,
                             void* rew_total, void* ob_sum, void* ob_sumsq,
                             const void* weights0, const void* weights1,
                             const void* obmean0, const void* obmean1, const void* obstd0,
                             const void* obstd1, const int32_t* dims0_host, int32_t ndims0,
                             const int32_t* dims1_host, int32_t ndims1, int64_t row_stride0,
                             int64_t row_stride1, float ob_clip0, float ob_clip1,
                             const void* ac_std_dev0, const void* ac_std_dev1,
                             const void* seed_dev, uint64_t salt_base, int32_t n_agents,
                             int32_t ob_dim, int32_t n_games, int32_t n_steps,
                             int32_t act_final, int32_t noiseless_from, void* stream) {
  if (n_agents != 2) return -112;
  if (ob_dim != TAG_OB) return -110;
  TagPolicy P0, P1;
  int rc = tag_policy_init(&P0, f32, weights0, obmean0, obstd0, ac_std_dev0, dims0_host,
                           ndims0, row_stride0, ob_clip0);
  if (rc) return rc;
  rc = tag_policy_init(&P1, f32, weights1, obmean1, obstd1, ac_std_dev1, dims1_host, ndims1,
                       row_stride1, ob_clip1);
  if (rc) return rc;
  if (n_games <= 0 || n_steps <= 0) return 0;
  const int maxdim = std::max(P0.sh.maxdim, P1.sh.maxdim);
  const unsigned lds = (unsigned)(mlp_lds_bytes(maxdim) + TAG_SLAB_BYTES);
  auto kernel = f32 ? tag_episode_kernel<float> : tag_episode_kernel<uint16_t>;
  kernel<<<dim3((unsigned)n_games), dim3(256), lds, (hipStream_t)stream>>>(
      (float*)p, (float*)v, (float*)alive, (float*)steps, (float*)rew_total,
      (double*)ob_sum, (double*)ob_sumsq, P0, P1, maxdim, (const uint64_t*)seed_dev,
      salt_base, n_steps, act_final, noiseless_from);
  ES_CHECK_LAUNCH();
  return 0;
}

// State, (n_games, ...) each, read at launch and written back at the end:
// p, v float (.,2,2); alive, steps float (.); rew_total float (.,2);
// ob_sum, ob_sumsq double (.,2,8). Policy i: bf16 weights (n_games,
// row_stride_i), obmean/obstd float (8), ac_std_dev_i float (1) or null.
// Step t of the launch (0-based) draws agent i's action noise with key
// *seed_dev + (salt_base + t + 1) * 2 + i. n_agents and ob_dim are what the
// caller's env has; only 2 and 8 are implemented.
extern "C" int es_tag_episode(void* p, void* v, void* alive, void* steps, void* rew_total,
                              void* ob_sum, void* ob_sumsq, const void* weights0,
                              const void* weights1, const void* obmean0,
                              const void* obmean1, const void* obstd0, const void* obstd1,
                              const int32_t* dims0_host, int32_t ndims0,
                              const int32_t* dims1_host, int32_t ndims1,
                              int64_t row_stride0, int64_t row_stride1, float ob_clip0,
                              float ob_clip1, const void* ac_std_dev0,
                              const void* ac_std_dev1, const void* seed_dev,
                              uint64_t salt_base, int32_t n_agents, int32_t ob_dim,
                              int32_t n_games, int32_t n_steps, int32_t act_final,
                              int32_t noiseless_from, void* stream) {
  return tag_launch(false, p, v, alive, steps, rew_total, ob_sum, ob_sumsq, weights0,
                    weights1, obmean0, obmean1, obstd0, obstd1, dims0_host, ndims0,
                    dims1_host, ndims1, row_stride0, row_stride1, ob_clip0, ob_clip1,
                    ac_std_dev0, ac_std_dev1, seed_dev, salt_base, n_agents, ob_dim, n_games,
                    n_steps, act_final, noiseless_from, stream);
}

// fp32 rows: same argument list and return codes; weights_i is float32
// (n_games, row_stride_i), row_stride_i counted in floats. A policy whose
// stride is no multiple of 4 floats, and any layer whose weight block is not
// 16-B aligned in the row or whose width is no multiple of 4, takes the
// scalar walks.
extern "C" int es_tag_episode_f32(void* p, void* v, void* alive, void* steps,
                                  void* rew_total, void* ob_sum, void* ob_sumsq,
                                  const void* weights0, const void* weights1,
                                  const void* obmean0, const void* obmean1,
                                  const void* obstd0, const void* obstd1,
                                  const int32_t* dims0_host, int32_t ndims0,
                                  const int32_t* dims1_host, int32_t ndims1,
                                  int64_t row_stride0, int64_t row_stride1, float ob_clip0,
                                  float ob_clip1, const void* ac_std_dev0,
                                  const void* ac_std_dev1, const void* seed_dev,
                                  uint64_t salt_base, int32_t n_agents, int32_t ob_dim,
                                  int32_t n_games, int32_t n_steps, int32_t act_final,
                                  int32_t noiseless_from, void* stream) {
  return tag_launch(true, p, v, alive, steps, rew_total, ob_sum, ob_sumsq, weights0,
                    weights1, obmean0, obmean1, obstd0, obstd1, dims0_host, ndims0,
                    dims1_host, ndims1, row_stride0, row_stride1, ob_clip0, ob_clip1,
                    ac_std_dev0, ac_std_dev1, seed_dev, salt_base, n_agents, ob_dim, n_games,
                    n_steps, act_final, noiseless_from, stream);
}

// ---- antithetic-pair form ---------------------------------------------------
// One workgroup plays BOTH games of an antithetic pair: block g < n_pairs has
// game g on bf16(theta_i) + bf16(eps_i[g]) (its "+" member) and game
// g + n_pairs on bf16(theta_i) - bf16(eps_i[g]) (its "-" member), one
// mlp_layers_pair per agent and step driving both. With n_single == 1, block
// n_pairs plays game 2 * n_pairs alone as a "+" member on eps row n_pairs,
// which the caller keeps zero: that block has no "-" member, reads and writes
// no state for one, and its "-" buffers are zero-filled.
//
// Threads 0..31 serve the "+" game and 32..63 the "-" game: lane lt of a
// member does what thread lt of tag_episode_kernel does (lt < 4 steps p/v,
// lt == 0 keeps the totals, lt < 16 the moments). The loop runs while either
// game is alive; a game that was caught is frozen while its partner plays on.
// LDS: TAG_PAIR_LDS_BYTES, the slab of tag_episode_kernel once per member.
struct TagPairLds {
  float *bufAp, *bufAm, *bufBp, *bufBm, *partial;
};

// Agent i's dual forward on the pre-step states of both games: member lane
// lt < 2 writes its game's raw action to act[2i + lt]. Ends on a barrier.
__device__ __forceinline__ void tag_pair_agent_forward(
    const TagPolicy& P, const uint16_t* __restrict__ eps_rows, int i, int g, int game,
    bool mine, int m, int lt, const float* st, float* act, const TagPairLds& L, float mean_k,
    float std_k, uint64_t seed, int act_final, int noiseless_from, int tid) {
  if (lt < TAG_OB) {
    const int who = (lt & 4) ? 1 - i : i;
    const float ob = st[((lt >> 1) & 1) * 4 + who * 2 + (lt & 1)];
    (m ? L.bufAm : L.bufAp)[lt] =
        mine ? fclampf((ob - mean_k) / std_k, -P.ob_clip, P.ob_clip) : 0.0f;
  }
  __syncthreads();
  const uint16_t* tb = reinterpret_cast<const uint16_t*>(P.weights);
  const uint16_t* eb = eps_rows + (int64_t)g * P.row_stride;
  float *outp, *outm;
  mlp_layers_pair(tb, eb, P.sh, L.bufAp, L.bufAm, L.bufBp, L.bufBm, L.partial, tid, 256,
                  act_final, &outp, &outm);
  if (lt < TAG_AC) {
    const int A = P.sh.dims[P.sh.n_layers];
    const float ac_std = P.ac_std_dev ? *P.ac_std_dev : 0.0f;
    float a = (m ? outm : outp)[lt];
    if (ac_std != 0.0f && game < noiseless_from)
      a += ac_std * es_actnoise(seed, (uint64_t)game * A + lt);
    act[i * 2 + lt] = a;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(256)
tag_pair_episode_kernel(float* __restrict__ p_g, float* __restrict__ v_g,
                        float* __restrict__ alive_g, float* __restrict__ steps_g,
                        float* __restrict__ rew_g, double* __restrict__ obsum_g,
                        double* __restrict__ obsq_g, TagPolicy P0, TagPolicy P1,
                        const uint16_t* __restrict__ eps0, const uint16_t* __restrict__ eps1,
                        int lds_maxdim, const uint64_t* __restrict__ seed_dev,
                        uint64_t salt_base, int n_pairs, int n_steps, int act_final,
                        int noiseless_from) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  TagPairLds L;
  L.bufAp = reinterpret_cast<float*>(smem);
  L.bufAm = L.bufAp + lds_maxdim;
  L.bufBp = L.bufAm + lds_maxdim;
  L.bufBm = L.bufBp + lds_maxdim;
  L.partial = L.bufBm + lds_maxdim;  // 2 x 256*8
  char* slabs = reinterpret_cast<char*>(L.partial + 2 * 256 * 8);
  const int g = blockIdx.x;
  const int tid = threadIdx.x;
  const bool has_m = g < n_pairs;
  const int gp = has_m ? g : 2 * n_pairs;  // the "+" game; the "-" one is g + n_pairs
  // the member this thread serves, its lane there (32: none) and its game
  const int m = (tid >> 5) & 1;
  const int lt = tid < 64 ? (tid & 31) : 32;
  const int game = m ? g + n_pairs : gp;
  const bool mine = lt < 32 && (m == 0 || has_m);

  char* slab = slabs + m * TAG_SLAB_BYTES;
  double* obsum = reinterpret_cast<double*>(slab);
  double* obsq = obsum + 2 * TAG_OB;
  float* st = reinterpret_cast<float*>(obsq + 2 * TAG_OB);  // p[2][2] v[2][2]
  float* act = st + 8;
  float* rew = act + 4;
  float* steps = rew + 2;
  const float* stP = reinterpret_cast<const float*>(slabs + 4 * TAG_OB * 8);
  const float* stM = reinterpret_cast<const float*>(slabs + TAG_SLAB_BYTES + 4 * TAG_OB * 8);

  if (mine) {
    if (lt < 4) {
      st[lt] = p_g[(int64_t)game * 4 + lt];
      st[4 + lt] = v_g[(int64_t)game * 4 + lt];
    }
    if (lt < 2 * TAG_OB) {
      obsum[lt] = obsum_g[(int64_t)game * 2 * TAG_OB + lt];
      obsq[lt] = obsq_g[(int64_t)game * 2 * TAG_OB + lt];
    }
    if (lt < 2) rew[lt] = rew_g[(int64_t)game * 2 + lt];
    if (lt == 0) steps[0] = steps_g[game];
  } else if (lt < 32) {
    // no "-" member: its slab holds zeros
    for (int k = lt; k < TAG_SLAB_BYTES / 4; k += 32) reinterpret_cast<float*>(slab)[k] = 0.0f;
  }
  if (!has_m)  // and so do its activation buffers
    for (int k = tid; k < lds_maxdim; k += 256) L.bufAm[k] = L.bufBm[k] = 0.0f;
  bool aliveP = alive_g[gp] != 0.0f;
  bool aliveM = has_m && alive_g[has_m ? g + n_pairs : gp] != 0.0f;
  // launch invariants of the lanes that build the observations
  float mean0 = 0.0f, std0 = 1.0f, mean1 = 0.0f, std1 = 1.0f;
  if (lt < TAG_OB) {
    mean0 = P0.obmean[lt];
    std0 = P0.obstd[lt];
    mean1 = P1.obmean[lt];
    std1 = P1.obstd[lt];
  }
  const uint64_t seed0 = seed_dev ? *seed_dev : 0;
  __syncthreads();

  for (int t = 0; t < n_steps && (aliveP || aliveM); ++t) {
    const uint64_t seed = seed0 + (salt_base + (uint64_t)t + 1) * 2;
    tag_pair_agent_forward(P0, eps0, 0, g, game, mine, m, lt, st, act, L, mean0, std0, seed,
                           act_final, noiseless_from, tid);
    tag_pair_agent_forward(P1, eps1, 1, g, game, mine, m, lt, st, act, L, mean1, std1,
                           seed + 1, act_final, noiseless_from, tid);
    {
      // BatchedPursuitTag.step for both games, op for op in fp32; a game
      // that is not alive keeps its state
#pragma clang fp contract(off)
      const bool my_alive = lt < 32 && (m ? aliveM : aliveP);
      if (lt < 4 && my_alive) {
        const float a = fclampf(act[lt], -1.0f, 1.0f);
        const float vn = 0.8f * st[4 + lt] + a * 0.1f * 5.0f;
        st[4 + lt] = vn;
        st[lt] = fclampf(st[lt] + vn * 0.1f, -TAG_ARENA, TAG_ARENA);
      }
      __syncthreads();
      const float dxP = stP[0] - stP[2], dyP = stP[1] - stP[3];
      const float dP = sqrtf(dxP * dxP + dyP * dyP);
      const float dxM = stM[0] - stM[2], dyM = stM[1] - stM[3];
      const float dM = sqrtf(dxM * dxM + dyM * dyM);
      const bool caughtP = dP < 0.3f, caughtM = dM < 0.3f;
      if (my_alive) {
        const float d = m ? dM : dP;
        const float bonus = (m ? caughtM : caughtP) ? 10.0f : 0.0f;
        if (lt == 0) {
          rew[0] += -d + bonus;
          rew[1] += d - bonus;
          steps[0] += 1.0f;
        }
        if (lt < 2 * TAG_OB) {
          // post-step observation of agent lt / 8, the terminal one included
          const int i = lt >> 3, k = lt & 7;
          const int who = (k & 4) ? 1 - i : i;
          const double ob = (double)st[((k >> 1) & 1) * 4 + who * 2 + (k & 1)];
          obsum[lt] += ob;
          obsq[lt] += ob * ob;
        }
      }
      aliveP = aliveP && !caughtP;
      aliveM = aliveM && !caughtM;
    }
    // as in tag_episode_kernel: the next step's first LDS writes go to
    // bufAp/bufAm, and every write to a slab sits behind one of its barriers
  }

  __syncthreads();
  if (mine) {
    if (lt < 4) {
      p_g[(int64_t)game * 4 + lt] = st[lt];
      v_g[(int64_t)game * 4 + lt] = st[4 + lt];
    }
    if (lt < 2 * TAG_OB) {
      obsum_g[(int64_t)game * 2 * TAG_OB + lt] = obsum[lt];
      obsq_g[(int64_t)game * 2 * TAG_OB + lt] = obsq[lt];
    }
    if (lt < 2) rew_g[(int64_t)game * 2 + lt] = rew[lt];
    if (lt == 0) {
      steps_g[game] = steps[0];
      alive_g[game] = (m ? aliveM : aliveP) ? 1.0f : 0.0f;
    }
  }
}

// The pair form of es_tag_episode. State as there, (n_games, ...) with
// n_games = 2 * n_pairs + n_single in the slot order [+pairs | -pairs |
// single]. Policy i: theta_i ONE bf16 row, eps_i bf16 sigma*eps rows
// (n_pairs + n_single, row_stride_i), row n_pairs zero when n_single == 1;
// row_stride_i a multiple of 8, so that every row is 16-B aligned. Action
// noise is keyed by the GAME index exactly as es_tag_episode keys it, so both
// forms draw the same noise. Return codes: those of es_tag_episode, and -113
// when n_single is neither 0 nor 1 or n_pairs is negative.
extern "C" int es_tag_pair_episode(void* p, void* v, void* alive, void* steps,
                                   void* rew_total, void* ob_sum, void* ob_sumsq,
                                   const void* theta0, const void* theta1,
                                   const void* eps0, const void* eps1,
                                   const void* obmean0, const void* obmean1,
                                   const void* obstd0, const void* obstd1,
                                   const int32_t* dims0_host, int32_t ndims0,
                                   const int32_t* dims1_host, int32_t ndims1,
                                   int64_t row_stride0, int64_t row_stride1, float ob_clip0,
                                   float ob_clip1, const void* ac_std_dev0,
                                   const void* ac_std_dev1, const void* seed_dev,
                                   uint64_t salt_base, int32_t n_agents, int32_t ob_dim,
                                   int32_t n_pairs, int32_t n_single, int32_t n_steps,
                                   int32_t act_final, int32_t noiseless_from, void* stream) {
  if (n_agents != 2) return -112;
  if (ob_dim != TAG_OB) return -110;
  TagPolicy P0, P1;
  int rc = tag_policy_init(&P0, false, theta0, obmean0, obstd0, ac_std_dev0, dims0_host,
                           ndims0, row_stride0, ob_clip0);
  if (rc) return rc;
  rc = tag_policy_init(&P1, false, theta1, obmean1, obstd1, ac_std_dev1, dims1_host, ndims1,
                       row_stride1, ob_clip1);
  if (rc) return rc;
  if (n_pairs < 0 || n_single < 0 || n_single > 1) return -113;
  if (n_pairs + n_single == 0 || n_steps <= 0) return 0;
  const int maxdim = std::max(P0.sh.maxdim, P1.sh.maxdim);
  const unsigned lds = (unsigned)TAG_PAIR_LDS_BYTES(maxdim);
  tag_pair_episode_kernel<<<dim3((unsigned)(n_pairs + n_single)), dim3(256), lds,
                            (hipStream_t)stream>>>(
      (float*)p, (float*)v, (float*)alive, (float*)steps, (float*)rew_total,
      (double*)ob_sum, (double*)ob_sumsq, P0, P1, (const uint16_t*)eps0,
      (const uint16_t*)eps1, maxdim, (const uint64_t*)seed_dev, salt_base, n_pairs, n_steps,
      act_final, noiseless_from);
  ES_CHECK_LAUNCH();
  return 0;
}
