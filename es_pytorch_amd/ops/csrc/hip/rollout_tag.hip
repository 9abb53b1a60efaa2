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
