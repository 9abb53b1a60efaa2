// What the PursuitTag episode kernels share (rollout_tag.hip: a workgroup
// per game, and its antithetic-pair form; rollout_tag_wave.hip: a wavefront
// per game): the game itself (BatchedPursuitTag, envs/multiagent.py: the
// observation layout, the move, the catch rule and the rewards), a policy's
// launch arguments, the C argument list of the per-game entry points and the
// checks every launch path makes.
#pragma once
#include "mlp_core.h"

#define TAG_OB 8        // own p, own v, other p, other v
#define TAG_AC 2
#define TAG_ARENA 5.0f  // BatchedPursuitTag.ARENA
#define TAG_CATCH_DIST 0.3f    // the chaser is within this of the runner: the game ends
#define TAG_CATCH_BONUS 10.0f  // to the chaser, from the runner, on that step

// Where observation k of `agent` sits in the game state st = p[2][2] v[2][2].
__device__ __forceinline__ int tag_ob_index(int agent, int k) {
  const int who = (k & 4) ? 1 - agent : agent;
  return ((k >> 1) & 1) * 4 + who * 2 + (k & 1);
}

// BatchedPursuitTag.step for one coordinate of one agent, op for op in fp32:
// raw action -> velocity -> position.
__device__ __forceinline__ void tag_move(float& p, float& v, float raw) {
#pragma clang fp contract(off)
  const float a = fclampf(raw, -1.0f, 1.0f);
  const float vn = 0.8f * v + a * 0.1f * 5.0f;
  v = vn;
  p = fclampf(p + vn * 0.1f, -TAG_ARENA, TAG_ARENA);
}

// The step's rewards at distance d after the move, added to the chaser's
// (agent 0) and the runner's (agent 1) totals.
__device__ __forceinline__ void tag_reward(float d, bool caught, float& rew0, float& rew1) {
#pragma clang fp contract(off)
  const float bonus = caught ? TAG_CATCH_BONUS : 0.0f;
  rew0 += -d + bonus;
  rew1 += d - bonus;
}

struct TagPolicy {
  const void* weights;  // member rows of the kernel's weight type, row_stride apart
  const float* obmean;
  const float* obstd;
  const float* ac_std_dev;
  int64_t row_stride;
  float ob_clip;
  MlpShape sh;
};

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

// One call's arguments, in the order of TAG_EPISODE_ENTRY's list.
struct TagCall {
  void *p, *v, *alive, *steps, *rew_total, *ob_sum, *ob_sumsq;
  const void *weights0, *weights1, *obmean0, *obmean1, *obstd0, *obstd1;
  const int32_t* dims0_host;
  int32_t ndims0;
  const int32_t* dims1_host;
  int32_t ndims1;
  int64_t row_stride0, row_stride1;
  float ob_clip0, ob_clip1;
  const void *ac_std_dev0, *ac_std_dev1, *seed_dev;
  uint64_t salt_base;
  int32_t n_agents, ob_dim, n_games, n_steps, act_final, noiseless_from;
  void* stream;
};

// The checks every launch path makes before any of its own, in this order:
// -112, -110, then policy 0's codes, then policy 1's (tag_policy_init). Fills
// both policies. 0: go on; a negative code: launch nothing.
static inline int tag_policies_init(const TagCall& c, bool f32, TagPolicy* P0, TagPolicy* P1) {
  if (c.n_agents != 2) return -112;
  if (c.ob_dim != TAG_OB) return -110;
  int rc = tag_policy_init(P0, f32, c.weights0, c.obmean0, c.obstd0, c.ac_std_dev0,
                           c.dims0_host, c.ndims0, c.row_stride0, c.ob_clip0);
  if (rc) return rc;
  return tag_policy_init(P1, f32, c.weights1, c.obmean1, c.obstd1, c.ac_std_dev1,
                         c.dims1_host, c.ndims1, c.row_stride1, c.ob_clip1);
}

// Defines the extern "C" entry point `name`, which calls
// launcher(f32, const TagCall&). The argument list of every per-game entry
// point (es_tag_episode[_f32], es_tag_wave_episode[_f32]):
//
// State, (n_games, ...) each, read at launch and written back at the end:
// p, v float (.,2,2); alive, steps float (.); rew_total float (.,2);
// ob_sum, ob_sumsq double (.,2,8). Policy i: weights_i (n_games,
// row_stride_i), bf16 or, for an _f32 entry point, float32 with row_stride_i
// counted in floats; obmean/obstd float (8), ac_std_dev_i float (1) or null.
// Step t of the launch (0-based) draws agent i's action noise with key
// *seed_dev + (salt_base + t + 1) * 2 + i. n_agents and ob_dim are what the
// caller's env has; only 2 and 8 are implemented.
#define TAG_EPISODE_ENTRY(name, launcher, f32)                                              \
  extern "C" int name(                                                                      \
      void* p, void* v, void* alive, void* steps, void* rew_total, void* ob_sum,            \
      void* ob_sumsq, const void* weights0, const void* weights1, const void* obmean0,      \
      const void* obmean1, const void* obstd0, const void* obstd1,                          \
      const int32_t* dims0_host, int32_t ndims0, const int32_t* dims1_host, int32_t ndims1, \
      int64_t row_stride0, int64_t row_stride1, float ob_clip0, float ob_clip1,             \
      const void* ac_std_dev0, const void* ac_std_dev1, const void* seed_dev,               \
      uint64_t salt_base, int32_t n_agents, int32_t ob_dim, int32_t n_games,                \
      int32_t n_steps, int32_t act_final, int32_t noiseless_from, void* stream) {           \
    return launcher(                                                                        \
        f32, TagCall{p, v, alive, steps, rew_total, ob_sum, ob_sumsq, weights0, weights1,   \
                     obmean0, obmean1, obstd0, obstd1, dims0_host, ndims0, dims1_host,      \
                     ndims1, row_stride0, row_stride1, ob_clip0, ob_clip1, ac_std_dev0,     \
                     ac_std_dev1, seed_dev, salt_base, n_agents, ob_dim, n_games, n_steps,  \
                     act_final, noiseless_from, stream});                                   \
  }
