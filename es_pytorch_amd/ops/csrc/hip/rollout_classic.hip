// Whole-episode rollout of the two classic-control envs (envs/classic.py,
// BatchedCartPole and BatchedPendulum) for the single-policy engine.
//
// One 256-thread workgroup per evaluation slot b plays up to n_steps env steps
// in one launch: per step it builds the observation, runs the slot's MLP
// (mlp_layers on bf16 rows, mlp_layers_f32 on fp32 rows; slot b reads weight
// row b / eps), steps the env in fp32 in the env's op order and does the
// engine's bookkeeping (reward and step totals, per-slot fp64 observation
// moments). The slot state lives in LDS between steps; it is read from global
// memory at launch and written back at the end, so a rollout may be cut into
// several launches with salt_base continuing. A slot whose episode ends
// leaves the step loop: every thread reads the same LDS values behind a
// barrier, so the condition is block-uniform and no barrier is divergent.
//
// Only the plain action head (act_mode 0, no bins), and only output 0 of the
// net is the action: both envs have one action dimension.
#include "classic_env.h"

// slot slab behind the mlp carve: fp64 ob_sum[4], ob_sumsq[4], then float
// st[4] (the env state), ob[4] (its observation), rew, member steps, env
// steps, pad
#define CLS_SLAB_BYTES (2 * CLS_MAXOB * 8 + 12 * 4)

template <typename WT>
__device__ __forceinline__ void classic_episode_body(const ClassicArgs& A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* bufA = reinterpret_cast<float*>(smem);
  float* bufB = bufA + A.sh.maxdim;
  float* partial = bufB + A.sh.maxdim;
  double* obsum = reinterpret_cast<double*>(partial + 256 * 8);
  double* obsq = obsum + CLS_MAXOB;
  float* st = reinterpret_cast<float*>(obsq + CLS_MAXOB);
  float* ob = st + 4;
  float* tot = ob + 4;  // rew, member steps, env steps
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int kind = A.kind;
  const int D = A.sh.dims[0];
  const int S = kind == CLS_CARTPOLE ? 4 : 2;
  const WT* wb = reinterpret_cast<const WT*>(A.weights) + (int64_t)(b / A.eps) * A.row_stride;

  if (tid < S) {
    if (kind == CLS_CARTPOLE) st[tid] = A.state[(int64_t)b * 4 + tid];
    else st[tid] = tid == 0 ? A.state[b] : A.state2[b];
  }
  if (tid < D) {
    obsum[tid] = A.ob_sum[(int64_t)b * D + tid];
    obsq[tid] = A.ob_sumsq[(int64_t)b * D + tid];
  }
  if (tid == 0) {
    tot[0] = A.rew_total[b];
    tot[1] = A.member_steps[b];
    tot[2] = A.env_steps[b];
  }
  bool alive = A.alive[b] != 0.0f;
  // launch invariants of the threads that build the observation
  float mean_k = 0.0f, std_k = 1.0f;
  if (tid < D) {
    mean_k = A.obmean[tid];
    std_k = A.obstd[tid];
  }
  const uint64_t seed0 = A.seed_dev ? *A.seed_dev : 0;
  const float ac_std = A.ac_std_dev ? *A.ac_std_dev : 0.0f;
  const int nout = A.sh.dims[A.sh.n_layers];
  __syncthreads();
  // the observation of the state a step starts from is the post-step one of
  // the step before: computed once, kept in LDS (Pendulum: one cosf, one sinf
  // per step instead of two)
  if (tid < D) ob[tid] = classic_ob(kind, st, tid);

  for (int t = 0; t < A.n_steps && alive; ++t) {
    if (tid < D)  // ob[tid] is this thread's own write
      bufA[tid] = fclampf((ob[tid] - mean_k) / std_k, -A.ob_clip, A.ob_clip);
    __syncthreads();
    const float* out;
    if constexpr (sizeof(WT) == 4)
      out = mlp_layers_f32(wb, A.sh, bufA, bufB, partial, tid, 256, A.act_final);
    else
      out = mlp_layers(wb, A.sh, bufA, bufB, partial, tid, 256, A.act_final);
    float a = 0.0f;
    if (tid == 0) {
      a = out[0];
      // the key of es_mlp_fwd at salt t + 1: the per-step engine's draw
      if (ac_std != 0.0f && b < A.noiseless_from)
        a += ac_std * es_actnoise(seed0 + A.salt_base + (uint64_t)t + 1, (uint64_t)b * nout);
    }
    if (tid == 0) {
      const float r = classic_env_step(kind, st, ob, a);
      tot[0] += r;
      tot[1] += 1.0f;
      tot[2] += 1.0f;
    }
    __syncthreads();
    if (tid < D) {
      // post-step observation, the terminal one included
      const float o = classic_ob(kind, st, tid);
      ob[tid] = o;
      obsum[tid] += (double)o;
      obsq[tid] += (double)o * (double)o;
    }
    bool done = tot[2] >= A.env_max_steps;
    if (kind == CLS_CARTPOLE)
      done = done || fabsf(st[0]) > CP_X_THRESHOLD || fabsf(st[2]) > CP_THETA_THRESHOLD;
    alive = !done;
    // the next step's first LDS writes are bufA and this thread's own ob[tid];
    // every write to st/tot sits behind the forward's barriers
  }

  __syncthreads();
  if (tid < S) {
    if (kind == CLS_CARTPOLE) A.state[(int64_t)b * 4 + tid] = st[tid];
    else if (tid == 0) A.state[b] = st[0];
    else A.state2[b] = st[1];
  }
  if (tid < D) {
    A.ob_sum[(int64_t)b * D + tid] = obsum[tid];
    A.ob_sumsq[(int64_t)b * D + tid] = obsq[tid];
  }
  if (tid == 0) {
    A.rew_total[b] = tot[0];
    A.member_steps[b] = tot[1];
    A.env_steps[b] = tot[2];
    A.alive[b] = alive ? 1.0f : 0.0f;
  }
}

__global__ void __launch_bounds__(256) classic_episode_kernel(ClassicArgs A) {
  classic_episode_body<uint16_t>(A);
}

__global__ void __launch_bounds__(256) classic_episode_f32_kernel(ClassicArgs A) {
  classic_episode_body<float>(A);
}

static inline int classic_launch(bool f32, const ClassicCall& c) {
  ClassicArgs A;
  const int rc = classic_args_init(&A, f32, c);
  if (rc) return rc;
  if (c.n_slots <= 0 || c.n_steps <= 0) return 0;
  const unsigned lds = (unsigned)(mlp_lds_bytes(A.sh.maxdim) + CLS_SLAB_BYTES);
  if (f32)
    classic_episode_f32_kernel<<<dim3((unsigned)c.n_slots), dim3(256), lds,
                                 (hipStream_t)c.stream>>>(A);
  else
    classic_episode_kernel<<<dim3((unsigned)c.n_slots), dim3(256), lds,
                             (hipStream_t)c.stream>>>(A);
  ES_CHECK_LAUNCH();
  return 0;
}

// Argument list and contract: CLASSIC_EPISODE_ENTRY (classic_env.h).
CLASSIC_EPISODE_ENTRY(es_classic_episode, classic_launch, false)
CLASSIC_EPISODE_ENTRY(es_classic_episode_f32, classic_launch, true)
