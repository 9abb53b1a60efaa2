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
#include "mlp_core.h"

#define CLS_CARTPOLE 0
#define CLS_PENDULUM 1
#define CLS_MAXOB 4
// slot slab behind the mlp carve: fp64 ob_sum[4], ob_sumsq[4], then float
// st[4] (the env state), ob[4] (its observation), rew, member steps, env
// steps, pad
#define CLS_SLAB_BYTES (2 * CLS_MAXOB * 8 + 12 * 4)

// The float32 values of the Python doubles the envs compute with.
#define CP_GRAVITY 9.8f
#define CP_MASSPOLE 0.1f
#define CP_TOTAL_MASS ((float)(0.1 + 1.0))
#define CP_LENGTH 0.5f
#define CP_POLEMASS_LENGTH ((float)(0.1 * 0.5))
#define CP_FORCE_MAG 10.0f
#define CP_TAU 0.02f
#define CP_FOUR_THIRDS ((float)(4.0 / 3.0))
#define CP_THETA_THRESHOLD ((float)(12 * 2 * 3.141592653589793 / 360))
#define CP_X_THRESHOLD 2.4f
#define PD_MAX_SPEED 8.0f
#define PD_MAX_TORQUE 2.0f
#define PD_DT 0.05f
#define PD_GRAV_COEF ((float)(3 * 10.0 / (2 * 1.0)))     // 3 g / (2 l)
#define PD_TORQUE_COEF ((float)(3.0 / (1.0 * 1.0 * 1.0)))  // 3 / (m l^2)

struct ClassicArgs {
  float* state;         // CartPole (n, 4); Pendulum th (n)
  float* state2;        // Pendulum thdot (n); CartPole: unused
  float* env_steps;     // the env's own step counter (n)
  float* alive;         // (n)
  float* member_steps;  // (n)
  float* rew_total;     // (n)
  double* ob_sum;       // (n, D)
  double* ob_sumsq;     // (n, D)
  const void* weights;
  const float* obmean;
  const float* obstd;
  const float* ac_std_dev;
  const uint64_t* seed_dev;
  uint64_t salt_base;
  int64_t row_stride;
  float ob_clip;
  float env_max_steps;
  int kind, n_steps, eps, act_final, noiseless_from;
  MlpShape sh;
};

// Observation k of env state st (CartPole: the state; Pendulum st = th, thdot).
__device__ __forceinline__ float classic_ob(int kind, const float* st, int k) {
  if (kind == CLS_CARTPOLE) return st[k];
  return k == 0 ? cosf(st[0]) : k == 1 ? sinf(st[0]) : st[1];
}

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
#pragma clang fp contract(off)
      float r;
      if (kind == CLS_CARTPOLE) {
        // BatchedCartPole.step, op for op in fp32
        const float force = a > 0.0f ? CP_FORCE_MAG : -CP_FORCE_MAG;
        const float x = st[0], x_dot = st[1], theta = st[2], theta_dot = st[3];
        const float costheta = cosf(theta), sintheta = sinf(theta);
        const float temp =
            (force + CP_POLEMASS_LENGTH * (theta_dot * theta_dot) * sintheta) / CP_TOTAL_MASS;
        const float thetaacc =
            (CP_GRAVITY * sintheta - costheta * temp) /
            (CP_LENGTH *
             (CP_FOUR_THIRDS - CP_MASSPOLE * (costheta * costheta) / CP_TOTAL_MASS));
        const float xacc = temp - CP_POLEMASS_LENGTH * thetaacc * costheta / CP_TOTAL_MASS;
        st[0] = x + CP_TAU * x_dot;
        st[1] = x_dot + CP_TAU * xacc;
        st[2] = theta + CP_TAU * theta_dot;
        st[3] = theta_dot + CP_TAU * thetaacc;
        r = 1.0f;
      } else {
        // BatchedPendulum.step; ob = (cos th, sin th, thdot) of the pre-step state
        const float u = fclampf(a, -PD_MAX_TORQUE, PD_MAX_TORQUE);
        const float th = st[0], thdot = st[1];
        const float costh = ob[0], sinth = ob[1];
        const float th_norm = atan2f(sinth, costh);
        const float cost = th_norm * th_norm + 0.1f * (thdot * thdot) + 0.001f * (u * u);
        float nd = thdot + (PD_GRAV_COEF * sinth + PD_TORQUE_COEF * u) * PD_DT;
        nd = fclampf(nd, -PD_MAX_SPEED, PD_MAX_SPEED);
        st[0] = th + nd * PD_DT;
        st[1] = nd;
        r = -cost;
      }
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

static inline int classic_launch(bool f32, void* state, void* state2, void* env_steps,
                                 void* alive, void* member_steps, void* rew_total,
                                 void* ob_sum, void* ob_sumsq, const void* weights,
                                 const void* obmean, const void* obstd,
                                 const int32_t* dims_host, int32_t ndims, int64_t row_stride,
                                 float ob_clip, const void* ac_std_dev, const void* seed_dev,
                                 uint64_t salt_base, int32_t env_kind, int32_t ob_dim,
                                 int32_t env_max_steps, int32_t n_slots, int32_t n_steps,
                                 int32_t eps, int32_t act_final, int32_t noiseless_from,
                                 void* stream) {
  ClassicArgs A;
  int rc = mlp_shape_init(&A.sh, dims_host, ndims, row_stride);
  if (rc) return rc;
  if (f32) mlp_shape_vec_f32(&A.sh, row_stride);
  if (env_kind != CLS_CARTPOLE && env_kind != CLS_PENDULUM) return -113;
  const int want_ob = env_kind == CLS_CARTPOLE ? 4 : 3;
  if (ob_dim != want_ob || A.sh.dims[0] != want_ob) return -114;
  if (A.sh.dims[A.sh.n_layers] < 1) return -115;
  if (n_slots <= 0 || n_steps <= 0) return 0;
  A.state = (float*)state;
  A.state2 = (float*)state2;
  A.env_steps = (float*)env_steps;
  A.alive = (float*)alive;
  A.member_steps = (float*)member_steps;
  A.rew_total = (float*)rew_total;
  A.ob_sum = (double*)ob_sum;
  A.ob_sumsq = (double*)ob_sumsq;
  A.weights = weights;
  A.obmean = (const float*)obmean;
  A.obstd = (const float*)obstd;
  A.ac_std_dev = (const float*)ac_std_dev;
  A.seed_dev = (const uint64_t*)seed_dev;
  A.salt_base = salt_base;
  A.row_stride = row_stride;
  A.ob_clip = ob_clip;
  A.env_max_steps = (float)env_max_steps;
  A.kind = env_kind;
  A.n_steps = n_steps;
  A.eps = eps > 0 ? eps : 1;
  A.act_final = act_final;
  A.noiseless_from = noiseless_from;
  const unsigned lds = (unsigned)(mlp_lds_bytes(A.sh.maxdim) + CLS_SLAB_BYTES);
  if (f32)
    classic_episode_f32_kernel<<<dim3((unsigned)n_slots), dim3(256), lds,
                                 (hipStream_t)stream>>>(A);
  else
    classic_episode_kernel<<<dim3((unsigned)n_slots), dim3(256), lds,
                             (hipStream_t)stream>>>(A);
  ES_CHECK_LAUNCH();
  return 0;
}

// State, (n_slots, ...) each, read at launch and written back at the end:
// CartPole (env_kind 0, ob_dim 4): state float (., 4) = x, x_dot, theta,
// theta_dot; state2 unused. Pendulum (env_kind 1, ob_dim 3): state = th,
// state2 = thdot, float (.) each. env_steps (the env's own counter, which ends
// the episode at env_max_steps), alive, member_steps, rew_total float (.);
// ob_sum, ob_sumsq double (., ob_dim). weights: bf16 (rows, row_stride), slot
// b on row b / eps; obmean/obstd float (ob_dim); ac_std_dev float (1) or null.
// Step t of the launch (0-based) draws the action noise of slots below
// noiseless_from with key *seed_dev + salt_base + t + 1 at counter b * A, A
// the net's output width: es_mlp_fwd's draw at salt salt_base + t + 1.
extern "C" int es_classic_episode(void* state, void* state2, void* env_steps, void* alive,
                                  void* member_steps, void* rew_total, void* ob_sum,
                                  void* ob_sumsq, const void* weights, const void* obmean,
                                  const void* obstd, const int32_t* dims_host, int32_t ndims,
                                  int64_t row_stride, float ob_clip, const void* ac_std_dev,
                                  const void* seed_dev, uint64_t salt_base, int32_t env_kind,
                                  int32_t ob_dim, int32_t env_max_steps, int32_t n_slots,
                                  int32_t n_steps, int32_t eps, int32_t act_final,
                                  int32_t noiseless_from, void* stream) {
  return classic_launch(false, state, state2, env_steps, alive, member_steps, rew_total,
                        ob_sum, ob_sumsq, weights, obmean, obstd, dims_host, ndims,
                        row_stride, ob_clip, ac_std_dev, seed_dev, salt_base, env_kind,
                        ob_dim, env_max_steps, n_slots, n_steps, eps, act_final,
                        noiseless_from, stream);
}

// fp32 rows: same argument list; `weights` is float32 (rows, row_stride).
extern "C" int es_classic_episode_f32(void* state, void* state2, void* env_steps,
                                      void* alive, void* member_steps, void* rew_total,
                                      void* ob_sum, void* ob_sumsq, const void* weights,
                                      const void* obmean, const void* obstd,
                                      const int32_t* dims_host, int32_t ndims,
                                      int64_t row_stride, float ob_clip,
                                      const void* ac_std_dev, const void* seed_dev,
                                      uint64_t salt_base, int32_t env_kind, int32_t ob_dim,
                                      int32_t env_max_steps, int32_t n_slots, int32_t n_steps,
                                      int32_t eps, int32_t act_final, int32_t noiseless_from,
                                      void* stream) {
  return classic_launch(true, state, state2, env_steps, alive, member_steps, rew_total,
                        ob_sum, ob_sumsq, weights, obmean, obstd, dims_host, ndims,
                        row_stride, ob_clip, ac_std_dev, seed_dev, salt_base, env_kind,
                        ob_dim, env_max_steps, n_slots, n_steps, eps, act_final,
                        noiseless_from, stream);
}
