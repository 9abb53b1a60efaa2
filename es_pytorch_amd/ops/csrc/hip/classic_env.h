// What the classic-control episode kernels share (rollout_classic.hip: a
// workgroup per slot; rollout_classic_wave.hip: a wavefront per slot): the env
// constants, the observation and the env step of BatchedCartPole /
// BatchedPendulum (envs/classic.py), the launch arguments and their checks,
// and the C argument list of the entry points.
#pragma once
#include "mlp_core.h"

#define CLS_CARTPOLE 0
#define CLS_PENDULUM 1
#define CLS_MAXOB 4

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

// One env step on st with action a, in the env's op order in fp32; returns the
// reward. ob is the observation of the pre-step state (Pendulum reads its
// cos th and sin th there).
__device__ __forceinline__ float classic_env_step(int kind, float* st, const float* ob,
                                                  float a) {
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
  return r;
}

// One call's arguments, in the order of CLASSIC_EPISODE_ENTRY's list.
struct ClassicCall {
  void *state, *state2, *env_steps, *alive, *member_steps, *rew_total, *ob_sum, *ob_sumsq;
  const void *weights, *obmean, *obstd;
  const int32_t* dims_host;
  int32_t ndims;
  int64_t row_stride;
  float ob_clip;
  const void *ac_std_dev, *seed_dev;
  uint64_t salt_base;
  int32_t env_kind, ob_dim, env_max_steps, n_slots, n_steps, eps, act_final, noiseless_from;
  void* stream;
};

// The argument checks both launchers make, in this order, and the fill of A.
// 0: launch; a negative code: launch nothing.
static inline int classic_args_init(ClassicArgs* Ap, bool f32, const ClassicCall& c) {
  ClassicArgs& A = *Ap;
  int rc = mlp_shape_init(&A.sh, c.dims_host, c.ndims, c.row_stride);
  if (rc) return rc;
  if (f32) mlp_shape_vec_f32(&A.sh, c.row_stride);
  if (c.env_kind != CLS_CARTPOLE && c.env_kind != CLS_PENDULUM) return -113;
  const int want_ob = c.env_kind == CLS_CARTPOLE ? 4 : 3;
  if (c.ob_dim != want_ob || A.sh.dims[0] != want_ob) return -114;
  if (A.sh.dims[A.sh.n_layers] < 1) return -115;
  A.state = (float*)c.state;
  A.state2 = (float*)c.state2;
  A.env_steps = (float*)c.env_steps;
  A.alive = (float*)c.alive;
  A.member_steps = (float*)c.member_steps;
  A.rew_total = (float*)c.rew_total;
  A.ob_sum = (double*)c.ob_sum;
  A.ob_sumsq = (double*)c.ob_sumsq;
  A.weights = c.weights;
  A.obmean = (const float*)c.obmean;
  A.obstd = (const float*)c.obstd;
  A.ac_std_dev = (const float*)c.ac_std_dev;
  A.seed_dev = (const uint64_t*)c.seed_dev;
  A.salt_base = c.salt_base;
  A.row_stride = c.row_stride;
  A.ob_clip = c.ob_clip;
  A.env_max_steps = (float)c.env_max_steps;
  A.kind = c.env_kind;
  A.n_steps = c.n_steps;
  A.eps = c.eps > 0 ? c.eps : 1;
  A.act_final = c.act_final;
  A.noiseless_from = c.noiseless_from;
  return 0;
}

// Defines the extern "C" entry point `name`, which calls
// launcher(f32, const ClassicCall&). The argument list of every entry point
// (es_classic_episode[_f32], es_classic_wave_episode[_f32]):
//
// State, (n_slots, ...) each, read at launch and written back at the end:
// CartPole (env_kind 0, ob_dim 4): state float (., 4) = x, x_dot, theta,
// theta_dot; state2 unused. Pendulum (env_kind 1, ob_dim 3): state = th,
// state2 = thdot, float (.) each. env_steps (the env's own counter, which ends
// the episode at env_max_steps), alive, member_steps, rew_total float (.);
// ob_sum, ob_sumsq double (., ob_dim). weights: (rows, row_stride), bf16 or,
// for an _f32 entry point, float32; slot b on row b / eps; obmean/obstd float
// (ob_dim); ac_std_dev float (1) or null.
// Step t of the launch (0-based) draws the action noise of slots below
// noiseless_from with key *seed_dev + salt_base + t + 1 at counter b * A, A
// the net's output width: es_mlp_fwd's draw at salt salt_base + t + 1.
#define CLASSIC_EPISODE_ENTRY(name, launcher, f32)                                          \
  extern "C" int name(                                                                      \
      void* state, void* state2, void* env_steps, void* alive, void* member_steps,          \
      void* rew_total, void* ob_sum, void* ob_sumsq, const void* weights,                   \
      const void* obmean, const void* obstd, const int32_t* dims_host, int32_t ndims,       \
      int64_t row_stride, float ob_clip, const void* ac_std_dev, const void* seed_dev,      \
      uint64_t salt_base, int32_t env_kind, int32_t ob_dim, int32_t env_max_steps,          \
      int32_t n_slots, int32_t n_steps, int32_t eps, int32_t act_final,                     \
      int32_t noiseless_from, void* stream) {                                               \
    return launcher(                                                                        \
        f32, ClassicCall{state, state2, env_steps, alive, member_steps, rew_total, ob_sum,  \
                         ob_sumsq, weights, obmean, obstd, dims_host, ndims, row_stride,    \
                         ob_clip, ac_std_dev, seed_dev, salt_base, env_kind, ob_dim,        \
                         env_max_steps, n_slots, n_steps, eps, act_final, noiseless_from,   \
                         stream});                                                          \
  }
