// Whole-episode rollout of the classic-control envs for SMALL nets (every
// layer at most 64 wide): a wavefront per evaluation slot.
//
// rollout_classic.hip gives a slot a 256-thread workgroup, which fits
// 376->256->256->17; a 4->32->32->1 net is 1 249 multiply-adds a step, and
// there most of the block idles between two block barriers per layer, the
// env step is a one-thread tail behind two more, and the slot's weight row
// comes from L2 again on every step. Here:
//
//  * a 256-thread block is four independent waves; wave w of block g owns
//    slot b = g * SPB + w for the whole launch (SPB = 4, 2 or 1 slots per
//    block, the most whose rows fit 64 KB of dynamic LDS; waves >= SPB and
//    waves with b >= n_slots return before touching memory);
//  * the wave copies its slot's row (row b / eps) into its own LDS region
//    once per launch; the step loop reads weights from LDS only;
//  * nothing behind the early return is a block barrier: the waves of a
//    block end at different steps. The wave reads only LDS it wrote itself,
//    so a wavefront-scope fence and a wave barrier order the copy before the
//    reads. All control flow is wave-uniform (the loop conditions go through
//    readfirstlane), so every cross-lane operation runs with the full wave;
//  * the slot's state, counters and reward live in registers, the same in
//    every lane, and every lane computes the env step: no serial tail. Lane
//    k < D keeps the fp64 moments of observation k.
//
// The row copy and the forward (wave_row_to_lds, wave_mlp_layers) are in
// wave_mlp.h, which rollout_tag_wave.hip shares.
//
// Contract, arguments and error codes are es_classic_episode's; a net with a
// layer wider than 64, or a row that does not fit the LDS budget alone, is
// -116 and launches nothing.
#include "classic_env.h"
#include "wave_mlp.h"

#define CLW_MAXW 64            // widest layer the lane mapping covers
#define CLW_LDS_BUDGET 65536   // dynamic LDS of a block
#define CLW_WAVES 4            // waves of a block

struct ClassicWaveArgs {
  ClassicArgs a;
  int n_slots;
  int spb;           // slots per block
  int region_bytes;  // LDS bytes of one wave's row, a multiple of 16
  int n_params;      // elements of a row
};

template <typename WT>
__device__ __forceinline__ void classic_wave_episode_body(const ClassicWaveArgs& W) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ClassicArgs& A = W.a;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * W.spb + wave;
  if (wave >= W.spb || b >= W.n_slots) return;
  // no block barrier from here on

  const int kind = A.kind;
  const int D = A.sh.dims[0];
  const int nout = A.sh.dims[A.sh.n_layers];
  WT* wl = reinterpret_cast<WT*>(smem + (size_t)wave * W.region_bytes);
  wave_row_to_lds(reinterpret_cast<const WT*>(A.weights) + (int64_t)(b / A.eps) * A.row_stride,
                  wl, W.n_params, lane);

  // slot state, the same in every lane
  float st[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (kind == CLS_CARTPOLE) {
#pragma unroll
    for (int k = 0; k < 4; ++k) st[k] = A.state[(int64_t)b * 4 + k];
  } else {
    st[0] = A.state[b];
    st[1] = A.state2[b];
  }
  float rew = A.rew_total[b], msteps = A.member_steps[b], esteps = A.env_steps[b];
  bool alive = __builtin_amdgcn_readfirstlane((int)(A.alive[b] != 0.0f)) != 0;
  // lane k < D owns observation k: its normalisation and its moments
  // (lanes >= D repeat observation D - 1 and store nothing)
  const int kk = min(lane, D - 1);
  const float mean_k = A.obmean[kk], std_k = A.obstd[kk];
  double obsum = A.ob_sum[(int64_t)b * D + kk], obsq = A.ob_sumsq[(int64_t)b * D + kk];
  const uint64_t seed0 = A.seed_dev ? *A.seed_dev : 0;
  const float ac_std = A.ac_std_dev ? *A.ac_std_dev : 0.0f;
  const bool noisy = ac_std != 0.0f && b < A.noiseless_from;

  // the observation a step starts from is the post-step one of the step before
  float ob[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < 3; ++k) ob[k] = classic_ob(kind, st, k);
  if (kind == CLS_CARTPOLE) ob[3] = st[3];

  for (int t = 0; t < A.n_steps && alive; ++t) {
    const float ob_k = kk == 0 ? ob[0] : kk == 1 ? ob[1] : kk == 2 ? ob[2] : ob[3];
    const float x = fclampf((ob_k - mean_k) / std_k, -A.ob_clip, A.ob_clip);
    float a = wave_mlp_layers(wl, A.sh, x, lane, A.act_final);
    // output 0 sits in lane 0; the draw is es_mlp_fwd's at salt t + 1
    if (noisy)
      a += ac_std * es_actnoise(seed0 + A.salt_base + (uint64_t)t + 1, (uint64_t)b * nout);
    a = clw_readlane(a, 0);
    rew += classic_env_step(kind, st, ob, a);
    msteps += 1.0f;
    esteps += 1.0f;
    // post-step observation, the terminal one included
#pragma unroll
    for (int k = 0; k < 3; ++k) ob[k] = classic_ob(kind, st, k);
    if (kind == CLS_CARTPOLE) ob[3] = st[3];
    const float o = kk == 0 ? ob[0] : kk == 1 ? ob[1] : kk == 2 ? ob[2] : ob[3];
    obsum += (double)o;
    obsq += (double)o * (double)o;
    bool done = esteps >= A.env_max_steps;
    if (kind == CLS_CARTPOLE)
      done = done || fabsf(st[0]) > CP_X_THRESHOLD || fabsf(st[2]) > CP_THETA_THRESHOLD;
    // every lane holds the same value; tell the compiler so
    alive = __builtin_amdgcn_readfirstlane((int)done) == 0;
  }

  if (lane == 0) {
    if (kind == CLS_CARTPOLE) {
#pragma unroll
      for (int k = 0; k < 4; ++k) A.state[(int64_t)b * 4 + k] = st[k];
    } else {
      A.state[b] = st[0];
      A.state2[b] = st[1];
    }
    A.rew_total[b] = rew;
    A.member_steps[b] = msteps;
    A.env_steps[b] = esteps;
    A.alive[b] = alive ? 1.0f : 0.0f;
  }
  if (lane < D) {
    A.ob_sum[(int64_t)b * D + lane] = obsum;
    A.ob_sumsq[(int64_t)b * D + lane] = obsq;
  }
}

// one template, named per weight type in the resource table and the profiles
template <typename WT>
__global__ void __launch_bounds__(256) CLW_KERNEL_ATTR
classic_wave_episode_kernel(ClassicWaveArgs W) {
  classic_wave_episode_body<WT>(W);
}

// Coverage, the one place it is decided: 0 and the launch geometry, or -116.
static inline int classic_wave_geometry(const MlpShape& sh, bool f32, int* spb,
                                        int* region_bytes, int* n_params) {
  for (int l = 0; l <= sh.n_layers; ++l)
    if (sh.dims[l] > CLW_MAXW) return -116;
  const int64_t n = sh.boff[sh.n_layers - 1] + sh.dims[sh.n_layers];
  const int64_t region = (n * (f32 ? 4 : 2) + 15) & ~(int64_t)15;
  if (region > CLW_LDS_BUDGET) return -116;
  *spb = 4 * region <= CLW_LDS_BUDGET ? 4 : 2 * region <= CLW_LDS_BUDGET ? 2 : 1;
  *region_bytes = (int)region;
  *n_params = (int)n;
  return 0;
}

static inline int classic_wave_launch(bool f32, void* state, void* state2, void* env_steps,
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
  ClassicWaveArgs W;
  int rc = classic_args_init(&W.a, f32, state, state2, env_steps, alive, member_steps,
                             rew_total, ob_sum, ob_sumsq, weights, obmean, obstd, dims_host,
                             ndims, row_stride, ob_clip, ac_std_dev, seed_dev, salt_base,
                             env_kind, ob_dim, env_max_steps, n_steps, eps, act_final,
                             noiseless_from);
  if (rc) return rc;
  rc = classic_wave_geometry(W.a.sh, f32, &W.spb, &W.region_bytes, &W.n_params);
  if (rc) return rc;
  if (n_slots <= 0 || n_steps <= 0) return 0;
  W.n_slots = n_slots;
  const dim3 grid((unsigned)((n_slots + W.spb - 1) / W.spb)), block(64 * CLW_WAVES);
  const unsigned lds = (unsigned)(W.spb * W.region_bytes);
  if (f32)
    classic_wave_episode_kernel<float><<<grid, block, lds, (hipStream_t)stream>>>(W);
  else
    classic_wave_episode_kernel<uint16_t><<<grid, block, lds, (hipStream_t)stream>>>(W);
  ES_CHECK_LAUNCH();
  return 0;
}

// What a launch with this net would return for its shape alone (0, one of
// mlp_shape_init's codes, -115 or -116), without launching.
extern "C" int es_classic_wave_check(const int32_t* dims_host, int32_t ndims,
                                     int64_t row_stride, int32_t f32) {
  MlpShape sh;
  int rc = mlp_shape_init(&sh, dims_host, ndims, row_stride);
  if (rc) return rc;
  if (sh.dims[sh.n_layers] < 1) return -115;
  int spb, region, n;
  return classic_wave_geometry(sh, f32 != 0, &spb, &region, &n);
}

// Argument list and contract of es_classic_episode (rollout_classic.hip).
extern "C" int es_classic_wave_episode(void* state, void* state2, void* env_steps,
                                       void* alive, void* member_steps, void* rew_total,
                                       void* ob_sum, void* ob_sumsq, const void* weights,
                                       const void* obmean, const void* obstd,
                                       const int32_t* dims_host, int32_t ndims,
                                       int64_t row_stride, float ob_clip,
                                       const void* ac_std_dev, const void* seed_dev,
                                       uint64_t salt_base, int32_t env_kind, int32_t ob_dim,
                                       int32_t env_max_steps, int32_t n_slots,
                                       int32_t n_steps, int32_t eps, int32_t act_final,
                                       int32_t noiseless_from, void* stream) {
  return classic_wave_launch(false, state, state2, env_steps, alive, member_steps, rew_total,
                             ob_sum, ob_sumsq, weights, obmean, obstd, dims_host, ndims,
                             row_stride, ob_clip, ac_std_dev, seed_dev, salt_base, env_kind,
                             ob_dim, env_max_steps, n_slots, n_steps, eps, act_final,
                             noiseless_from, stream);
}

// fp32 rows: same argument list; `weights` is float32 (rows, row_stride).
extern "C" int es_classic_wave_episode_f32(void* state, void* state2, void* env_steps,
                                           void* alive, void* member_steps, void* rew_total,
                                           void* ob_sum, void* ob_sumsq, const void* weights,
                                           const void* obmean, const void* obstd,
                                           const int32_t* dims_host, int32_t ndims,
                                           int64_t row_stride, float ob_clip,
                                           const void* ac_std_dev, const void* seed_dev,
                                           uint64_t salt_base, int32_t env_kind,
                                           int32_t ob_dim, int32_t env_max_steps,
                                           int32_t n_slots, int32_t n_steps, int32_t eps,
                                           int32_t act_final, int32_t noiseless_from,
                                           void* stream) {
  return classic_wave_launch(true, state, state2, env_steps, alive, member_steps, rew_total,
                             ob_sum, ob_sumsq, weights, obmean, obstd, dims_host, ndims,
                             row_stride, ob_clip, ac_std_dev, seed_dev, salt_base, env_kind,
                             ob_dim, env_max_steps, n_slots, n_steps, eps, act_final,
                             noiseless_from, stream);
}
