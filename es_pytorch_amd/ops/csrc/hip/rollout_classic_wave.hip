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

// The coverage (wave_mlp.h): 0 and the geometry of W, or -116.
static inline int classic_wave_geometry(const MlpShape& sh, bool f32, ClassicWaveArgs* W) {
  W->n_params = wave_row_elems(sh);
  if (W->n_params < 0) return W->n_params;
  W->region_bytes = wave_row_bytes(W->n_params, f32);
  W->spb = wave_regions_per_block(W->region_bytes);
  return W->spb < 0 ? W->spb : 0;
}

static inline int classic_wave_launch(bool f32, const ClassicCall& c) {
  ClassicWaveArgs W;
  int rc = classic_args_init(&W.a, f32, c);
  if (rc) return rc;
  rc = classic_wave_geometry(W.a.sh, f32, &W);
  if (rc) return rc;
  if (c.n_slots <= 0 || c.n_steps <= 0) return 0;
  W.n_slots = c.n_slots;
  const dim3 grid((unsigned)((c.n_slots + W.spb - 1) / W.spb)), block(64 * WAVE_WAVES);
  const unsigned lds = (unsigned)(W.spb * W.region_bytes);
  if (f32)
    classic_wave_episode_kernel<float><<<grid, block, lds, (hipStream_t)c.stream>>>(W);
  else
    classic_wave_episode_kernel<uint16_t><<<grid, block, lds, (hipStream_t)c.stream>>>(W);
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
  ClassicWaveArgs W;
  return classic_wave_geometry(sh, f32 != 0, &W);
}

// Argument list and contract: CLASSIC_EPISODE_ENTRY (classic_env.h).
CLASSIC_EPISODE_ENTRY(es_classic_wave_episode, classic_wave_launch, false)
CLASSIC_EPISODE_ENTRY(es_classic_wave_episode_f32, classic_wave_launch, true)
