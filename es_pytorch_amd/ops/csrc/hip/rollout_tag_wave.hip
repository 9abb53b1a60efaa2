// Whole-episode rollout of the PursuitTag game for SMALL co-evolution nets
// (every layer of both policies at most 64 wide): a wavefront per game.
//
// rollout_tag.hip gives a game a 256-thread workgroup: two mlp_layers per
// step, each with two block barriers per layer, a one-to-four-thread env step
// behind two more, and both member rows re-read from L2 on every step. On
// 8->32->32->2 (1 410 multiply-adds a forward) most of that block idles. Here,
// as in rollout_classic_wave.hip:
//
//  * a 256-thread block is four independent waves; wave w of block g owns
//    game b = g * GPB + w for the whole launch (GPB = 4, 2 or 1 games per
//    block, the most whose row pairs fit 64 KB of dynamic LDS; waves >= GPB
//    and waves with b >= n_games return before touching memory);
//  * the wave copies row b of BOTH policies' blobs into its own LDS region
//    once per launch (blob 0's row at offset 0, blob 1's behind it, 16-B
//    padded); the step loop reads weights from LDS only;
//  * nothing behind the early return is a block barrier: the waves of a block
//    end at different steps. All control flow is wave-uniform (the loop
//    condition goes through readfirstlane);
//  * p, v, the reward totals and the step count live in registers, the same
//    in every lane. Lane k < 8 builds observation k of an agent from them by
//    selects and normalizes it; the two forwards (wave_mlp_layers, wave_mlp.h)
//    run one after the other on the pre-step state; raw action j of an agent
//    is in lane j, gets its noise there and is broadcast with readlane; every
//    lane then computes the env step: no serial tail. Lane l < 16 keeps the
//    fp64 moments of observation l & 7 of agent l >> 3.
//
// Contract, arguments, noise keys and error codes are es_tag_episode's; a
// policy with a layer wider than 64, or a row pair that does not fit the LDS
// budget alone, is -116 and launches nothing.
#include "tag_env.h"
#include "wave_mlp.h"

struct TagWaveArgs {
  float *p, *v, *alive, *steps, *rew;  // (n, 2, 2) x2, (n), (n), (n, 2)
  double *obsum, *obsq;                // (n, 2, 8)
  TagPolicy P0, P1;
  const uint64_t* seed_dev;
  uint64_t salt_base;
  int n_games, n_steps, act_final, noiseless_from;
  int gpb;           // games per block
  int region_bytes;  // LDS bytes of one wave's two rows, a multiple of 16
  int row1_bytes;    // where blob 1's row starts in the region
  int n0, n1;        // elements of a row of blob 0 / blob 1
};

// st[idx] for a per-lane idx in 0..7, st in registers: a tree of selects on
// the bits of idx (written as an indexed read, or as a chain of idx == j
// selects, the array goes to scratch memory).
__device__ __forceinline__ float tgw_pick(const float (&st)[8], int idx) {
  const bool b0 = idx & 1, b1 = idx & 2, b2 = idx & 4;
  const float s01 = b0 ? st[1] : st[0], s23 = b0 ? st[3] : st[2];
  const float s45 = b0 ? st[5] : st[4], s67 = b0 ? st[7] : st[6];
  const float lo = b1 ? s23 : s01, hi = b1 ? s67 : s45;
  return b2 ? hi : lo;
}

// BatchedPursuitTag.step on st with the raw actions act[agent][xy], op for op
// in fp32 as tag_episode_kernel has it; returns the distance after the step.
__device__ __forceinline__ float tgw_env_step(float (&st)[8], const float (&act)[4]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < 4; ++k) tag_move(st[k], st[4 + k], act[k]);
  const float dx = st[0] - st[2], dy = st[1] - st[3];
  return sqrtf(dx * dx + dy * dy);
}

// Agent i's forward on the pre-step state st and its row wl: lane j < 2
// returns raw action j, noise added.
template <typename WT>
__device__ __forceinline__ float tgw_agent_forward(const TagPolicy& P, const WT* wl,
                                                   const float (&st)[8], int ob_idx,
                                                   float mean_k, float std_k, bool noisy,
                                                   float ac_std, uint64_t seed, int b,
                                                   int act_final, int lane) {
  const float ob = tgw_pick(st, ob_idx);
  const float x = fclampf((ob - mean_k) / std_k, -P.ob_clip, P.ob_clip);
  float a = wave_mlp_layers(wl, P.sh, x, lane, act_final);
  // output j sits in lane j; the draw is es_mlp_fwd's for output j of member b
  if (noisy)
    a += ac_std * es_actnoise(seed, (uint64_t)b * P.sh.dims[P.sh.n_layers] + (lane & 1));
  return a;
}

template <typename WT>
__global__ void __launch_bounds__(256) CLW_KERNEL_ATTR
tag_wave_episode_kernel(TagWaveArgs W) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * W.gpb + wave;
  if (wave >= W.gpb || b >= W.n_games) return;
  // no block barrier from here on

  char* region = smem + (size_t)wave * W.region_bytes;
  WT* wl0 = reinterpret_cast<WT*>(region);
  WT* wl1 = reinterpret_cast<WT*>(region + W.row1_bytes);
  wave_row_to_lds(reinterpret_cast<const WT*>(W.P0.weights) + (int64_t)b * W.P0.row_stride,
                  wl0, W.n0, lane);
  wave_row_to_lds(reinterpret_cast<const WT*>(W.P1.weights) + (int64_t)b * W.P1.row_stride,
                  wl1, W.n1, lane);

  // game state, the same in every lane: p[2][2] v[2][2]
  float st[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    st[k] = W.p[(int64_t)b * 4 + k];
    st[4 + k] = W.v[(int64_t)b * 4 + k];
  }
  float rew0 = W.rew[(int64_t)b * 2], rew1 = W.rew[(int64_t)b * 2 + 1];
  float steps = W.steps[b];
  bool alive = __builtin_amdgcn_readfirstlane((int)(W.alive[b] != 0.0f)) != 0;
  // lane k < 8 owns observation k of either agent: its normalisation
  // (lanes >= 8 repeat observation k & 7; the forward reads lanes < 8 only)
  const int k8 = lane & 7;
  const int ob_idx0 = tag_ob_index(0, k8), ob_idx1 = tag_ob_index(1, k8);
  const float mean0 = W.P0.obmean[k8], std0 = W.P0.obstd[k8];
  const float mean1 = W.P1.obmean[k8], std1 = W.P1.obstd[k8];
  // lane l < 16 owns the moments of observation l & 7 of agent l >> 3
  // (lanes >= 16 repeat lane l & 15 and store nothing)
  const int l16 = lane & 15;
  const int mom_idx = tag_ob_index(l16 >> 3, k8);
  double obsum = W.obsum[(int64_t)b * 2 * TAG_OB + l16];
  double obsq = W.obsq[(int64_t)b * 2 * TAG_OB + l16];
  const uint64_t seed0 = W.seed_dev ? *W.seed_dev : 0;
  const float ac_std0 = W.P0.ac_std_dev ? *W.P0.ac_std_dev : 0.0f;
  const float ac_std1 = W.P1.ac_std_dev ? *W.P1.ac_std_dev : 0.0f;
  const bool noisy0 = ac_std0 != 0.0f && b < W.noiseless_from;
  const bool noisy1 = ac_std1 != 0.0f && b < W.noiseless_from;

  for (int t = 0; t < W.n_steps && alive; ++t) {
    // the key of es_mlp_fwd at salt (t+1)*2 + i: the per-step engine's draw
    const uint64_t seed = seed0 + (W.salt_base + (uint64_t)t + 1) * 2;
    const float a0 = tgw_agent_forward(W.P0, wl0, st, ob_idx0, mean0, std0, noisy0, ac_std0,
                                       seed, b, W.act_final, lane);
    const float a1 = tgw_agent_forward(W.P1, wl1, st, ob_idx1, mean1, std1, noisy1, ac_std1,
                                       seed + 1, b, W.act_final, lane);
    const float act[4] = {clw_readlane(a0, 0), clw_readlane(a0, 1), clw_readlane(a1, 0),
                          clw_readlane(a1, 1)};
    const float d = tgw_env_step(st, act);
    const bool caught = d < TAG_CATCH_DIST;
    tag_reward(d, caught, rew0, rew1);
    steps += 1.0f;
    // post-step observation, the terminal one included
    const double o = (double)tgw_pick(st, mom_idx);
    obsum += o;
    obsq += o * o;
    // every lane holds the same value; tell the compiler so
    alive = __builtin_amdgcn_readfirstlane((int)caught) == 0;
  }

  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      W.p[(int64_t)b * 4 + k] = st[k];
      W.v[(int64_t)b * 4 + k] = st[4 + k];
    }
    W.rew[(int64_t)b * 2] = rew0;
    W.rew[(int64_t)b * 2 + 1] = rew1;
    W.steps[b] = steps;
    W.alive[b] = alive ? 1.0f : 0.0f;
  }
  if (lane < 2 * TAG_OB) {
    W.obsum[(int64_t)b * 2 * TAG_OB + lane] = obsum;
    W.obsq[(int64_t)b * 2 * TAG_OB + lane] = obsq;
  }
}

// The shared checks (tag_policies_init), then the coverage: fills the policies
// and the geometry of W.
static inline int tag_wave_init(TagWaveArgs* W, bool f32, const TagCall& c) {
  const int rc = tag_policies_init(c, f32, &W->P0, &W->P1);
  if (rc) return rc;
  W->n0 = wave_row_elems(W->P0.sh);
  W->n1 = wave_row_elems(W->P1.sh);
  if (W->n0 < 0 || W->n1 < 0) return -116;
  W->row1_bytes = wave_row_bytes(W->n0, f32);
  W->region_bytes = W->row1_bytes + wave_row_bytes(W->n1, f32);
  W->gpb = wave_regions_per_block(W->region_bytes);
  return W->gpb < 0 ? W->gpb : 0;
}

static inline int tag_wave_launch(bool f32, const TagCall& c) {
  TagWaveArgs W;
  const int rc = tag_wave_init(&W, f32, c);
  if (rc) return rc;
  if (c.n_games <= 0 || c.n_steps <= 0) return 0;
  W.p = (float*)c.p;
  W.v = (float*)c.v;
  W.alive = (float*)c.alive;
  W.steps = (float*)c.steps;
  W.rew = (float*)c.rew_total;
  W.obsum = (double*)c.ob_sum;
  W.obsq = (double*)c.ob_sumsq;
  W.seed_dev = (const uint64_t*)c.seed_dev;
  W.salt_base = c.salt_base;
  W.n_games = c.n_games;
  W.n_steps = c.n_steps;
  W.act_final = c.act_final;
  W.noiseless_from = c.noiseless_from;
  const dim3 grid((unsigned)((c.n_games + W.gpb - 1) / W.gpb)), block(64 * WAVE_WAVES);
  const unsigned lds = (unsigned)(W.gpb * W.region_bytes);
  if (f32)
    tag_wave_episode_kernel<float><<<grid, block, lds, (hipStream_t)c.stream>>>(W);
  else
    tag_wave_episode_kernel<uint16_t><<<grid, block, lds, (hipStream_t)c.stream>>>(W);
  ES_CHECK_LAUNCH();
  return 0;
}

// What a launch with this pair of nets would return for the shapes alone (0,
// one of mlp_shape_init's codes, -110, -111 or -116), without launching.
extern "C" int es_tag_wave_check(const int32_t* dims0_host, int32_t ndims0,
                                 const int32_t* dims1_host, int32_t ndims1,
                                 int64_t row_stride0, int64_t row_stride1, int32_t f32) {
  TagCall c{};
  c.dims0_host = dims0_host;
  c.ndims0 = ndims0;
  c.dims1_host = dims1_host;
  c.ndims1 = ndims1;
  c.row_stride0 = row_stride0;
  c.row_stride1 = row_stride1;
  c.n_agents = 2;
  c.ob_dim = TAG_OB;
  TagWaveArgs W;
  return tag_wave_init(&W, f32 != 0, c);
}

// Argument list and contract: TAG_EPISODE_ENTRY (tag_env.h).
TAG_EPISODE_ENTRY(es_tag_wave_episode, tag_wave_launch, false)
TAG_EPISODE_ENTRY(es_tag_wave_episode_f32, tag_wave_launch, true)
