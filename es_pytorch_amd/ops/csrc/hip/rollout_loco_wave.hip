// Whole-episode rollout of the synthetic locomotion envs for SMALL envs and
// nets (state dim and every layer at most 64 wide): a wavefront per slot.
//
// rollout_loco.hip gives a slot a 256-thread workgroup, which fits Humanoid's
// 376 -> 256 -> 256 -> 17; Hopper's 11 -> 64 -> 64 -> 3 fills a quarter of a
// wave, and there the block waits at several barriers per layer and in the
// epilogue, reads the member row and the A matrix from L2 again on every step
// and goes on stepping a slot that fell. Here:
//
//  * a 256-thread block is four independent waves; wave w of block g owns
//    slot b = member_base + g * SPB + w for the whole launch (SPB = 4, 2 or 1,
//    the most row regions that fit 64 KB of dynamic LDS beside the env block);
//  * the env block - A (bf16), B, b0, wv, wy, wh, wa, obmean, obstd - is
//    staged into LDS once per block by all 256 threads. The __syncthreads()
//    behind it, ahead of every return, is the only block barrier: the waves
//    of a block end at different steps;
//  * each wave copies its slot's row (row b / eps - wrow0) into its own LDS
//    region; the step loop reads weights and env matrices from LDS only;
//  * the slot lives in registers for the whole launch: lane i < S holds s[i],
//    lane o < D the running mo_sum[o] and mo_sumsq[o], and pos, goal,
//    rew_total, member_steps and alive are the same value in every lane.
//    Global memory is read once on entry and written once on exit;
//  * the forward is wave_mlp_layers (wave_mlp.h); the dynamics matvec uses
//    its lane mapping on A and B (lane owns output l % OP and input partition
//    l / OP, an ascending fmaf chain, the fixed butterfly), so the order of
//    every sum is fixed by the shape alone; vfwd, vy, h and |a|^2 are
//    xor-butterfly sums that leave the same bits in every lane, and every
//    lane computes the reward, the position and the fall test;
//  * all control flow around cross-lane operations is wave-uniform (the loop
//    condition goes through readfirstlane).
//
// A wave leaves the loop as soon as its slot is no longer alive, and a slot
// that enters dead writes nothing. This differs from es_loco_episode, which
// goes on stepping s and pos of a dead slot: here they keep their values from
// the step at which the slot died. Nothing in the engine reads them after
// that (behv, which it does read, is frozen by both kernels).
//
// Arguments and return codes are es_loco_episode's without block_threads; a
// layer or a state wider than 64, or a row that does not fit the LDS budget
// beside the env block, is -116 and launches nothing.
#include "loco_env.h"
#include "wave_mlp.h"

struct LocoWaveArgs {
  MlpShape sh;
  LocoArgs la;
  LocoPtrs P;
  int member_base, n_members, n_steps, salt_base;
  int spb;           // slots per block
  int env_bytes;     // LDS bytes of the env block, a multiple of 16
  int region_bytes;  // LDS bytes of one wave's row, a multiple of 16
  int n_params;      // elements of a row
};

// The env block in LDS, carved the same way by the host (its size) and the
// kernel: A in bf16, padded to 16 B, then the float arrays.
__host__ __device__ __forceinline__ int loco_wave_a_bytes(int S) {
  return (S * S * 2 + 15) & ~15;
}
__host__ __device__ __forceinline__ int loco_wave_env_floats(int S, int A, int D) {
  return A * S + 4 * S + A + 2 * D;  // Bm | b0 wv wy wh | wa | obmean obstd
}

// acc + sum_i x[i] * M[i][o] over the rows i of this lane's partition p of
// M (I rows, O wide, in LDS), x[i] read from lane i: the trips, the clamped
// reads behind a lane's last input and the hand-written fours are those of
// wave_mlp_layers. lg = log2 OP; the caller runs the butterfly.
template <typename MT>
__device__ __forceinline__ float loco_wave_dot(const MT* M, int I, int O, int lg, int o,
                                               int p, float x, float acc) {
  if (lg == 6) {
    auto wx = [&](int i, float& w, float& xi) {
      w = clw_weight(M, i * O + o);
      xi = clw_readlane(x, i);
    };
    int i = 0;
    for (; i + 4 <= I; i += 4) {
      float w[4], xi[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) wx(i + u, w[u], xi[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = fmaf(xi[u], w[u], acc);
    }
    for (; i < I; ++i) {
      float w, xi;
      wx(i, w, xi);
      acc = fmaf(xi, w, acc);
    }
  } else {
    const int P = 64 >> lg, T = (I + P - 1) >> (6 - lg);
    auto wx = [&](int k, float& w, float& xi) {  // returns: the trip has an input
      const int i = p + (k << (6 - lg));
      const int ic = min(i, I - 1);
      w = clw_weight(M, ic * O + o);
      xi = __shfl(x, ic, 64);
      return i < I;
    };
    int k = 0;
    for (; k + 4 <= T; k += 4) {
      float w[4], xi[4];
      bool ok[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) ok[u] = wx(k + u, w[u], xi[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = ok[u] ? fmaf(xi[u], w[u], acc) : acc;
    }
    for (; k < T; ++k) {
      float w, xi;
      const bool ok = wx(k, w, xi);
      acc = ok ? fmaf(xi, w, acc) : acc;
    }
  }
  return acc;
}

// a + b on both sides of every exchange: every lane ends on the same bits
__device__ __forceinline__ float loco_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Net output (output j in lane j) -> the clamped env action, action k in lane
// k < A and 0 in the lanes behind: loco_decode_action's four modes, its tie
// rule and its noise keys and counters.
__device__ __forceinline__ float loco_wave_decode(const LocoArgs& la, int odim, int b,
                                                  uint64_t seed, float ac_std, float out,
                                                  int lane) {
  const int A = la.A;
  const bool mine = lane < A;
  float a;
  if (la.act_mode == 2 || la.act_mode == 3) {
    // integrated gaussian actions: mode 2 keeps its std in output 0 and the
    // mean of action k in output k + 1, mode 3 its stds in outputs A + k
    const float up = __shfl(out, min(lane + (la.act_mode == 2 ? 1 : A), 63), 64);
    const float std_o = la.act_mode == 2 ? clw_readlane(out, 0) : fabsf(up);
    a = la.act_mode == 2 ? up : out;
    if (mine && b < la.noiseless_from && std_o != 0.0f)
      a += std_o * es_actnoise(seed, (uint64_t)b * odim + lane);
    a = fclampf(a, -1.0f, 1.0f);
  } else if (la.bins > 1) {
    // per-dim argmax over `bins` lanes, the first maximum wins
    const int base = min(lane, A - 1) * la.bins;
    int best = 0;
    float bv = __shfl(out, base, 64);
    for (int j = 1; j < la.bins; ++j) {
      const float v = __shfl(out, base + j, 64);
      if (v > bv) { bv = v; best = j; }
    }
    a = -1.0f + 2.0f * (float)best / (float)(la.bins - 1);
  } else {
    a = out;
    if (mine && ac_std != 0.0f && b < la.noiseless_from)
      a += ac_std * es_actnoise(seed, (uint64_t)b * A + lane);
    a = fclampf(a, -1.0f, 1.0f);
  }
  return mine ? a : 0.0f;
}

template <typename WT>
__device__ __forceinline__ void loco_wave_episode_body(const LocoWaveArgs& W) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const MlpShape& sh = W.sh;
  const LocoArgs& la = W.la;
  const LocoPtrs& P = W.P;
  const int S = la.S, A = la.A, D = la.D;

  // ---- env block: staged by the whole block, read by each of its waves
  uint16_t* Am = reinterpret_cast<uint16_t*>(smem);
  float* Bm = reinterpret_cast<float*>(smem + loco_wave_a_bytes(S));
  float* b0 = Bm + A * S;
  float *wv = b0 + S, *wy = wv + S, *wh = wy + S, *wa = wh + S;
  float *obmean = wa + A, *obstd = obmean + D;
  {
    const int tid = threadIdx.x;
    for (int k = tid; k < S * S; k += 64 * WAVE_WAVES) Am[k] = P.Am[k];
    for (int k = tid; k < A * S; k += 64 * WAVE_WAVES) Bm[k] = P.Bm[k];
    if (tid < S) {
      b0[tid] = P.b0[tid];
      wv[tid] = P.wv[tid];
      wy[tid] = P.wy[tid];
      wh[tid] = P.wh[tid];
    }
    if (tid < A) wa[tid] = P.wa[tid];
    if (tid < D) {
      obmean[tid] = P.obmean[tid];
      obstd[tid] = P.obstd[tid];
    }
  }
  __syncthreads();
  // no block barrier from here on

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int rel = blockIdx.x * W.spb + wave;
  if (wave >= W.spb || rel >= W.n_members) return;
  const int b = W.member_base + rel;
  bool alive = __builtin_amdgcn_readfirstlane((int)(P.alive[b] > 0.0f)) != 0;
  if (!alive) return;  // a slot that enters dead keeps everything it owns

  WT* wl = reinterpret_cast<WT*>(smem + W.env_bytes + (size_t)wave * W.region_bytes);
  wave_row_to_lds(reinterpret_cast<const WT*>(P.weights) +
                      (int64_t)(b / la.eps - la.wrow0) * la.row_stride,
                  wl, W.n_params, lane);

  // ---- the slot, in registers
  const bool own_s = lane < S;                // lane i < S holds s[i]
  const bool own_g = la.goal && (lane == S || lane == S + 1);  // goal-relative dims
  const int ls = min(lane, S - 1), ld = min(lane, D - 1), lk = min(lane, A - 1);
  float s = own_s ? P.s_glob[(int64_t)b * S + lane] : 0.0f;
  LocoWaveSlot st;
  st.px = P.pos[(int64_t)b * 3 + 0];
  st.py = P.pos[(int64_t)b * 3 + 1];
  st.ph = 0.0f;
  st.gx = la.goal ? P.goal[(int64_t)b * 2 + 0] : 0.0f;
  st.gy = la.goal ? P.goal[(int64_t)b * 2 + 1] : 0.0f;
  st.rew_total = P.rew_total[b];
  st.member_steps = P.member_steps[b];
  float msum = P.mo_sum[(int64_t)b * D + ld], msq = P.mo_sumsq[(int64_t)b * D + ld];
  // this lane's own entries of the env vectors
  const float mean_l = obmean[ld], std_l = obstd[ld];
  const float b0_l = b0[ls];
  const float wv_l = own_s ? wv[ls] : 0.0f, wy_l = own_s ? wy[ls] : 0.0f,
              wh_l = own_s ? wh[ls] : 0.0f;
  const float wa_l = lane < A ? wa[lk] : 0.0f;

  const int odim = sh.dims[sh.n_layers];
  const uint64_t seed0 = P.seed_dev ? *P.seed_dev : 0;
  const float ac_std = P.ac_std_dev ? *P.ac_std_dev : 0.0f;
  // dynamics lane mapping: OP = the power of two >= S
  const int lg = S <= 1 ? 0 : 32 - __clz(S - 1);
  const int OP = 1 << lg;
  const int o = min(lane & (OP - 1), S - 1), p = lane >> lg;

  for (int t = 1; t <= W.n_steps && alive; ++t) {
    // observation: loco_build_obs's expression, division and clamp included
    float raw = s;
    if (own_g) raw = ((lane == S ? st.gx : st.gy) - (lane == S ? st.px : st.py)) * 0.1f;
    const float x = fclampf((raw - mean_l) / std_l, -la.ob_clip, la.ob_clip);
    const float out = wave_mlp_layers(wl, sh, x, lane, 1);
    const float a = loco_wave_decode(la, odim, b, seed0 + (uint64_t)(W.salt_base + t),
                                     ac_std, out, lane);
    // dynamics: pre[o] = b0[o] + sum_i s[i] A[i][o] + sum_k a[k] B[k][o]
    float acc = loco_wave_dot(Am, S, S, lg, o, p, s, 0.0f);
    acc = loco_wave_dot(Bm, A, S, lg, o, p, a, acc);
    for (int off = OP; off < 64; off <<= 1) acc += __shfl_xor(acc, off, 64);
    float sn = 0.0f, rel_l = 0.0f;
    {
#pragma clang fp contract(off)
      if (own_s) sn = (1.0f - la.leak) * s + la.leak * tanhf(b0_l + acc);
      s = sn;
      const float vfwd = loco_wave_sum(fmaf(0.5f * a, wa_l, sn * wv_l));
      const float vy = loco_wave_sum(sn * wy_l);
      const float h = loco_wave_sum(sn * wh_l);
      const float asq = loco_wave_sum(a * a);
      const bool done = loco_wave_book(la, st, vfwd, vy, h, asq);
      // the slot was alive before the step: its moments take the new
      // observation, goal-relative dims from the new position
      if (own_g) rel_l = ((lane == S ? st.gx : st.gy) - (lane == S ? st.px : st.py)) * 0.1f;
      const float ob_new = own_g ? rel_l : sn;
      msum += ob_new;
      msq += ob_new * ob_new;
      // every lane holds the same value; tell the compiler so
      alive = __builtin_amdgcn_readfirstlane((int)done) == 0;
    }
  }

  // ---- written once; behv is the position of the last step the slot took alive
  if (own_s) P.s_glob[(int64_t)b * S + lane] = s;
  if (lane < D) {
    P.mo_sum[(int64_t)b * D + lane] = msum;
    P.mo_sumsq[(int64_t)b * D + lane] = msq;
  }
  if (lane == 0) {
    P.pos[(int64_t)b * 3 + 0] = st.px;
    P.pos[(int64_t)b * 3 + 1] = st.py;
    P.pos[(int64_t)b * 3 + 2] = st.ph;
    P.behv[(int64_t)b * 3 + 0] = st.px;
    P.behv[(int64_t)b * 3 + 1] = st.py;
    P.behv[(int64_t)b * 3 + 2] = st.ph;
    P.rew_total[b] = st.rew_total;
    P.member_steps[b] = st.member_steps;
    P.alive[b] = alive ? 1.0f : 0.0f;
  }
}

// one template, named per weight type in the resource table and the profiles
template <typename WT>
__global__ void __launch_bounds__(256) CLW_KERNEL_ATTR
loco_wave_episode_kernel(LocoWaveArgs W) {
  loco_wave_episode_body<WT>(W);
}

// The coverage, the one place it is decided: 0 and the geometry of W, or -116.
static inline int loco_wave_geometry(const MlpShape& sh, int sdim, int adim, bool f32,
                                     LocoWaveArgs* W) {
  W->n_params = wave_row_elems(sh);
  if (W->n_params < 0) return W->n_params;
  if (sdim < 1 || sdim > WAVE_MAXW || adim < 1 || adim > WAVE_MAXW) return -116;
  W->region_bytes = wave_row_bytes(W->n_params, f32);
  W->env_bytes = loco_wave_a_bytes(sdim) +
                 ((loco_wave_env_floats(sdim, adim, sh.dims[0]) * 4 + 15) & ~15);
  W->spb = wave_regions_per_block(W->region_bytes, W->env_bytes);
  return W->spb < 0 ? W->spb : 0;
}

static int loco_wave_launch(bool f32, const LocoLaunch& L, int32_t n_steps,
                            int32_t member_base, int32_t n_members, int32_t salt_base,
                            int32_t wrow0, void* stream) {
  LocoWaveArgs W;
  W.sh = L.sh; W.la = L.la; W.P = L.P;
  W.la.wrow0 = wrow0;
  const int rc = loco_wave_geometry(W.sh, W.la.S, W.la.A, f32, &W);
  if (rc) return rc;
  if (n_steps <= 0 || n_members <= 0) return 0;
  W.member_base = member_base; W.n_members = n_members;
  W.n_steps = n_steps; W.salt_base = salt_base;
  const dim3 grid((unsigned)((n_members + W.spb - 1) / W.spb)), block(64 * WAVE_WAVES);
  const unsigned lds = (unsigned)(W.env_bytes + W.spb * W.region_bytes);
  if (f32)
    loco_wave_episode_kernel<float><<<grid, block, lds, (hipStream_t)stream>>>(W);
  else
    loco_wave_episode_kernel<uint16_t><<<grid, block, lds, (hipStream_t)stream>>>(W);
  ES_CHECK_LAUNCH();
  return 0;
}

// What a launch with this net and env would return for the shapes alone (0,
// one of mlp_shape_init's codes, -103, -104 or -116), without launching.
extern "C" int es_loco_wave_check(const int32_t* dims_host, int32_t ndims,
                                  int64_t row_stride, int32_t sdim, int32_t adim,
                                  int32_t goal_flag, int32_t f32) {
  MlpShape sh;
  int rc = mlp_shape_init(&sh, dims_host, ndims, row_stride);
  if (rc) return rc;
  if (adim > 64 || sdim > ES_MAXDIM) return -103;
  if (sh.dims[0] != sdim + (goal_flag ? 2 : 0)) return -104;
  LocoWaveArgs W;
  return loco_wave_geometry(sh, sdim, adim, f32 != 0, &W);
}

// es_loco_episode's argument list without block_threads; member_base,
// n_members, salt_base, wrow0, eps and noiseless_from mean what they mean
// there. n_steps <= 0 or n_members <= 0 is a no-op returning 0.
#define LOCO_WAVE_ENTRY(NAME, F32)                                                        \
  extern "C" int NAME(                                                                    \
      const void* weights, const void* obmean, const void* obstd,                         \
      const int32_t* dims_host, int32_t ndims, const void* seed_dev, int32_t n_steps,     \
      float ob_clip, const void* ac_std_dev, int64_t row_stride, void* s_glob, void* pos, \
      const void* goal, const void* Am, const void* Bm, const void* b0, const void* wv,   \
      const void* wa, const void* wy, const void* wh, void* alive, void* rew_total,       \
      void* member_steps, void* behv, void* mo_sum, void* mo_sumsq, int32_t member_base,  \
      int32_t n_members, int32_t salt_base, int32_t wrow0, int32_t sdim, int32_t adim,    \
      int32_t goal_flag, int32_t terminate, int32_t noiseless_from, int32_t bins,         \
      int32_t eps, int32_t act_mode, float leak, float ctrl, float alive_bonus,           \
      float fall_thr, float dt, void* stream) {                                           \
    LocoLaunch L;                                                                         \
    int rc = loco_setup(&L, weights, obmean, obstd, dims_host, ndims, seed_dev, ob_clip,  \
                        ac_std_dev, row_stride, s_glob, pos, goal, Am, Bm, b0, wv, wa,    \
                        wy, wh, alive, rew_total, member_steps, behv, mo_sum, mo_sumsq,   \
                        sdim, adim, goal_flag, terminate, noiseless_from, bins, eps,      \
                        act_mode, leak, ctrl, alive_bonus, fall_thr, dt);                 \
    return rc ? rc                                                                        \
              : loco_wave_launch(F32, L, n_steps, member_base, n_members, salt_base,      \
                                 wrow0, stream);                                          \
  }

LOCO_WAVE_ENTRY(es_loco_wave_episode, false)
LOCO_WAVE_ENTRY(es_loco_wave_episode_f32, true)
