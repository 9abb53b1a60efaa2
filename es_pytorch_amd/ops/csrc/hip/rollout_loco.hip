// Fused rollout kernels for the synthetic locomotion envs.
//
// Per population member (one workgroup), one env step comprises:
//   policy MLP forward (mlp_core.h scheme, bf16 weight streaming)
//   + gaussian action noise or K9 binned decode (skipped / noise-free for
//     the noiseless evaluation, reference es.py:48 passes rs=None)
//   + env dynamics  s' = (1-leak) s + leak tanh(s A + a B + b0)
//   + reward / positions / fall-termination (envs/locomotion.py semantics)
//   + alive-masked bookkeeping: total reward, per-member steps, behaviour
//     freeze, per-member observation sums for ObStat
//
// Two launch shapes share the body:
//  * es_loco_step    — ONE step for a whole population (grid = pop). The
//    engine replays max_steps of these from a hipGraph. Replaced ~25 small
//    torch kernels + a forward launch per step (measured ~470 us/step).
//  * es_loco_episode — a WHOLE episode for a few members (internal step
//    loop). Used for the noiseless evaluation on a side stream so the main
//    per-step grid stays an exact multiple of the CU slot count (a +1
//    straggler block measured ~15-20% tail on every step).
#include "mlp_core.h"

struct LocoArgs {
  int S;               // latent state dim
  int A;               // action dim
  int D;               // obs dim (= S, or S+2 goal-conditioned)
  int goal;            // goal-conditioned flag
  int terminate;       // terminate_on_fall
  int noiseless_from;  // members >= this index get no action noise
  int bins;            // >1: K9 binned-action decode (FFBinned)
  int act_mode;        // 0 plain, 1 binned, 2 integ-gauss, 3 integ-gauss-multi
  int eps;             // episodes per perturbation: slot b uses weights row b/eps
  int wrow0;           // weights-row index of slot 0 (episode kernel on a
                       // sub-blob, e.g. the pair path's 1-row theta blob)
  float leak, ctrl, alive_bonus, fall_thr, dt, ob_clip;
  int64_t row_stride;
};

struct LocoPtrs {
  const uint16_t* weights;
  const float *obmean, *obstd, *ac_std_dev;
  const uint64_t* seed_dev;
  float *s_glob, *pos;
  const float *goal, *Bm, *b0, *wv, *wa, *wy, *wh;
  const uint16_t* Am;  // bf16 state-transition matrix (S, S)
  float *alive, *rew_total, *member_steps, *behv, *mo_sum, *mo_sumsq;
};

// ---- build normalized obs for slot b; keep raw state in LDS --------------
__device__ __forceinline__ void loco_build_obs(
    const LocoArgs& la, const LocoPtrs& P, int b, float* bufA, float* raws,
    int tid, int nth) {
  const int S = la.S;
  const float* sb = P.s_glob + (int64_t)b * S;
  for (int i = tid; i < S; i += nth) {
    const float v = sb[i];
    raws[i] = v;
    bufA[i] = fclampf((v - P.obmean[i]) / P.obstd[i], -la.ob_clip, la.ob_clip);
  }
  if (la.goal && tid < 2) {
    const float rel = (P.goal[(int64_t)b * 2 + tid] - P.pos[(int64_t)b * 3 + tid]) * 0.1f;
    bufA[S + tid] = fclampf((rel - P.obmean[S + tid]) / P.obstd[S + tid], -la.ob_clip,
                            la.ob_clip);
  }
}

// LDS copies of operands that cannot change during a launch (the multi-step
// fp8 pair kernel's STAGE levels): the step reads them here instead of taking
// a global round trip behind a barrier. Laid out after the pair carve in this
// order; `bias`, `ht`, `he` are mlp_layers_pair_fp8's stage.
struct LocoStage {
  const float *obmean, *obstd;     // D each
  const float *b0, *wv, *wy, *wh;  // S each
  const float* wa;                 // A
  const float* bias;
  const uint16_t* ht;
  const uint8_t* he;
  bool head;  // the last layer's weights are staged (level 2, scalar head)
};

// One obs pass for both members of a pair: obmean/obstd are loaded once and
// both members' state loads issue together. Same per-member arithmetic as
// loco_build_obs, division included. STAGE: obmean/obstd come from G.
template <int STAGE = 0>
__device__ __forceinline__ void loco_build_obs_pair(
    const LocoArgs& la, const LocoPtrs& P, int bp, int bm, float* bufAp, float* bufAm,
    float* rawsP, float* rawsM, int tid, int nth, const LocoStage& G = LocoStage{}) {
  const int S = la.S;
  const float* sp = P.s_glob + (int64_t)bp * S;
  const float* sm = P.s_glob + (int64_t)bm * S;
  const float* obmean;
  const float* obstd;
  if constexpr (STAGE >= 1) { obmean = G.obmean; obstd = G.obstd; }
  else { obmean = P.obmean; obstd = P.obstd; }
  for (int i = tid; i < S; i += nth) {
    const float vp = sp[i], vm = sm[i];
    const float mean = obmean[i], sd = obstd[i];
    rawsP[i] = vp;
    rawsM[i] = vm;
    bufAp[i] = fclampf((vp - mean) / sd, -la.ob_clip, la.ob_clip);
    bufAm[i] = fclampf((vm - mean) / sd, -la.ob_clip, la.ob_clip);
  }
  if (la.goal && tid < 2) {
    const float relp = (P.goal[(int64_t)bp * 2 + tid] - P.pos[(int64_t)bp * 3 + tid]) * 0.1f;
    const float relm = (P.goal[(int64_t)bm * 2 + tid] - P.pos[(int64_t)bm * 3 + tid]) * 0.1f;
    const float mean = obmean[S + tid], sd = obstd[S + tid];
    bufAp[S + tid] = fclampf((relp - mean) / sd, -la.ob_clip, la.ob_clip);
    bufAm[S + tid] = fclampf((relm - mean) / sd, -la.ob_clip, la.ob_clip);
  }
}

// ---- net output -> clamped env action for slot b (modes 0/1/2/3) ---------
__device__ __forceinline__ void loco_decode_action(
    const MlpShape& sh, const LocoArgs& la, const LocoPtrs& P, int b, uint64_t salt,
    const float* aout, float* abuf, int tid) {
  const int A = la.A;
  const uint64_t seed = P.seed_dev ? (*P.seed_dev + salt) : salt;
  const float ac_std = P.ac_std_dev ? *P.ac_std_dev : 0.0f;
  if (la.act_mode == 2 || la.act_mode == 3) {
    // integrated gaussian actions (reference nn.py:53-96)
    const int odim = sh.dims[sh.n_layers];
    if (tid < A) {
      float a = la.act_mode == 2 ? aout[1 + tid] : aout[tid];
      const float std_o = la.act_mode == 2 ? aout[0] : fabsf(aout[A + tid]);
      if (b < la.noiseless_from && std_o != 0.0f)
        a += std_o * es_actnoise(seed, (uint64_t)b * odim + tid);
      abuf[tid] = fclampf(a, -1.0f, 1.0f);
    }
  } else if (la.bins > 1) {
    // K9 binned decode (FFBinned): per-dim argmax over bins -> [-1, 1]
    if (tid < A) {
      const float* row = aout + tid * la.bins;
      int best = 0;
      float bv = row[0];
      for (int j = 1; j < la.bins; ++j)
        if (row[j] > bv) { bv = row[j]; best = j; }
      abuf[tid] = -1.0f + 2.0f * (float)best / (float)(la.bins - 1);
    }
  } else if (tid < A) {
    float a = aout[tid];
    if (ac_std != 0.0f && b < la.noiseless_from)
      a += ac_std * es_actnoise(seed, (uint64_t)b * A + tid);
    abuf[tid] = fclampf(a, -1.0f, 1.0f);  // env action clamp (locomotion.py)
  }
}

// WT = uint16_t: P.weights is the bf16 member blob (mlp_layers); WT = float:
// the same pointer holds float32 rows (weights_dtype = "fp32",
// mlp_layers_f32). row_stride counts elements of WT either way.
template <typename WT = uint16_t>
__device__ __forceinline__ void loco_fwd_body(
    const MlpShape& sh, const LocoArgs& la, const LocoPtrs& P, int b, uint64_t salt,
    float* bufA, float* bufB, float* partial, float* raws, float* abuf) {
  const int tid = threadIdx.x;
  const int nth = blockDim.x;
  loco_build_obs(la, P, b, bufA, raws, tid, nth);
  __syncthreads();
  const WT* wb = reinterpret_cast<const WT*>(P.weights) +
                 (int64_t)(b / la.eps - la.wrow0) * la.row_stride;
  const float* aout;
  if constexpr (sizeof(WT) == 4)
    aout = mlp_layers_f32(wb, sh, bufA, bufB, partial, tid, nth, 1);
  else
    aout = mlp_layers(wb, sh, bufA, bufB, partial, tid, nth, 1);
  loco_decode_action(sh, la, P, b, salt, aout, abuf, tid);
  __syncthreads();
}

// A-matvec partial sums for ONE member (bf16 A, octet-tiled like the policy
// layers in mlp_core.h; S % 8 == 0 required). Writes the (PART, OCT, 8)
// partial layout consumed by loco_dyn_finish's output sweep.
__device__ __forceinline__ void loco_dyn_partials(
    const uint16_t* Am, int S, const float* raws, float* partial, int tid, int nth) {
  const int OCT = S >> 3;
  const int PART = nth / OCT;
  const int oi = tid % OCT, ip = tid / OCT;
  float acc[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) acc[q] = 0.0f;
  if (ip < PART) {
    const uint16_t* acol = Am + (oi << 3);
    auto ld = [&](int i) {
      return *reinterpret_cast<const uint4*>(acol + (int64_t)i * S);
    };
    int i = ip;
    const int step4 = PART * 4;
    // 8-deep lookahead on the shared-A L2 stream (12 uint4 live instead of
    // the 8 of a depth-4 walk; measured -4.3% us/step on the fp8 flagship
    // when the pair kernels got it). Accumulation order stays ascending i.
    // Written out here and in loco_dyn_partials_pair<false>, not shared like
    // es_walk_ring4: with the FMA behind a lambda loco_step_kernel goes from
    // 91 to 107 VGPRs (5 -> 4 waves).
    if (i + 7 * PART < S) {
      uint4 c0 = ld(i), c1 = ld(i + PART), c2 = ld(i + 2 * PART), c3 = ld(i + 3 * PART);
      uint4 d0 = ld(i + 4 * PART), d1 = ld(i + 5 * PART), d2 = ld(i + 6 * PART),
            d3 = ld(i + 7 * PART);
      for (; i + 11 * PART < S; i += step4) {
        const uint4 n0 = ld(i + 8 * PART), n1 = ld(i + 9 * PART),
                    n2 = ld(i + 10 * PART), n3 = ld(i + 11 * PART);
        bf8_fma(c0, raws[i], acc);
        bf8_fma(c1, raws[i + PART], acc);
        bf8_fma(c2, raws[i + 2 * PART], acc);
        bf8_fma(c3, raws[i + 3 * PART], acc);
        c0 = d0; c1 = d1; c2 = d2; c3 = d3;
        d0 = n0; d1 = n1; d2 = n2; d3 = n3;
      }
      if (i < S) bf8_fma(c0, raws[i], acc);
      if (i + PART < S) bf8_fma(c1, raws[i + PART], acc);
      if (i + 2 * PART < S) bf8_fma(c2, raws[i + 2 * PART], acc);
      if (i + 3 * PART < S) bf8_fma(c3, raws[i + 3 * PART], acc);
      if (i + 4 * PART < S) bf8_fma(d0, raws[i + 4 * PART], acc);
      if (i + 5 * PART < S) bf8_fma(d1, raws[i + 5 * PART], acc);
      if (i + 6 * PART < S) bf8_fma(d2, raws[i + 6 * PART], acc);
      if (i + 7 * PART < S) bf8_fma(d3, raws[i + 7 * PART], acc);
      i += 8 * PART;
    }
    for (; i < S; i += PART) bf8_fma(ld(i), raws[i], acc);
#pragma unroll
    for (int q = 0; q < 8; ++q) partial[(ip * OCT + oi) * 8 + q] = acc[q];
  }
  __syncthreads();
}

// ES_DYN_BM_BT: action-term batch depth. The B column of an output is loaded
// ES_DYN_BM_BT rows at a time into registers before the ordered fmaf chain
// consumes them (all of it up front when A <= 16; Humanoid's A = 17 takes
// two batches instead of five serialized L2 round trips per output).
#define ES_DYN_BM_BT 16

// Scalars a member's bookkeeping lane needs. Their addresses depend on no
// computed value, so the lane loads them BEFORE the output sweep instead of
// on demand in the serial section while the rest of the block waits.
struct LocoBook {
  float px, py, gx, gy, rew_total, member_steps, ms0, ms1, mq0, mq1;
};

// Dynamics output sweep + fused epilogue for NM members in ONE pass. The
// sweep that materializes s' also accumulates the reward/behaviour reduction
// partials AND the per-member obs statistics (one s'-sweep instead of three,
// and wave shuffles replace the 8-barrier LDS reduction tree). b0, the B
// column and wv/wy/wh of an output are loaded once for all members; the
// members share one shuffle reduction and one pair of barriers, and member
// m's scalar bookkeeping runs in lane 0 of wave m, concurrently (needs
// nth >= 64 * NM). Per-member arithmetic and summation order are those of a
// one-member call, so NM only changes when loads issue and how often waves
// wait. When S % 8 == 0 the A-matvec partials must already be in part[m]
// (loco_dyn_partials*); otherwise the scalar fallback reads Am directly.
//
// CARRY (multi-step kernels): when `carry` is set (block-uniform; requires
// S % 8 == 0, where raws[m][o] is read by its own thread only) the thread
// that owns output o also leaves s' in raws[m][o] and the next step's
// normalized observation in obs[m][o] — loco_build_obs_pair's expression,
// division included — and member m's bookkeeping lane writes the goal dims
// from the position it just computed. The caller's next step then skips the
// s_glob reload and the obs pass. s_glob is still written every step.
// Measured 0.1-0.5 us per step SLOWER than the reload at the flagship shape
// (profiles/README.md, round 6), so es_loco_pair_episode_fp8 has it off by
// default.
//
// STAGE (never with CARRY): b0, wv, wy, wh and wa come from the LDS copies
// in G instead of global memory.
template <int NM, bool CARRY = false, int STAGE = 0>
__device__ __forceinline__ void loco_dyn_finish_n(
    const LocoArgs& la, const LocoPtrs& P, const int* b, const float* const* raws,
    const float* const* abuf, float* const* part, int tid, int nth,
    float* const* obs = nullptr, bool carry = false,
    const LocoStage& G = LocoStage{}) {
  static_assert(!(CARRY && STAGE), "the staged levels do not carry");
  const int S = la.S, A = la.A;
  const float *b0v, *wvv, *wyv, *whv, *wav;
  if constexpr (STAGE >= 1) {
    b0v = G.b0; wvv = G.wv; wyv = G.wy; whv = G.wh; wav = G.wa;
  } else {
    b0v = P.b0; wvv = P.wv; wyv = P.wy; whv = P.wh; wav = P.wa;
  }
  float w_alive[NM];  // pre-step alive, used as obstat weight
  float *sb[NM], *ms[NM], *mq[NM];
#pragma unroll
  for (int m = 0; m < NM; ++m) {
    w_alive[m] = P.alive[b[m]];
    sb[m] = P.s_glob + (int64_t)b[m] * S;
    ms[m] = P.mo_sum + (int64_t)b[m] * la.D;
    mq[m] = P.mo_sumsq + (int64_t)b[m] * la.D;
  }
  // bookkeeping lane of member m: lane 0 of wave m
  const int wid = tid >> 6;
  const bool book = (tid & 63) == 0 && wid < NM;
  int bme = b[0];
  float alive_me = w_alive[0];
  float *part_me = part[0], *ms_me = ms[0], *mq_me = mq[0];
#pragma unroll
  for (int m = 1; m < NM; ++m)
    if (wid == m) {
      bme = b[m]; alive_me = w_alive[m];
      part_me = part[m]; ms_me = ms[m]; mq_me = mq[m];
    }
  LocoBook bk = {};
  if (book) {
    bk.px = P.pos[(int64_t)bme * 3 + 0];
    bk.py = P.pos[(int64_t)bme * 3 + 1];
    bk.rew_total = P.rew_total[bme];
    bk.member_steps = P.member_steps[bme];
    if (la.goal) {
      bk.gx = P.goal[(int64_t)bme * 2 + 0];
      bk.gy = P.goal[(int64_t)bme * 2 + 1];
      if (alive_me > 0.0f) {
        bk.ms0 = ms_me[S]; bk.ms1 = ms_me[S + 1];
        bk.mq0 = mq_me[S]; bk.mq1 = mq_me[S + 1];
      }
    }
  }
  // carried goal dims: normalization constants load with the lane's scalars
  float* obs_me = nullptr;
  float gmean0 = 0.0f, gmean1 = 0.0f, gsd0 = 1.0f, gsd1 = 1.0f;
  if constexpr (CARRY) {
    if (carry && la.goal && book) {
      obs_me = obs[0];
#pragma unroll
      for (int m = 1; m < NM; ++m)
        if (wid == m) obs_me = obs[m];
      gmean0 = P.obmean[S]; gmean1 = P.obmean[S + 1];
      gsd0 = P.obstd[S]; gsd1 = P.obstd[S + 1];
    }
  }

  float p0[NM], p1[NM], p2[NM], p3[NM];
#pragma unroll
  for (int m = 0; m < NM; ++m) p0[m] = p1[m] = p2[m] = p3[m] = 0.0f;
  {
    const bool oct8 = (S % 8 == 0);
    const int OCT = S >> 3;
    const int PART = oct8 ? nth / OCT : 0;
    for (int o = tid; o < S; o += nth) {
      // every load of this output whose address is known up front
      const float b0o = b0v[o], wvo = wvv[o], wyo = wyv[o], who = whv[o];
      float omean = 0.0f, osd = 1.0f;
      if constexpr (CARRY)
        if (carry) { omean = P.obmean[o]; osd = P.obstd[o]; }
      float mso[NM], mqo[NM];
#pragma unroll
      for (int m = 0; m < NM; ++m)
        if (w_alive[m] > 0.0f) {
          mso[m] = ms[m][o];
          mqo[m] = mq[m][o];
        }
      float p[NM];
#pragma unroll
      for (int m = 0; m < NM; ++m) p[m] = b0o;
      if (oct8) {
        const int oo = o >> 3, j = o & 7;
        for (int pp = 0; pp < PART; ++pp)
#pragma unroll
          for (int m = 0; m < NM; ++m) p[m] += part[m][(pp * OCT + oo) * 8 + j];
      } else {
        for (int i = 0; i < S; ++i) {
          const float a = bf2f(P.Am[(int64_t)i * S + o]);
#pragma unroll
          for (int m = 0; m < NM; ++m) p[m] = fmaf(raws[m][i], a, p[m]);
        }
      }
      // action term: batched B-column loads, ordered fmaf chain
      const float* bcol = P.Bm + o;
      int k0 = 0;
      for (; k0 + ES_DYN_BM_BT <= A; k0 += ES_DYN_BM_BT) {
        float bv[ES_DYN_BM_BT];
#pragma unroll
        for (int u = 0; u < ES_DYN_BM_BT; ++u) bv[u] = bcol[(int64_t)(k0 + u) * S];
#pragma unroll
        for (int u = 0; u < ES_DYN_BM_BT; ++u)
#pragma unroll
          for (int m = 0; m < NM; ++m) p[m] = fmaf(abuf[m][k0 + u], bv[u], p[m]);
      }
      if (k0 < A) {  // guarded drain (A is block-uniform)
        float bv[ES_DYN_BM_BT];
#pragma unroll
        for (int u = 0; u < ES_DYN_BM_BT - 1; ++u)
          if (k0 + u < A) bv[u] = bcol[(int64_t)(k0 + u) * S];
#pragma unroll
        for (int u = 0; u < ES_DYN_BM_BT - 1; ++u)
          if (k0 + u < A) {
#pragma unroll
            for (int m = 0; m < NM; ++m) p[m] = fmaf(abuf[m][k0 + u], bv[u], p[m]);
          }
      }
#pragma unroll
      for (int m = 0; m < NM; ++m) {
        const float sn = (1.0f - la.leak) * raws[m][o] + la.leak * tanhf(p[m]);
        sb[m][o] = sn;
        if constexpr (CARRY)
          if (carry) {
            const_cast<float*>(raws[m])[o] = sn;
            obs[m][o] = fclampf((sn - omean) / osd, -la.ob_clip, la.ob_clip);
          }
        p0[m] = fmaf(sn, wvo, p0[m]);
        p1[m] = fmaf(sn, wyo, p1[m]);
        p2[m] = fmaf(sn, who, p2[m]);
        if (w_alive[m] > 0.0f) {
          ms[m][o] = mso[m] + sn;
          mq[m][o] = mqo[m] + sn * sn;
        }
      }
    }
    for (int j = tid; j < A; j += nth) {
      const float waj = wav[j];
#pragma unroll
      for (int m = 0; m < NM; ++m) {
        p0[m] = fmaf(0.5f * abuf[m][j], waj, p0[m]);
        p3[m] = fmaf(abuf[m][j], abuf[m][j], p3[m]);
      }
    }
  }
  // wave-level shuffle reduction, then one cross-wave pass through LDS
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      p0[m] += __shfl_down(p0[m], off);
      p1[m] += __shfl_down(p1[m], off);
      p2[m] += __shfl_down(p2[m], off);
      p3[m] += __shfl_down(p3[m], off);
    }
  }
  __syncthreads();  // part[] reuse after the dynamics matvec
  if ((tid & 63) == 0) {
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      part[m][wid * 4 + 0] = p0[m];
      part[m][wid * 4 + 1] = p1[m];
      part[m][wid * 4 + 2] = p2[m];
      part[m][wid * 4 + 3] = p3[m];
    }
  }
  __syncthreads();

  // ---- scalar bookkeeping (lane 0 of wave m for member m) ----------------
  if (book) {
    const int nw = nth >> 6;
    float vfwd = 0, vy = 0, h = 0, asq = 0;
    for (int wdx = 0; wdx < nw; ++wdx) {
      vfwd += part_me[wdx * 4 + 0];
      vy += part_me[wdx * 4 + 1];
      h += part_me[wdx * 4 + 2];
      asq += part_me[wdx * 4 + 3];
    }
    const float alive_old = alive_me;
    float rew;
    if (la.goal) {
      const float rx = bk.gx - bk.px;
      const float ry = bk.gy - bk.py;
      const float inv = 1.0f / (sqrtf(rx * rx + ry * ry) + 1e-6f);
      rew = vfwd * rx * inv + vy * ry * inv - la.ctrl * asq + la.alive_bonus;
    } else {
      rew = vfwd - la.ctrl * asq + la.alive_bonus;
    }
    const float px = bk.px + la.dt * vfwd;
    const float py = bk.py + la.dt * vy;
    P.pos[(int64_t)bme * 3 + 0] = px;
    P.pos[(int64_t)bme * 3 + 1] = py;
    P.pos[(int64_t)bme * 3 + 2] = h;
    const float done = (la.terminate && h < la.fall_thr) ? 1.0f : 0.0f;
    P.rew_total[bme] = bk.rew_total + rew * alive_old;
    P.member_steps[bme] = bk.member_steps + alive_old;
    if (alive_old > 0.0f) {
      P.behv[(int64_t)bme * 3 + 0] = px;
      P.behv[(int64_t)bme * 3 + 1] = py;
      P.behv[(int64_t)bme * 3 + 2] = h;
    }
    P.alive[bme] = alive_old * (1.0f - done);
    // goal-relative obs dims of the per-member obs statistics (new pos)
    if (la.goal && alive_old > 0.0f) {
      const float rel0 = (bk.gx - px) * 0.1f;
      const float rel1 = (bk.gy - py) * 0.1f;
      ms_me[S] = bk.ms0 + rel0;
      mq_me[S] = bk.mq0 + rel0 * rel0;
      ms_me[S + 1] = bk.ms1 + rel1;
      mq_me[S + 1] = bk.mq1 + rel1 * rel1;
    }
    if constexpr (CARRY) {
      // goal-relative obs dims of the next step, from the position stored
      // above (loco_build_obs_pair's expression on the same float values)
      if (carry && la.goal) {
        const float rel0 = (bk.gx - px) * 0.1f;
        const float rel1 = (bk.gy - py) * 0.1f;
        obs_me[S] = fclampf((rel0 - gmean0) / gsd0, -la.ob_clip, la.ob_clip);
        obs_me[S + 1] = fclampf((rel1 - gmean1) / gsd1, -la.ob_clip, la.ob_clip);
      }
    }
  }
  // next step of an episode kernel: alive/pos written above are read by
  // other threads, and raws/part are rewritten
  __syncthreads();
}

__device__ __forceinline__ void loco_dyn_finish(
    const LocoArgs& la, const LocoPtrs& P, int b, const float* raws,
    const float* abuf, float* partial, int tid, int nth) {
  const int bs[1] = {b};
  const float* const rs[1] = {raws};
  const float* const as[1] = {abuf};
  float* const ps[1] = {partial};
  loco_dyn_finish_n<1>(la, P, bs, rs, as, ps, tid, nth);
}

// One fused epilogue for both members of a pair.
template <bool CARRY = false, int STAGE = 0>
__device__ __forceinline__ void loco_dyn_finish_pair(
    const LocoArgs& la, const LocoPtrs& P, int bp, int bm, const float* rawsP,
    const float* rawsM, const float* abufP, const float* abufM, float* partP,
    float* partM, int tid, int nth, float* obsP = nullptr, float* obsM = nullptr,
    bool carry = false, const LocoStage& G = LocoStage{}) {
  const int bs[2] = {bp, bm};
  const float* const rs[2] = {rawsP, rawsM};
  const float* const as[2] = {abufP, abufM};
  float* const ps[2] = {partP, partM};
  float* const os[2] = {obsP, obsM};
  loco_dyn_finish_n<2, CARRY, STAGE>(la, P, bs, rs, as, ps, tid, nth, os, carry, G);
}

template <typename WT = uint16_t>
__device__ __forceinline__ void loco_step_body(
    const MlpShape& sh, const LocoArgs& la, const LocoPtrs& P, int b, uint64_t salt,
    float* bufA, float* bufB, float* partial, float* raws, float* abuf) {
  loco_fwd_body<WT>(sh, la, P, b, salt, bufA, bufB, partial, raws, abuf);
  if (la.S % 8 == 0)
    loco_dyn_partials(P.Am, la.S, raws, partial, threadIdx.x, blockDim.x);
  loco_dyn_finish(la, P, b, raws, abuf, partial, threadIdx.x, blockDim.x);
}

// NTH = block size: the partial slab is NTH * 8 floats
#define ES_LOCO_CARVE(NTH)                                       \
  extern __shared__ __attribute__((aligned(16))) char smem[];    \
  float* bufA = reinterpret_cast<float*>(smem);                  \
  float* bufB = bufA + sh.maxdim;                                \
  float* partial = bufB + sh.maxdim;                             \
  float* raws = partial + (NTH) * 8;                             \
  float* abuf = raws + ((la.S + 3) & ~3);

__global__ void __launch_bounds__(256)
loco_step_kernel(MlpShape sh, LocoArgs la, LocoPtrs P, uint64_t salt) {
  ES_LOCO_CARVE(256);
  loco_step_body(sh, la, P, blockIdx.x, salt, bufA, bufB, partial, raws, abuf);
}

__global__ void __launch_bounds__(256)
loco_episode_kernel(MlpShape sh, LocoArgs la, LocoPtrs P, int member_base, int n_steps,
                    int salt_base) {
  ES_LOCO_CARVE(256);
  const int b = member_base + blockIdx.x;
  for (int t = 1; t <= n_steps; ++t)
    loco_step_body(sh, la, P, b, (uint64_t)(salt_base + t), bufA, bufB, partial, raws,
                   abuf);
}

// 512-thread variant for the LATENCY-BOUND noiseless side episode: one
// block runs max_steps sequential steps, so halving every per-step
// partition (PART doubles) shortens the serial dependency chains. Used
// only for the noiseless member (block_threads=512) — the episode-mode
// population grid keeps 256-thread blocks for occupancy.
__global__ void __launch_bounds__(512)
loco_episode512_kernel(MlpShape sh, LocoArgs la, LocoPtrs P, int member_base,
                       int n_steps, int salt_base) {
  ES_LOCO_CARVE(512);
  const int b = member_base + blockIdx.x;
  for (int t = 1; t <= n_steps; ++t)
    loco_step_body(sh, la, P, b, (uint64_t)(salt_base + t), bufA, bufB, partial, raws,
                   abuf);
}

// ---- fp32-weights variants (weights_dtype = "fp32") ------------------------
// The step and episode kernels above with the fp32 forward (mlp_layers_f32);
// obs build, action decode, dynamics, epilogue and bookkeeping are the same
// device functions, and A stays the env's bf16-valued matrix. Same LDS
// carve: the quad partials need PART * O <= nthreads * 4 floats, or O <=
// ES_MAXDIM = 256 * 8 floats when a layer is wider than 4 * nthreads.
__global__ void __launch_bounds__(256)
loco_step_f32_kernel(MlpShape sh, LocoArgs la, LocoPtrs P, uint64_t salt) {
  ES_LOCO_CARVE(256);
  loco_step_body<float>(sh, la, P, blockIdx.x, salt, bufA, bufB, partial, raws, abuf);
}

__global__ void __launch_bounds__(256)
loco_episode_f32_kernel(MlpShape sh, LocoArgs la, LocoPtrs P, int member_base,
                        int n_steps, int salt_base) {
  ES_LOCO_CARVE(256);
  const int b = member_base + blockIdx.x;
  for (int t = 1; t <= n_steps; ++t)
    loco_step_body<float>(sh, la, P, b, (uint64_t)(salt_base + t), bufA, bufB, partial,
                          raws, abuf);
}

__global__ void __launch_bounds__(512)
loco_episode512_f32_kernel(MlpShape sh, LocoArgs la, LocoPtrs P, int member_base,
                           int n_steps, int salt_base) {
  ES_LOCO_CARVE(512);
  const int b = member_base + blockIdx.x;
  for (int t = 1; t <= n_steps; ++t)
    loco_step_body<float>(sh, la, P, b, (uint64_t)(salt_base + t), bufA, bufB, partial,
                          raws, abuf);
}

// ---- split-dynamics path ---------------------------------------------------
// The fused kernel re-reads the shared (S, S) bf16 transition matrix A once
// per MEMBER (pop x 283 KB per step for Humanoid = the measured ~20 us/step
// L2-bandwidth bound, profiles/README.md). The split path factors one env
// step into two launches:
//   loco_fwd_kernel  — grid = pop: obs build + policy forward + action
//                      decode, actions written to a (pop, 64) global scratch;
//   loco_dyn_kernel<G> — grid = pop/G: each block stages G members' states
//                      and actions in LDS and FMAs every A octet it loads
//                      into all G members' accumulators, cutting A traffic
//                      G-fold. Per-member accumulation order is IDENTICAL to
//                      the fused kernel (same (oi, ip) tiling, same depth-4
//                      pipeline, same loco_dyn_finish), so split and fused
//                      trajectories match bitwise.
__global__ void __launch_bounds__(256)
loco_fwd_kernel(MlpShape sh, LocoArgs la, LocoPtrs P, uint64_t salt, float* act_glob) {
  ES_LOCO_CARVE(256);
  const int b = blockIdx.x;
  loco_fwd_body(sh, la, P, b, salt, bufA, bufB, partial, raws, abuf);
  if (threadIdx.x < la.A) act_glob[(int64_t)b * 64 + threadIdx.x] = abuf[threadIdx.x];
}

template <int G>
__global__ void __launch_bounds__(256)
loco_dyn_kernel(LocoArgs la, LocoPtrs P, const float* act_glob, int n_pop) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int S = la.S;
  const int Spad = (S + 3) & ~3;
  float* raws = reinterpret_cast<float*>(smem);  // G x Spad raw states
  float* abuf = raws + G * Spad;                 // G x 64 actions
  float* partial = abuf + G * 64;                // G x 2048 matvec partials
  const int tid = threadIdx.x, nth = blockDim.x;
  const int b0 = blockIdx.x * G;
  const int gs = min(G, n_pop - b0);  // members in this block (tail block < G)

  // stage states + actions; zero-fill tail slots so the accumulator loop can
  // stay fully unrolled with compile-time member indices (register arrays)
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const float* sb = P.s_glob + (int64_t)(b0 + g) * S;
    for (int i = tid; i < S; i += nth) raws[g * Spad + i] = g < gs ? sb[i] : 0.0f;
    if (tid < la.A)
      abuf[g * 64 + tid] = g < gs ? act_glob[(int64_t)(b0 + g) * 64 + tid] : 0.0f;
  }
  __syncthreads();

  // shared-A sweep: one uint4 A-octet load feeds G members' bf8_fma chains
  const int OCT = S >> 3;
  const int PART = nth / OCT;
  const int oi = tid % OCT, ip = tid / OCT;
  if (ip < PART) {
    float acc[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[g][q] = 0.0f;
    const uint16_t* acol = P.Am + (oi << 3);
    auto ld = [&](int i) {
      return *reinterpret_cast<const uint4*>(acol + (int64_t)i * S);
    };
    auto fmaG = [&](const uint4& c, int i) {
#pragma unroll
      for (int g = 0; g < G; ++g) bf8_fma(c, raws[g * Spad + i], acc[g]);
    };
    es_walk_ring4(ip, PART, S, ld, fmaG);
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int q = 0; q < 8; ++q)
        partial[g * 2048 + (ip * OCT + oi) * 8 + q] = acc[g][q];
  }
  __syncthreads();

  for (int g = 0; g < gs; ++g)
    loco_dyn_finish(la, P, b0 + g, raws + g * Spad, abuf + g * 64,
                    partial + g * 2048, tid, nth);
}

template <int G>
static int loco_launch_dyn(const LocoArgs& la, const LocoPtrs& P, const float* act_glob,
                           int n_pop, hipStream_t stream) {
  const int Spad = (la.S + 3) & ~3;
  const unsigned lds = (unsigned)((G * Spad + G * 64 + G * 2048) * sizeof(float));
  const unsigned grid = (unsigned)((n_pop + G - 1) / G);
  loco_dyn_kernel<G><<<dim3(grid), dim3(256), lds, stream>>>(la, P, act_glob, n_pop);
  ES_CHECK_LAUNCH();
  return 0;
}

// ---- antithetic-pair rollout step ------------------------------------------
// One block per (pair, episode): the +noise and -noise members' forwards run
// together off ONE HBM sigma*eps stream plus the L2-resident shared theta
// stream (mlp_layers_pair, mlp_core.h) — the per-step HBM weight traffic
// halves vs materialized per-member blobs. Dynamics shares each A octet
// between the two members; the epilogue is the two-member instance of the
// fused step's (loco_dyn_finish_n), same per-member arithmetic and order, so
// per-slot bookkeeping is identical to the fused step.
// Effective weights are bf16(theta) +- bf16(sigma*eps) (two roundings); with
// sigma = 0 the trajectories are BITWISE-identical to es_loco_step.

// A-matvec partial sums for both members of a pair off one A stream. PIPE =
// true streams A through the set ring; PIPE = false keeps the 8-deep
// copy-rotated walk of loco_dyn_partials: the whole-episode kernel runs under
// a 128-VGPR bound with spills, and the set ring adds to them.
template <bool PIPE = true>
__device__ __forceinline__ void loco_dyn_partials_pair(
    const uint16_t* Am, int S, const float* rawsP, const float* rawsM,
    float* partP, float* partM, int tid, int nth) {
  const int OCT = S >> 3;
  const int PART = nth / OCT;
  const int oi = tid % OCT, ip = tid / OCT;
  float accp[8], accm[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) accp[q] = accm[q] = 0.0f;
  if (ip < PART) {
    const uint16_t* acol = Am + (oi << 3);
    auto ld = [&](int i) {
      return *reinterpret_cast<const uint4*>(acol + (int64_t)i * S);
    };
    auto fma2 = [&](const uint4& c, int i) {
      bf8_fma(c, rawsP[i], accp);
      bf8_fma(c, rawsM[i], accm);
    };
    int i = ip;
    if constexpr (PIPE) {
      // Set ring (design note at the ring in mlp_layers_pair_fp8,
      // mlp_core.h): three 4-row sets that change role by name over a steady
      // loop of whole turns; each sub-trip fills the free set 8 rows ahead,
      // then consumes the oldest, so a load is first waited for two
      // sub-trips after it issues. Every lane owns nmin or nmin + 1 rows;
      // the turn count is block-uniform, and the 0..12 rows a lane has left
      // behind the two held sets load ahead of the drain.
      const int nmin = S / PART;
      if (nmin >= 8) {
        const int T = (nmin - 8) / 12;
        const int rem = (S - 1 - ip) / PART + 1 - 12 * T - 8;
        EsRowStream as(Am, ip, PART, 2 * S, oi << 4);
        const float* xP = rawsP + ip;
        const float* xM = rawsM + ip;
        es_f32x2 a2p[4], a2m[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) a2p[q] = a2m[q] = es_f32x2{0.0f, 0.0f};
        struct Set { es_u32x4 v[4]; };
        auto fill = [&](Set& s) {
#pragma unroll
          for (int k = 0; k < 4; ++k) s.v[k] = as.ld(k);
          as.advance(4);
        };
        auto eat = [&](const Set& s) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            bf8_fma_pk(s.v[k], xP[k * PART], a2p);
            bf8_fma_pk(s.v[k], xM[k * PART], a2m);
          }
          xP += 4 * PART;
          xM += 4 * PART;
        };
        Set c, d, n;
        fill(c);
        fill(d);
        // the fences keep a sub-trip's work out of the next one, where the
        // set it reads is refilled
        for (int t = T; t > 0; --t) {
          fill(n); eat(c);
          __builtin_amdgcn_sched_barrier(0);
          fill(c); eat(d);
          __builtin_amdgcn_sched_barrier(0);
          fill(d); eat(n);
          __builtin_amdgcn_sched_barrier(0);
        }
        // drain: the rows left load into fresh names (merging with a set's
        // stale rows would copy them), then c, d and they are consumed
        es_u32x4 f[12];
#pragma unroll
        for (int k = 0; k < 12; ++k)
          if (k < rem) f[k] = as.ld(k);
        __builtin_amdgcn_sched_barrier(0);
        eat(c);
        __builtin_amdgcn_sched_barrier(0);
        eat(d);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < 12; ++k) {
          if (k < rem) {
            bf8_fma_pk(f[k], xP[k * PART], a2p);
            bf8_fma_pk(f[k], xM[k * PART], a2m);
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          accp[2 * q] = a2p[q].x; accp[2 * q + 1] = a2p[q].y;
          accm[2 * q] = a2m[q].x; accm[2 * q + 1] = a2m[q].y;
        }
        i = S;  // every owned row is consumed
      }
    } else {
      const int step4 = PART * 4;
      if (i + 7 * PART < S) {
        uint4 c0 = ld(i), c1 = ld(i + PART), c2 = ld(i + 2 * PART), c3 = ld(i + 3 * PART);
        uint4 d0 = ld(i + 4 * PART), d1 = ld(i + 5 * PART), d2 = ld(i + 6 * PART),
              d3 = ld(i + 7 * PART);
        for (; i + 11 * PART < S; i += step4) {
          const uint4 n0 = ld(i + 8 * PART), n1 = ld(i + 9 * PART),
                      n2 = ld(i + 10 * PART), n3 = ld(i + 11 * PART);
          fma2(c0, i);
          fma2(c1, i + PART);
          fma2(c2, i + 2 * PART);
          fma2(c3, i + 3 * PART);
          c0 = d0; c1 = d1; c2 = d2; c3 = d3;
          d0 = n0; d1 = n1; d2 = n2; d3 = n3;
        }
        // drain the 8 preloaded blocks (guarded; order stays ascending)
        if (i < S) fma2(c0, i);
        if (i + PART < S) fma2(c1, i + PART);
        if (i + 2 * PART < S) fma2(c2, i + 2 * PART);
        if (i + 3 * PART < S) fma2(c3, i + 3 * PART);
        if (i + 4 * PART < S) fma2(d0, i + 4 * PART);
        if (i + 5 * PART < S) fma2(d1, i + 5 * PART);
        if (i + 6 * PART < S) fma2(d2, i + 6 * PART);
        if (i + 7 * PART < S) fma2(d3, i + 7 * PART);
        i += 8 * PART;
      }
    }
    for (; i < S; i += PART) fma2(ld(i), i);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      partP[(ip * OCT + oi) * 8 + q] = accp[q];
      partM[(ip * OCT + oi) * 8 + q] = accm[q];
    }
  }
  __syncthreads();
}

// EB = uint16_t (bf16 eps rows) or uint8_t (fp8 row-pair-interleaved rows).
// tid is the caller's threadIdx.x (the multi-step fp8 kernel hands in a copy
// the optimizer cannot see through). CARRY: `have` = the previous step of
// this launch left raws and the normalized obs in LDS, `keep` = this step
// leaves them for the next (loco_dyn_finish_n); both block-uniform.
template <typename EB, bool PIPE = true, bool CARRY = false, int STAGE = 0>
__device__ __forceinline__ void loco_pair_step_body(
    const MlpShape& sh, const LocoArgs& la, const LocoPtrs& P,
    const uint16_t* tb, const EB* eb, int bp, int bm, uint64_t salt,
    float* bufAp, float* bufAm, float* bufBp, float* bufBm, float* partial,
    float* rawsP, float* rawsM, float* abufP, float* abufM, int tid,
    bool have = false, bool keep = false, const LocoStage& G = LocoStage{}) {
  const int nth = blockDim.x;
  if (!(CARRY && have)) {
    loco_build_obs_pair<STAGE>(la, P, bp, bm, bufAp, bufAm, rawsP, rawsM, tid, nth, G);
    __syncthreads();
  }
  float *ap, *am;
  if constexpr (sizeof(EB) == 1)
    mlp_layers_pair_fp8<STAGE>(tb, (const uint8_t*)eb, sh, bufAp, bufAm, bufBp, bufBm,
                               partial, tid, nth, 1, &ap, &am, G.bias, G.ht, G.he,
                               G.head);
  else
    mlp_layers_pair(tb, (const uint16_t*)eb, sh, bufAp, bufAm, bufBp, bufBm,
                    partial, tid, nth, 1, &ap, &am);
  loco_decode_action(sh, la, P, bp, salt, ap, abufP, tid);
  loco_decode_action(sh, la, P, bm, salt, am, abufM, tid);
  __syncthreads();
  if (la.S % 8 == 0)
    loco_dyn_partials_pair<PIPE>(P.Am, la.S, rawsP, rawsM, partial, partial + 2048,
                                 tid, nth);
  loco_dyn_finish_pair<CARRY, STAGE>(la, P, bp, bm, rawsP, rawsM, abufP, abufM,
                                     partial, partial + 2048, tid, nth, bufAp, bufAm,
                                     keep, G);
}

#define ES_LOCO_PAIR_CARVE()                                     \
  extern __shared__ __attribute__((aligned(16))) char smem[];    \
  float* bufAp = reinterpret_cast<float*>(smem);                 \
  float* bufAm = bufAp + sh.maxdim;                              \
  float* bufBp = bufAm + sh.maxdim;                              \
  float* bufBm = bufBp + sh.maxdim;                              \
  float* partial = bufBm + sh.maxdim; /* 2 x 256*8 */            \
  float* rawsP = partial + 2 * 256 * 8;                          \
  float* rawsM = rawsP + ((la.S + 3) & ~3);                      \
  float* abufP = rawsM + ((la.S + 3) & ~3);                      \
  float* abufM = abufP + 64;                                     \
  const int q = blockIdx.x;                                      \
  const int p = q / la.eps, e = q % la.eps;                      \
  const int bp = p * la.eps + e;                                 \
  const int bm = (n_pairs + p) * la.eps + e;                     \
  const auto* ebp = eb + (int64_t)p * la.row_stride;

__global__ void __launch_bounds__(256, 1)
loco_pair_step_kernel(MlpShape sh, LocoArgs la, LocoPtrs P, const uint16_t* tb,
                      const uint16_t* eb, int n_pairs, uint64_t salt) {
  ES_LOCO_PAIR_CARVE();
  loco_pair_step_body(sh, la, P, tb, ebp, bp, bm, salt, bufAp, bufAm, bufBp, bufBm,
                      partial, rawsP, rawsM, abufP, abufM, threadIdx.x);
}

__global__ void __launch_bounds__(256, 1)
loco_pair_step_fp8_kernel(MlpShape sh, LocoArgs la, LocoPtrs P, const uint16_t* tb,
                          const uint8_t* eb, int n_pairs, uint64_t salt) {
  ES_LOCO_PAIR_CARVE();
  loco_pair_step_body(sh, la, P, tb, ebp, bp, bm, salt, bufAp, bufAm, bufBp, bufBm,
                      partial, rawsP, rawsM, abufP, abufM, threadIdx.x);
}

// Whole-episode (or k-step chunk) pair rollout in ONE launch: each block
// owns its (pair, episode) slot for n_steps consecutive env steps. Unlike
// the per-step launch, blocks never rendezvous chip-wide, so one block's
// L2-side dynamics phase overlaps other blocks' HBM sigma*eps streaming
// (the per-step grid runs phase-locked: every block starts its forward at
// launch, leaving HBM idle during the correlated dynamics phases — measured
// 47% HBM duty at the flagship config). Trajectories are bitwise-identical
// to n_steps sequential es_loco_pair_step launches (same salt_base + t
// sequence, same body).
// unroll(disable): the step loop's only carried state is scalar, but an
// unrolled body doubles the live vector ranges (256 VGPRs = 2 blocks/CU,
// or 328 B/lane spills under a 3-wave bound). Episode mode REQUIRES
// >= 3 blocks/CU: 640 flagship blocks must all be resident, since blocks
// retire only at episode end.
__global__ void __launch_bounds__(256, 4)
loco_pair_episode_kernel(MlpShape sh, LocoArgs la, LocoPtrs P, const uint16_t* tb,
                         const uint16_t* eb, int n_pairs, int n_steps,
                         int salt_base) {
  ES_LOCO_PAIR_CARVE();
#pragma clang loop unroll(disable)
  for (int t = 1; t <= n_steps; ++t)
    loco_pair_step_body<uint16_t, false>(sh, la, P, tb, ebp, bp, bm, (uint64_t)(salt_base + t),
                        bufAp, bufAm, bufBp, bufBm, partial, rawsP, rawsM, abufP,
                        abufM, threadIdx.x);
}

// The fp8 sibling: the set-ring body (PIPE = true) in a step loop. Left to
// itself the optimizer hoists every per-lane address and every load that does
// not change from step to step out of the loop and holds them across it
// (naive loop under a 4-wave bound: 64 VGPRs spilled, 292 B/lane scratch).
// So once per step the kernel passes its loop-invariant inputs — every
// pointer, the slot indices and the thread index — through an empty asm the
// optimizer cannot see through: a few scalar moves per step, and the body
// compiles as it does in the per-step kernel. MINB = blocks per CU the
// register budget is sized for (4: 128 VGPRs, 3: 134-138); none of the
// instantiations spills or uses scratch. CARRY keeps the state and the next
// observation in LDS between the steps of a launch (loco_dyn_finish_n); it
// falls back to the reload when S % 8 != 0.
#define ES_OPAQUE_S(x) asm volatile("" : "+s"(x))
#define ES_OPAQUE_V(x) asm volatile("" : "+v"(x))
// A pointer that crosses the asm as a pointer comes back generic: its loads
// become flat_*, which count on vmcnt and lgkmcnt both, so every wait drains
// the whole queue (vmcnt(0)) and the set rings are gone. It crosses as an
// integer instead and is cast to the global address space on the way back;
// null stays null.
template <typename T>
__device__ __forceinline__ T* es_opaque_global(T* p) {
  unsigned long long v = (unsigned long long)p;
  ES_OPAQUE_S(v);
  return (T*)(__attribute__((address_space(1))) T*)v;
}
#define ES_OPAQUE_G(x) ((x) = es_opaque_global(x))

// STAGE (with CARRY = false): what a block reads every step but nothing
// writes during a launch is copied to LDS once, behind the pair carve, and
// read there (LocoStage). 1: obmean, obstd, b0, wv, wy, wh, wa and the layer
// biases; 2: also the last layer's weights when it is on the scalar path.
// The launcher adds loco_stage_lds_bytes() and only picks a level at which
// the whole grid is resident.
static int64_t loco_stage_floats(const MlpShape& sh, const LocoArgs& la) {
  return 2 * (int64_t)la.D + 4 * (int64_t)la.S + la.A + mlp_pair_fp8_bias_floats(sh);
}
static unsigned loco_stage_lds_bytes(const MlpShape& sh, const LocoArgs& la, int level) {
  if (level < 1) return 0;
  int64_t n = 4 * loco_stage_floats(sh, la);
  if (level >= 2) n += 3 * mlp_pair_fp8_head_elems(sh);  // bf16 theta + fp8 eps
  return (unsigned)((n + 15) & ~(int64_t)15);
}

template <int MINB, bool CARRY, int STAGE = 0>
__global__ void __launch_bounds__(256, MINB)
loco_pair_chunk_fp8_kernel(MlpShape sh, LocoArgs la, LocoPtrs Pk, const uint16_t* tb,
                           const uint8_t* eb, int n_pairs, int n_steps, int salt_base) {
  ES_LOCO_PAIR_CARVE();
  LocoPtrs P = Pk;
  int bpl = bp, bml = bm;
  int tid = threadIdx.x;
  const bool oct8 = (la.S % 8 == 0);
  LocoStage G = {};
  if constexpr (STAGE >= 1) {
    float* g = abufM + 64;  // end of the pair carve
    float* gmean = g;
    float* gstd = gmean + la.D;
    float* gb0 = gstd + la.D;
    float* gwv = gb0 + la.S;
    float* gwy = gwv + la.S;
    float* gwh = gwy + la.S;
    float* gwa = gwh + la.S;
    float* gbias = gwa + la.A;
    int nb = 0;
    for (int l = 0; l < sh.n_layers; ++l) nb += 2 * sh.dims[l + 1];
    const int hl = sh.n_layers - 1;
    uint16_t* ght = reinterpret_cast<uint16_t*>(gbias + nb);
    uint8_t* ghe = reinterpret_cast<uint8_t*>(ght + sh.dims[hl] * sh.dims[hl + 1]);
    const bool head = STAGE >= 2 && !sh.vec_ok[hl];
    for (int i = tid; i < la.D; i += 256) {
      gmean[i] = Pk.obmean[i];
      gstd[i] = Pk.obstd[i];
    }
    for (int i = tid; i < la.S; i += 256) {
      gb0[i] = Pk.b0[i];
      gwv[i] = Pk.wv[i];
      gwy[i] = Pk.wy[i];
      gwh[i] = Pk.wh[i];
    }
    for (int i = tid; i < la.A; i += 256) gwa[i] = Pk.wa[i];
    mlp_pair_fp8_stage_fill(tb, ebp, sh, gbias, ght, ghe, head, tid, 256);
    __syncthreads();
    G = LocoStage{gmean, gstd, gb0, gwv, gwy, gwh, gwa, gbias, ght, ghe, head};
  }
#pragma clang loop unroll(disable)
  for (int t = 1; t <= n_steps; ++t) {
    ES_OPAQUE_G(P.weights); ES_OPAQUE_G(P.obmean); ES_OPAQUE_G(P.obstd);
    ES_OPAQUE_G(P.ac_std_dev); ES_OPAQUE_G(P.seed_dev); ES_OPAQUE_G(P.s_glob);
    ES_OPAQUE_G(P.pos); ES_OPAQUE_G(P.goal); ES_OPAQUE_G(P.Bm); ES_OPAQUE_G(P.b0);
    ES_OPAQUE_G(P.wv); ES_OPAQUE_G(P.wa); ES_OPAQUE_G(P.wy); ES_OPAQUE_G(P.wh);
    ES_OPAQUE_G(P.Am); ES_OPAQUE_G(P.alive); ES_OPAQUE_G(P.rew_total);
    ES_OPAQUE_G(P.member_steps); ES_OPAQUE_G(P.behv); ES_OPAQUE_G(P.mo_sum);
    ES_OPAQUE_G(P.mo_sumsq); ES_OPAQUE_G(tb); ES_OPAQUE_G(ebp);
    ES_OPAQUE_S(bpl); ES_OPAQUE_S(bml);
    ES_OPAQUE_V(tid);
    // 1 - leak and -ob_clip are otherwise computed once and held in VGPRs
    // (the last 4 spilled registers of the 4-block variant). Laundering the
    // LDS pointers or the integer members of `la` as well brings spills back.
    ES_OPAQUE_S(la.leak); ES_OPAQUE_S(la.ob_clip);
    loco_pair_step_body<uint8_t, true, CARRY, STAGE>(
        sh, la, P, tb, ebp, bpl, bml, (uint64_t)(salt_base + t), bufAp, bufAm, bufBp,
        bufBm, partial, rawsP, rawsM, abufP, abufM, tid, oct8 && t > 1,
        oct8 && t < n_steps, G);
  }
}

// (A 128-thread 2-waves/SIMD variant — zero spills, 4 blocks/CU — was
// measured 24% SLOWER than per-step launches and cannot match them bitwise
// (different PART split changes summation order); removed after the A/B.)

// ---- host side --------------------------------------------------------------
// Every entry point is loco_setup (validate, build the kernel arguments) and
// then its group's launcher. Arguments are bound by position in
// ops/__init__.py; loco_setup takes the ones all entry points share, in the
// order they appear there.
struct LocoLaunch {
  MlpShape sh;
  LocoArgs la;
  LocoPtrs P;
};

static int loco_setup(LocoLaunch* L, const void* weights, const void* obmean,
                      const void* obstd, const int32_t* dims_host, int32_t ndims,
                      const void* seed_dev, float ob_clip, const void* ac_std_dev,
                      int64_t row_stride, void* s_glob, void* pos, const void* goal,
                      const void* Am, const void* Bm, const void* b0, const void* wv,
                      const void* wa, const void* wy, const void* wh, void* alive,
                      void* rew_total, void* member_steps, void* behv, void* mo_sum,
                      void* mo_sumsq, int32_t sdim, int32_t adim, int32_t goal_flag,
                      int32_t terminate, int32_t noiseless_from, int32_t bins,
                      int32_t eps, int32_t act_mode, float leak, float ctrl,
                      float alive_bonus, float fall_thr, float dt) {
  MlpShape* sh = &L->sh;
  int rc = mlp_shape_init(sh, dims_host, ndims, row_stride);
  if (rc) return rc;
  if (adim > 64 || sdim > ES_MAXDIM) return -103;
  if (sh->dims[0] != sdim + (goal_flag ? 2 : 0)) return -104;
  int out_dim = adim;
  if (bins > 1) out_dim = adim * bins;
  else if (act_mode == 2) out_dim = adim + 1;
  else if (act_mode == 3) out_dim = adim * 2;
  if (sh->dims[sh->n_layers] != out_dim) return -105;
  LocoArgs* la = &L->la;
  la->S = sdim; la->A = adim; la->D = sh->dims[0]; la->goal = goal_flag;
  la->terminate = terminate; la->noiseless_from = noiseless_from; la->bins = bins;
  la->act_mode = act_mode;
  la->eps = eps > 0 ? eps : 1;
  la->wrow0 = 0;
  la->leak = leak; la->ctrl = ctrl; la->alive_bonus = alive_bonus; la->fall_thr = fall_thr;
  la->dt = dt; la->ob_clip = ob_clip; la->row_stride = row_stride;
  LocoPtrs* P = &L->P;
  P->weights = (const uint16_t*)weights;
  P->obmean = (const float*)obmean; P->obstd = (const float*)obstd;
  P->ac_std_dev = (const float*)ac_std_dev; P->seed_dev = (const uint64_t*)seed_dev;
  P->s_glob = (float*)s_glob; P->pos = (float*)pos; P->goal = (const float*)goal;
  P->Am = (const uint16_t*)Am; P->Bm = (const float*)Bm; P->b0 = (const float*)b0;
  P->wv = (const float*)wv; P->wa = (const float*)wa; P->wy = (const float*)wy;
  P->wh = (const float*)wh; P->alive = (float*)alive; P->rew_total = (float*)rew_total;
  P->member_steps = (float*)member_steps; P->behv = (float*)behv;
  P->mo_sum = (float*)mo_sum; P->mo_sumsq = (float*)mo_sumsq;
  return 0;
}

// dynamic LDS of the one-member kernels at 256 threads
static unsigned loco_lds_bytes(const LocoLaunch& L) {
  return (unsigned)(mlp_lds_bytes(L.sh.maxdim) + (((L.la.S + 3) & ~3) + 64 + 8) * 4);
}

// es_loco_step / es_loco_step_f32: WT = uint16_t (bf16 blob) or float
template <typename WT>
static int loco_launch_step(LocoLaunch& L, int32_t n_pop, uint64_t salt, void* stream) {
  constexpr bool f32 = sizeof(WT) == 4;
  if (f32) mlp_shape_vec_f32(&L.sh, L.la.row_stride);
  auto* kern = f32 ? loco_step_f32_kernel : loco_step_kernel;
  kern<<<dim3((unsigned)n_pop), dim3(256), loco_lds_bytes(L), (hipStream_t)stream>>>(
      L.sh, L.la, L.P, salt);
  ES_CHECK_LAUNCH();
  return 0;
}

// es_loco_episode / es_loco_episode_f32
template <typename WT>
static int loco_launch_episode(LocoLaunch& L, int32_t n_steps, int32_t member_base,
                               int32_t n_members, int32_t salt_base, int32_t wrow0,
                               int32_t block_threads, void* stream) {
  constexpr bool f32 = sizeof(WT) == 4;
  if (f32) mlp_shape_vec_f32(&L.sh, L.la.row_stride);
  L.la.wrow0 = wrow0;
  const bool wide = block_threads == 512;
  auto* kern = wide ? (f32 ? loco_episode512_f32_kernel : loco_episode512_kernel)
                    : (f32 ? loco_episode_f32_kernel : loco_episode_kernel);
  // partial[] grows with the block size
  const unsigned lds = loco_lds_bytes(L) + (wide ? 256 * 8 * 4 : 0);
  kern<<<dim3((unsigned)n_members), dim3(wide ? 512 : 256), lds, (hipStream_t)stream>>>(
      L.sh, L.la, L.P, member_base, n_steps, salt_base);
  ES_CHECK_LAUNCH();
  return 0;
}

// The three pair entry points: `kern` is the step kernel (tail = salt), its
// fp8 sibling or the episode kernel (tail = n_steps, salt_base); EB is the
// element type of its eps rows. Grid = n_pairs * eps blocks, each evaluating
// the +/- slots of one (pair, episode).
// `lds` = dynamic LDS bytes: the pair carve, plus the stage of the multi-step
// fp8 kernel's staged levels.
template <typename EB, typename... Tail>
static int loco_launch_pair_lds(void (*kern)(MlpShape, LocoArgs, LocoPtrs,
                                             const uint16_t*, const EB*, int, Tail...),
                                const LocoLaunch& L, const void* theta_row,
                                const void* eps_rows, int32_t n_pairs, void* stream,
                                unsigned lds, Tail... tail) {
  const unsigned grid = (unsigned)(n_pairs * L.la.eps);
  kern<<<dim3(grid), dim3(256), lds, (hipStream_t)stream>>>(
      L.sh, L.la, L.P, (const uint16_t*)theta_row, (const EB*)eps_rows, n_pairs, tail...);
  ES_CHECK_LAUNCH();
  return 0;
}

template <typename EB, typename... Tail>
static int loco_launch_pair(void (*kern)(MlpShape, LocoArgs, LocoPtrs, const uint16_t*,
                                         const EB*, int, Tail...),
                            const LocoLaunch& L, const void* theta_row,
                            const void* eps_rows, int32_t n_pairs, void* stream,
                            Tail... tail) {
  return loco_launch_pair_lds(kern, L, theta_row, eps_rows, n_pairs, stream,
                              (unsigned)mlp_pair_lds_bytes(L.sh.maxdim, L.la.S), tail...);
}

extern "C" int es_loco_step(const void* weights, const void* obmean, const void* obstd,
                            const int32_t* dims_host, int32_t ndims, const void* seed_dev,
                            uint64_t salt, float ob_clip, const void* ac_std_dev,
                            int64_t row_stride,
                            void* s_glob, void* pos, const void* goal, const void* Am,
                            const void* Bm, const void* b0, const void* wv, const void* wa,
                            const void* wy, const void* wh, void* alive, void* rew_total,
                            void* member_steps, void* behv, void* mo_sum, void* mo_sumsq,
                            int32_t n_pop, int32_t sdim, int32_t adim, int32_t goal_flag,
                            int32_t terminate, int32_t noiseless_from, int32_t bins,
                            int32_t eps, int32_t act_mode, float leak, float ctrl,
                            float alive_bonus, float fall_thr, float dt, void* stream) {
  LocoLaunch L;
  int rc = loco_setup(&L, weights, obmean, obstd, dims_host, ndims, seed_dev, ob_clip,
                      ac_std_dev, row_stride, s_glob, pos, goal, Am, Bm, b0, wv, wa, wy,
                      wh, alive, rew_total, member_steps, behv, mo_sum, mo_sumsq, sdim,
                      adim, goal_flag, terminate, noiseless_from, bins, eps, act_mode,
                      leak, ctrl, alive_bonus, fall_thr, dt);
  return rc ? rc : loco_launch_step<uint16_t>(L, n_pop, salt, stream);
}

// Split-dynamics step: forward kernel (grid = pop) then shared-A dynamics
// kernel (grid = pop/G). act_glob = (n_pop, 64) float32 scratch. Requires
// S % 8 == 0 (octet A tiling) and G in {2, 4, 5, 8}. Bitwise-identical
// trajectories to es_loco_step (tests/test_gpu_kernels.py).
extern "C" int es_loco_step_split(
    const void* weights, const void* obmean, const void* obstd,
    const int32_t* dims_host, int32_t ndims, const void* seed_dev, uint64_t salt,
    float ob_clip, const void* ac_std_dev, int64_t row_stride, void* s_glob, void* pos,
    const void* goal, const void* Am, const void* Bm, const void* b0, const void* wv,
    const void* wa, const void* wy, const void* wh, void* alive, void* rew_total,
    void* member_steps, void* behv, void* mo_sum, void* mo_sumsq, int32_t n_pop,
    int32_t sdim, int32_t adim, int32_t goal_flag, int32_t terminate,
    int32_t noiseless_from, int32_t bins, int32_t eps, int32_t act_mode, float leak,
    float ctrl, float alive_bonus, float fall_thr, float dt, void* act_glob, int32_t G,
    void* stream) {
  LocoLaunch L;
  int rc = loco_setup(&L, weights, obmean, obstd, dims_host, ndims, seed_dev, ob_clip,
                      ac_std_dev, row_stride, s_glob, pos, goal, Am, Bm, b0, wv, wa, wy,
                      wh, alive, rew_total, member_steps, behv, mo_sum, mo_sumsq, sdim,
                      adim, goal_flag, terminate, noiseless_from, bins, eps, act_mode,
                      leak, ctrl, alive_bonus, fall_thr, dt);
  if (rc) return rc;
  if (sdim % 8 != 0) return -106;
  hipStream_t s = (hipStream_t)stream;
  loco_fwd_kernel<<<dim3((unsigned)n_pop), dim3(256), loco_lds_bytes(L), s>>>(
      L.sh, L.la, L.P, salt, (float*)act_glob);
  ES_CHECK_LAUNCH();
  switch (G) {
    case 2: return loco_launch_dyn<2>(L.la, L.P, (const float*)act_glob, n_pop, s);
    case 4: return loco_launch_dyn<4>(L.la, L.P, (const float*)act_glob, n_pop, s);
    case 5: return loco_launch_dyn<5>(L.la, L.P, (const float*)act_glob, n_pop, s);
    case 8: return loco_launch_dyn<8>(L.la, L.P, (const float*)act_glob, n_pop, s);
    default: return -107;
  }
}

// Antithetic-pair step: theta_row = (1, row_stride) bf16(theta);
// eps_rows = (n_pairs, row_stride) bf16(sigma*eps).
extern "C" int es_loco_pair_step(
    const void* theta_row, const void* eps_rows, const void* obmean,
    const void* obstd, const int32_t* dims_host, int32_t ndims, const void* seed_dev,
    uint64_t salt, float ob_clip, const void* ac_std_dev, int64_t row_stride,
    void* s_glob, void* pos, const void* goal, const void* Am, const void* Bm,
    const void* b0, const void* wv, const void* wa, const void* wy, const void* wh,
    void* alive, void* rew_total, void* member_steps, void* behv, void* mo_sum,
    void* mo_sumsq, int32_t n_pairs, int32_t sdim, int32_t adim, int32_t goal_flag,
    int32_t terminate, int32_t noiseless_from, int32_t bins, int32_t eps,
    int32_t act_mode, float leak, float ctrl, float alive_bonus, float fall_thr,
    float dt, void* stream) {
  LocoLaunch L;
  int rc = loco_setup(&L, nullptr, obmean, obstd, dims_host, ndims, seed_dev, ob_clip,
                      ac_std_dev, row_stride, s_glob, pos, goal, Am, Bm, b0, wv, wa, wy,
                      wh, alive, rew_total, member_steps, behv, mo_sum, mo_sumsq, sdim,
                      adim, goal_flag, terminate, noiseless_from, bins, eps, act_mode,
                      leak, ctrl, alive_bonus, fall_thr, dt);
  return rc ? rc
            : loco_launch_pair(loco_pair_step_kernel, L, theta_row, eps_rows, n_pairs,
                               stream, salt);
}

// fp8-eps pair step: eps_rows = (n_pairs, row_stride) BYTES, written by
// es_pheno_fp8 (row-pair-interleaved e4m3); theta_row stays bf16.
extern "C" int es_loco_pair_step_fp8(
    const void* theta_row, const void* eps_rows, const void* obmean,
    const void* obstd, const int32_t* dims_host, int32_t ndims, const void* seed_dev,
    uint64_t salt, float ob_clip, const void* ac_std_dev, int64_t row_stride,
    void* s_glob, void* pos, const void* goal, const void* Am, const void* Bm,
    const void* b0, const void* wv, const void* wa, const void* wy, const void* wh,
    void* alive, void* rew_total, void* member_steps, void* behv, void* mo_sum,
    void* mo_sumsq, int32_t n_pairs, int32_t sdim, int32_t adim, int32_t goal_flag,
    int32_t terminate, int32_t noiseless_from, int32_t bins, int32_t eps,
    int32_t act_mode, float leak, float ctrl, float alive_bonus, float fall_thr,
    float dt, void* stream) {
  LocoLaunch L;
  int rc = loco_setup(&L, nullptr, obmean, obstd, dims_host, ndims, seed_dev, ob_clip,
                      ac_std_dev, row_stride, s_glob, pos, goal, Am, Bm, b0, wv, wa, wy,
                      wh, alive, rew_total, member_steps, behv, mo_sum, mo_sumsq, sdim,
                      adim, goal_flag, terminate, noiseless_from, bins, eps, act_mode,
                      leak, ctrl, alive_bonus, fall_thr, dt);
  return rc ? rc
            : loco_launch_pair(loco_pair_step_fp8_kernel, L, theta_row, eps_rows,
                               n_pairs, stream, salt);
}

// Pair-episode: n_steps consecutive env steps per launch (n_steps =
// max_steps -> whole generation in one launch; smaller -> chunked step
// mode). Same buffers as es_loco_pair_step.
extern "C" int es_loco_pair_episode(
    const void* theta_row, const void* eps_rows, const void* obmean,
    const void* obstd, const int32_t* dims_host, int32_t ndims, const void* seed_dev,
    float ob_clip, const void* ac_std_dev, int64_t row_stride,
    void* s_glob, void* pos, const void* goal, const void* Am, const void* Bm,
    const void* b0, const void* wv, const void* wa, const void* wy, const void* wh,
    void* alive, void* rew_total, void* member_steps, void* behv, void* mo_sum,
    void* mo_sumsq, int32_t n_pairs, int32_t sdim, int32_t adim, int32_t goal_flag,
    int32_t terminate, int32_t noiseless_from, int32_t bins, int32_t eps,
    int32_t act_mode, float leak, float ctrl, float alive_bonus, float fall_thr,
    float dt, int32_t n_steps, int32_t salt_base, void* stream) {
  LocoLaunch L;
  int rc = loco_setup(&L, nullptr, obmean, obstd, dims_host, ndims, seed_dev, ob_clip,
                      ac_std_dev, row_stride, s_glob, pos, goal, Am, Bm, b0, wv, wa, wy,
                      wh, alive, rew_total, member_steps, behv, mo_sum, mo_sumsq, sdim,
                      adim, goal_flag, terminate, noiseless_from, bins, eps, act_mode,
                      leak, ctrl, alive_bonus, fall_thr, dt);
  return rc ? rc
            : loco_launch_pair(loco_pair_episode_kernel, L, theta_row, eps_rows, n_pairs,
                               stream, n_steps, salt_base);
}

// Which loco_pair_chunk_fp8_kernel instantiation es_loco_pair_episode_fp8
// launches: blocks per CU the register budget is sized for (3 or 4) and
// whether the state is carried in LDS between the steps of a launch. A
// process-wide switch so that tools/kbench.py can A/B the four variants; the
// defaults are the round-6 sweep's choice (profiles/README.md).
#define ES_CHUNK_FP8_MIN_BLOCKS 4
#define ES_CHUNK_FP8_CARRY 0
static int g_chunk_fp8_min_blocks = ES_CHUNK_FP8_MIN_BLOCKS;
static int g_chunk_fp8_carry = ES_CHUNK_FP8_CARRY;
// STAGE level: -1 = automatic, the highest level up to g_chunk_fp8_stage_max
// at which every block of the grid is resident (blocks retire only at the end
// of the launch, and the stage costs LDS, hence blocks per CU); 0/1/2 force a
// level. CARRY builds have no staged form and run level 0. The automatic
// choice is capped at level 0: staging measured +2.0 % per flagship
// generation, every run ahead of every unstaged one, but short of the
// project's bar of three times the run-to-run spread (profiles/README.md,
// round 7). -DES_CHUNK_FP8_STAGE_MAX=2 builds a library that stages by default
// (tools/build_variants.py), es_loco_pair_episode_fp8_stage_max sets it at
// run time.
#ifndef ES_CHUNK_FP8_STAGE_MAX
#define ES_CHUNK_FP8_STAGE_MAX 0
#endif
static int g_chunk_fp8_stage = -1;
static int g_chunk_fp8_stage_max = ES_CHUNK_FP8_STAGE_MAX;

// min_blocks = 0 restores the defaults, the automatic stage level included.
extern "C" int es_loco_pair_episode_fp8_config(int32_t min_blocks, int32_t carry) {
  if (min_blocks == 0) {
    min_blocks = ES_CHUNK_FP8_MIN_BLOCKS;
    carry = ES_CHUNK_FP8_CARRY;
    g_chunk_fp8_stage = -1;
    g_chunk_fp8_stage_max = ES_CHUNK_FP8_STAGE_MAX;
  }
  if (min_blocks != 3 && min_blocks != 4) return -108;
  g_chunk_fp8_min_blocks = min_blocks;
  g_chunk_fp8_carry = carry != 0;
  return 0;
}

// level: -1 automatic (the default), 0/1/2 forced. A forced level at which
// the grid is not resident makes es_loco_pair_episode_fp8 return -110.
extern "C" int es_loco_pair_episode_fp8_stage(int32_t level) {
  if (level < -1 || level > 2) return -109;
  g_chunk_fp8_stage = level;
  return 0;
}

// highest level the automatic choice may take (0..2)
extern "C" int es_loco_pair_episode_fp8_stage_max(int32_t max_level) {
  if (max_level < 0 || max_level > 2) return -109;
  g_chunk_fp8_stage_max = max_level;
  return 0;
}

// the level es_loco_pair_episode_fp8 launched last (tests, tools/kbench.py)
static int g_chunk_fp8_last_stage = 0;
extern "C" int es_loco_pair_episode_fp8_last_stage() { return g_chunk_fp8_last_stage; }

typedef void (*ChunkFp8Kern)(MlpShape, LocoArgs, LocoPtrs, const uint16_t*,
                             const uint8_t*, int, int, int);
static ChunkFp8Kern chunk_fp8_kernel(bool four, bool carry, int stage) {
  if (carry)
    return four ? loco_pair_chunk_fp8_kernel<4, true> : loco_pair_chunk_fp8_kernel<3, true>;
  switch (stage) {
    case 2:
      // one build for both settings: under the 4-block budget level 2
      // spills (2 VGPRs, 12 B per lane of scratch); at the flagship shape its
      // LDS holds 3 blocks per CU in any case
      return loco_pair_chunk_fp8_kernel<3, false, 2>;
    case 1:
      return four ? loco_pair_chunk_fp8_kernel<4, false, 1>
                  : loco_pair_chunk_fp8_kernel<3, false, 1>;
    default:
      return four ? loco_pair_chunk_fp8_kernel<4, false>
                  : loco_pair_chunk_fp8_kernel<3, false>;
  }
}

// Blocks of `kern` (256 threads, `lds` dynamic bytes) the current device
// holds at once: the occupancy query times the CU count, 0 where it cannot
// launch at all. Remembered per (kernel, lds, device): the engine asks the
// same question every launch.
static int64_t chunk_fp8_resident(ChunkFp8Kern kern, unsigned lds) {
  struct Memo { ChunkFp8Kern kern; unsigned lds; int dev; int64_t n; };
  static Memo memo[8];
  static int n_memo = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  for (int i = 0; i < n_memo; ++i)
    if (memo[i].kern == kern && memo[i].lds == lds && memo[i].dev == dev) return memo[i].n;
  int cus = 0, per_cu = 0;
  int64_t n = 0;
  if (lds <= 64 * 1024 &&
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, lds) == hipSuccess)
    n = (int64_t)per_cu * cus;
  else
    (void)hipGetLastError();
  static int next = 0;
  memo[next] = Memo{kern, lds, dev, n};
  next = (next + 1) % 8;
  if (n_memo < 8) ++n_memo;
  return n;
}

// fp8-eps pair-episode: the argument list of es_loco_pair_episode; eps_rows
// as for es_loco_pair_step_fp8. Step i of the launch draws its action noise
// with salt_base + i, i = 1..n_steps.
extern "C" int es_loco_pair_episode_fp8(
    const void* theta_row, const void* eps_rows, const void* obmean,
    const void* obstd, const int32_t* dims_host, int32_t ndims, const void* seed_dev,
    float ob_clip, const void* ac_std_dev, int64_t row_stride,
    void* s_glob, void* pos, const void* goal, const void* Am, const void* Bm,
    const void* b0, const void* wv, const void* wa, const void* wy, const void* wh,
    void* alive, void* rew_total, void* member_steps, void* behv, void* mo_sum,
    void* mo_sumsq, int32_t n_pairs, int32_t sdim, int32_t adim, int32_t goal_flag,
    int32_t terminate, int32_t noiseless_from, int32_t bins, int32_t eps,
    int32_t act_mode, float leak, float ctrl, float alive_bonus, float fall_thr,
    float dt, int32_t n_steps, int32_t salt_base, void* stream) {
  LocoLaunch L;
  int rc = loco_setup(&L, nullptr, obmean, obstd, dims_host, ndims, seed_dev, ob_clip,
                      ac_std_dev, row_stride, s_glob, pos, goal, Am, Bm, b0, wv, wa, wy,
                      wh, alive, rew_total, member_steps, behv, mo_sum, mo_sumsq, sdim,
                      adim, goal_flag, terminate, noiseless_from, bins, eps, act_mode,
                      leak, ctrl, alive_bonus, fall_thr, dt);
  if (rc) return rc;
  const bool four = g_chunk_fp8_min_blocks == 4, carry = g_chunk_fp8_carry != 0;
  const int64_t grid = (int64_t)n_pairs * L.la.eps;
  const unsigned lds0 = (unsigned)mlp_pair_lds_bytes(L.sh.maxdim, L.la.S);
  int level = 0;
  if (!carry) {
    const int forced = g_chunk_fp8_stage;
    for (level = forced < 0 ? g_chunk_fp8_stage_max : forced; level > 0; --level) {
      const unsigned lds = lds0 + loco_stage_lds_bytes(L.sh, L.la, level);
      if (chunk_fp8_resident(chunk_fp8_kernel(four, false, level), lds) >= grid) break;
      if (forced >= 0) return -110;  // a forced level must hold the whole grid
    }
  } else if (g_chunk_fp8_stage > 0) {
    return -110;
  }
  g_chunk_fp8_last_stage = level;
  return loco_launch_pair_lds(chunk_fp8_kernel(four, carry, level), L, theta_row,
                              eps_rows, n_pairs, stream,
                              lds0 + loco_stage_lds_bytes(L.sh, L.la, level), n_steps,
                              salt_base);
}

extern "C" int es_loco_episode(const void* weights, const void* obmean, const void* obstd,
                               const int32_t* dims_host, int32_t ndims, const void* seed_dev,
                               int32_t n_steps, float ob_clip, const void* ac_std_dev,
                               int64_t row_stride,
                               void* s_glob, void* pos, const void* goal, const void* Am,
                               const void* Bm, const void* b0, const void* wv,
                               const void* wa, const void* wy, const void* wh, void* alive,
                               void* rew_total, void* member_steps, void* behv,
                               void* mo_sum, void* mo_sumsq, int32_t member_base,
                               int32_t n_members, int32_t salt_base, int32_t wrow0,
                               int32_t sdim, int32_t adim,
                               int32_t goal_flag, int32_t terminate, int32_t noiseless_from,
                               int32_t bins, int32_t eps, int32_t act_mode, float leak,
                               float ctrl, float alive_bonus, float fall_thr, float dt,
                               int32_t block_threads, void* stream) {
  LocoLaunch L;
  int rc = loco_setup(&L, weights, obmean, obstd, dims_host, ndims, seed_dev, ob_clip,
                      ac_std_dev, row_stride, s_glob, pos, goal, Am, Bm, b0, wv, wa, wy,
                      wh, alive, rew_total, member_steps, behv, mo_sum, mo_sumsq, sdim,
                      adim, goal_flag, terminate, noiseless_from, bins, eps, act_mode,
                      leak, ctrl, alive_bonus, fall_thr, dt);
  return rc ? rc
            : loco_launch_episode<uint16_t>(L, n_steps, member_base, n_members, salt_base,
                                            wrow0, block_threads, stream);
}

// fp32-weights step / episode: the argument lists of es_loco_step and
// es_loco_episode; `weights` is float32 (rows, row_stride), row_stride in
// elements.
extern "C" int es_loco_step_f32(
    const void* weights, const void* obmean, const void* obstd,
    const int32_t* dims_host, int32_t ndims, const void* seed_dev, uint64_t salt,
    float ob_clip, const void* ac_std_dev, int64_t row_stride, void* s_glob, void* pos,
    const void* goal, const void* Am, const void* Bm, const void* b0, const void* wv,
    const void* wa, const void* wy, const void* wh, void* alive, void* rew_total,
    void* member_steps, void* behv, void* mo_sum, void* mo_sumsq, int32_t n_pop,
    int32_t sdim, int32_t adim, int32_t goal_flag, int32_t terminate,
    int32_t noiseless_from, int32_t bins, int32_t eps, int32_t act_mode, float leak,
    float ctrl, float alive_bonus, float fall_thr, float dt, void* stream) {
  LocoLaunch L;
  int rc = loco_setup(&L, weights, obmean, obstd, dims_host, ndims, seed_dev, ob_clip,
                      ac_std_dev, row_stride, s_glob, pos, goal, Am, Bm, b0, wv, wa, wy,
                      wh, alive, rew_total, member_steps, behv, mo_sum, mo_sumsq, sdim,
                      adim, goal_flag, terminate, noiseless_from, bins, eps, act_mode,
                      leak, ctrl, alive_bonus, fall_thr, dt);
  return rc ? rc : loco_launch_step<float>(L, n_pop, salt, stream);
}

extern "C" int es_loco_episode_f32(
    const void* weights, const void* obmean, const void* obstd,
    const int32_t* dims_host, int32_t ndims, const void* seed_dev, int32_t n_steps,
    float ob_clip, const void* ac_std_dev, int64_t row_stride, void* s_glob, void* pos,
    const void* goal, const void* Am, const void* Bm, const void* b0, const void* wv,
    const void* wa, const void* wy, const void* wh, void* alive, void* rew_total,
    void* member_steps, void* behv, void* mo_sum, void* mo_sumsq, int32_t member_base,
    int32_t n_members, int32_t salt_base, int32_t wrow0, int32_t sdim, int32_t adim,
    int32_t goal_flag, int32_t terminate, int32_t noiseless_from, int32_t bins,
    int32_t eps, int32_t act_mode, float leak, float ctrl, float alive_bonus,
    float fall_thr, float dt, int32_t block_threads, void* stream) {
  LocoLaunch L;
  int rc = loco_setup(&L, weights, obmean, obstd, dims_host, ndims, seed_dev, ob_clip,
                      ac_std_dev, row_stride, s_glob, pos, goal, Am, Bm, b0, wv, wa, wy,
                      wh, alive, rew_total, member_steps, behv, mo_sum, mo_sumsq, sdim,
                      adim, goal_flag, terminate, noiseless_from, bins, eps, act_mode,
                      leak, ctrl, alive_bonus, fall_thr, dt);
  return rc ? rc
            : loco_launch_episode<float>(L, n_steps, member_base, n_members, salt_base,
                                         wrow0, block_threads, stream);
}
