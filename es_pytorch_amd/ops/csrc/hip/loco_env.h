// What the locomotion rollout files share (rollout_loco.hip,
// rollout_loco_wave.hip, rollout_loco_batch.hip): the kernel arguments of one
// launch, the bookkeeping of a slot kept on chip and the host function that
// validates an entry point's arguments and fills them.
#pragma once
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

// ---- what the whole-episode kernels that keep a slot on chip share ----------
// (rollout_loco_wave.hip, rollout_loco_batch.hip)
// What a step leaves in the slot's uniform registers.
struct LocoWaveSlot {
  float px, py, ph, gx, gy, rew_total, member_steps;
};

// loco_dyn_finish_n's bookkeeping of a live slot in its op order, computed by
// every lane from the reduced sums; returns whether the slot fell.
__device__ __forceinline__ bool loco_wave_book(const LocoArgs& la, LocoWaveSlot& st,
                                               float vfwd, float vy, float h, float asq) {
#pragma clang fp contract(off)
  float rew;
  if (la.goal) {
    const float rx = st.gx - st.px;
    const float ry = st.gy - st.py;
    const float inv = 1.0f / (sqrtf(rx * rx + ry * ry) + 1e-6f);
    rew = vfwd * rx * inv + vy * ry * inv - la.ctrl * asq + la.alive_bonus;
  } else {
    rew = vfwd - la.ctrl * asq + la.alive_bonus;
  }
  st.px = st.px + la.dt * vfwd;
  st.py = st.py + la.dt * vy;
  st.ph = h;
  st.rew_total = st.rew_total + rew;
  st.member_steps = st.member_steps + 1.0f;
  return la.terminate && h < la.fall_thr;
}

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
