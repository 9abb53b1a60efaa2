// Whole-episode rollout of the synthetic locomotion envs for eps_per_policy
// > 1: a 256-thread block per MEMBER, the member's E = eps episodes as the
// columns of matrix products on the fp32 matrix cores.
//
// Every other locomotion kernel treats the E slots of a member as unrelated:
// the block kernels stream the member's row once per slot and step, the wave
// kernels copy it E times into LDS. With the E observations side by side the
// forward of a layer is W^T (O x I) . X (I x E) and the dynamics are
// A^T (S x S) . s (S x E) + B^T (S x A) . a (A x E): every weight and every
// element of A is loaded once per step for all E episodes.
//
//  * Block g owns member m = member_base / eps + g and its slots b = m * eps
//    + e, e < E <= 16, for the whole launch.
//  * Numerics are those of the other kernels: weights exact bf16 (or fp32),
//    activations and state fp32, products exact and accumulated in fp32. The
//    instruction is v_mfma_f32_16x16x4_f32; a bf16 weight becomes its fp32
//    operand by a 16-bit shift and nothing else is rounded.
//  * Operands: lane l supplies A[m = l % 16][k = l / 16] and B[k = l / 16]
//    [n = l % 16] and holds D[4 * (l / 16) + r][n = l % 16] in accumulator
//    register r. Outputs are M, inputs K, the episode is column n.
//  * loco_batch_product is the one tile product, used for every layer, for A
//    and for B: a wave walks a group of 64 outputs, a lane loads its 4
//    contiguous outputs of row k0 + l / 16 as one vector (8 B of bf16, 16 B of
//    fp32: sixteen lanes read one contiguous run of a row of W^T (I, O), no
//    transpose) and issues 4 MFMAs per 4 inputs, MFMA j on element j of every
//    lane's vector, so tile j is the strided output set {ob + 4 m + j}. A
//    matrix that is not aligned for that (odd O, row stride n + 3) takes one
//    element load per lane per MFMA, tile j = {ob + m + 16 j}, coalesced
//    across lanes. 64-output groups, not 128: Humanoid's 256-wide layers then
//    give each of the four waves a group of its own and no partial sums.
//  * The four waves split the groups when there are at least three, the K
//    range otherwise; K partials meet in LDS and are added in slice order, so
//    the order of every sum is fixed by the shapes alone.
//  * Loads run a fragment (8 k-steps, 32 inputs) ahead of the MFMAs that use
//    them, in two named fragments that swap roles in a 2x unrolled loop.
//  * Inputs behind I get a zero B operand (the weight read is clamped into the
//    matrix and is finite); tiles behind O and columns behind E are computed
//    and never stored.
//  * LDS (column stride E): s[S][E] for the whole launch, two activation
//    buffers sized to the even- and the odd-indexed widths, the action
//    a[A][E], mo_sum and mo_sumsq [D][E], the K partials and a slab of
//    per-column scalars. Above 64 KB the launch raises the kernel's limit.
//    Global memory is read on entry and written once on exit.
//  * A column whose slot is dead is still multiplied but owns nothing: s, pos,
//    moments and sums keep their values from the step at which it died (the
//    wave kernel's semantic), a slot that enters dead writes nothing, and the
//    block leaves the loop when none of its columns is alive. Barriers are
//    block barriers; every branch around one is decided by the shapes or by
//    an LDS word all threads read.
//
// Arguments and return codes are es_loco_wave_episode's. -117: eps outside
// 1..16, member_base or n_members no multiple of eps, or an LDS need above the
// device's limit; nothing is launched.
#include "loco_env.h"

typedef float lb_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t lb_u32x2 __attribute__((ext_vector_type(2)));

#define LB_MAXE 16   // columns of an MFMA tile
#define LB_NE 4      // outputs a lane loads per row = MFMA tiles per k-step
#define LB_GROUP 64  // outputs of a group (16 lanes x LB_NE)
#define LB_U 8       // k-steps (4 inputs each) of a load fragment, vector form
#define LB_UE 2      // the same, element form (4 loads a k-step)
#define LB_WAVES 4
// per-column scalars and reduction scratch behind the matrices, in floats
#define LB_CS_FLOATS (10 * LB_MAXE + LB_WAVES * 4 * LB_MAXE + 4)
enum { LB_PX, LB_PY, LB_PH, LB_GX, LB_GY, LB_REW, LB_STEPS, LB_ALIVE, LB_ENTERED, LB_SPARE };

// LDS carve in floats; the host sizes it, the kernel reads the offsets.
struct LocoBatchCarve {
  int bufe, bufo, msum, msq, abuf, part, cs, total;
};

struct LocoBatchArgs {
  MlpShape sh;
  LocoArgs la;
  LocoPtrs P;
  LocoBatchCarve cv;
  int member_base, n_steps, salt_base;
};

// How the waves share a product with O outputs: G groups, KS K slices each.
__host__ __device__ __forceinline__ void loco_batch_split(int O, int* G, int* KS) {
  *G = (O + LB_GROUP - 1) / LB_GROUP;
  *KS = *G == 1 ? 4 : *G == 2 ? 2 : 1;
}
// rows of a K slice's partial slab
__host__ __device__ __forceinline__ int loco_batch_part_rows(int O, int G) {
  return G == 1 ? (O < LB_GROUP ? O : LB_GROUP) : LB_GROUP;
}

__device__ __forceinline__ uint32_t lb_ld(const uint16_t* p) { return *p; }
__device__ __forceinline__ uint32_t lb_ld(const float* p) { return __float_as_uint(*p); }

// A fragment: the raw weight registers of LB_U k-steps and their B operands.
template <int U, int NR>
struct LbFrag {
  uint32_t w[U][NR];
  float x[U];
};

// Y = M^T X for a row-major (I, O) matrix M in global memory and X (I, E) in
// LDS; epi(o, n, v) receives every element o < O, n < E once, from the lane
// that owns it. `part` holds the K partials. Called by the whole block; ends
// without a barrier (the caller's follows).
template <typename MT, bool NT, bool VEC, typename EPI>
__device__ __forceinline__ void loco_batch_product_v(const MT* __restrict__ M, int I, int O,
                                                     const float* X, int E, float* part,
                                                     int tid, EPI epi) {
  constexpr bool BF = sizeof(MT) == 2;
  constexpr int NR = (VEC && BF) ? 2 : 4;
  constexpr int U = VEC ? LB_U : LB_UE;
  typedef LbFrag<U, NR> Frag;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int mq = lane & 15, kq = lane >> 4;  // A row / B column, k of the lane
  const bool col = mq < E;
  const int xn = col ? mq : 0;
  int G, KS;
  loco_batch_split(O, &G, &KS);
  const int ksteps = (I + 3) >> 2;
  const int kper = (ksteps + KS - 1) / KS;  // k-steps of a slice
  const int ks = KS == 1 ? 0 : KS == 2 ? (wave & 1) : wave;
  const int g0 = KS == 1 ? wave : KS == 2 ? (wave >> 1) : 0;
  const int gstep = KS == 1 ? LB_WAVES : G;  // KS > 1: one unit per wave
  const int kb = ks * kper * 4, ke = min(I, (ks + 1) * kper * 4);
  const int R = loco_batch_part_rows(O, G);

  for (int g = g0; g < G; g += gstep) {
    const int ob = g * LB_GROUP;
    lb_f32x4 acc[LB_NE];
#pragma unroll
    for (int j = 0; j < LB_NE; ++j) acc[j] = lb_f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    auto load = [&](Frag& f, int k0) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = k0 + 4 * u + kq;
        const bool ok = i < ke;
        const int ic = min(i, I - 1);
        f.x[u] = (ok && col) ? X[ic * E + xn] : 0.0f;
        if constexpr (VEC) {
          const MT* p = M + ((uint32_t)ic * (uint32_t)O + (uint32_t)min(ob + LB_NE * mq, O - LB_NE));
          if constexpr (BF) {
            const lb_u32x2* q = reinterpret_cast<const lb_u32x2*>(p);
            const lb_u32x2 v = NT ? __builtin_nontemporal_load(q) : *q;
            f.w[u][0] = v.x; f.w[u][1] = v.y;
          } else {
            const es_u32x4* q = reinterpret_cast<const es_u32x4*>(p);
            const es_u32x4 v = NT ? __builtin_nontemporal_load(q) : *q;
            f.w[u][0] = v.x; f.w[u][1] = v.y; f.w[u][2] = v.z; f.w[u][3] = v.w;
          }
        } else {
          const uint32_t row = (uint32_t)ic * (uint32_t)O;
#pragma unroll
          for (int j = 0; j < LB_NE; ++j)
            f.w[u][j] = lb_ld(M + (row + (uint32_t)min(ob + mq + 16 * j, O - 1)));
        }
      }
    };
    auto mma = [&](const Frag& f) {
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int j = 0; j < LB_NE; ++j) {
          uint32_t r;
          if constexpr (VEC && BF)
            r = (j & 1) ? (f.w[u][j >> 1] & 0xFFFF0000u) : (f.w[u][j >> 1] << 16);
          else if constexpr (BF)
            r = f.w[u][j] << 16;
          else
            r = f.w[u][j];
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(r), f.x[u], acc[j],
                                                        0, 0, 0);
        }
    };
    // two fragments swapping roles: the loads of one are in flight while the
    // MFMAs consume the other (wave-uniform control flow throughout)
    if (kb < ke) {
      constexpr int KB = 4 * U;
      Frag fa, fb;
      int k = kb;
      load(fa, k);
      for (;;) {
        if (k + KB >= ke) { mma(fa); break; }
        load(fb, k + KB);
        mma(fa);
        k += KB;
        if (k + KB >= ke) { mma(fb); break; }
        load(fa, k + KB);
        mma(fb);
        k += KB;
      }
    }

    // accumulator register r of tile j: output o, column mq
    auto out_of = [&](int j, int r) {
      const int mrow = 4 * kq + r;
      return VEC ? ob + LB_NE * mrow + j : ob + mrow + 16 * j;
    };
    if (KS > 1) {  // block-uniform: every wave has exactly one unit
      if (ks > 0) {
        float* ps = part + (g * (KS - 1) + ks - 1) * R * E;
#pragma unroll
        for (int j = 0; j < LB_NE; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int o = out_of(j, r);
            if (o < O && col) ps[(o - ob) * E + mq] = acc[j][r];
          }
      }
      __syncthreads();
      if (ks > 0) continue;
    }
#pragma unroll
    for (int j = 0; j < LB_NE; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = out_of(j, r);
        if (o < O && col) {
          float v = acc[j][r];
          for (int q = 1; q < KS; ++q)
            v += part[((g * (KS - 1) + q - 1) * R + (o - ob)) * E + mq];
          epi(o, mq, v);
        }
      }
  }
}

// The vector form where the matrix is aligned for it (block-uniform), the
// element form otherwise.
template <typename MT, bool NT, typename EPI>
__device__ __forceinline__ void loco_batch_product(const MT* __restrict__ M, int I, int O,
                                                   const float* X, int E, float* part,
                                                   int tid, EPI epi) {
  asm volatile("" : "+v"(tid));  // no lane invariant outlives a product
  const bool vec = O % LB_NE == 0 &&
                   (reinterpret_cast<uintptr_t>(M) & (LB_NE * sizeof(MT) - 1)) == 0;
  if (vec)
    loco_batch_product_v<MT, NT, true>(M, I, O, X, E, part, tid, epi);
  else
    loco_batch_product_v<MT, NT, false>(M, I, O, X, E, part, tid, epi);
}

__device__ __forceinline__ float lb_weight(const uint16_t* w, int k) { return bf2f(w[k]); }
__device__ __forceinline__ float lb_weight(const float* w, int k) { return w[k]; }

template <typename WT>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
loco_batch_episode_kernel(LocoBatchArgs W) {
  extern __shared__ __attribute__((aligned(16))) float lb_smem[];
  const MlpShape& sh = W.sh;
  const LocoArgs& la = W.la;
  const LocoPtrs& P = W.P;
  const int S = la.S, A = la.A, D = la.D, E = la.eps;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m = W.member_base / E + blockIdx.x;
  const int b0slot = m * E;

  float* s = lb_smem;
  float* bufe = lb_smem + W.cv.bufe;
  float* bufo = lb_smem + W.cv.bufo;
  float* msum = lb_smem + W.cv.msum;
  float* msq = lb_smem + W.cv.msq;
  float* abuf = lb_smem + W.cv.abuf;
  float* part = lb_smem + W.cv.part;
  float* cs = lb_smem + W.cv.cs;                   // [10][16] per-column scalars
  float* red = cs + 10 * LB_MAXE;                  // [waves][4][16]
  int* any_alive = reinterpret_cast<int*>(red + LB_WAVES * 4 * LB_MAXE);
  auto csv = [&](int q, int n) -> float& { return cs[q * LB_MAXE + n]; };

  // ---- entry: the columns' scalars; a member whose columns are all dead
  // writes nothing
  if (wave == 0) {
    bool al = false;
    if (lane < E) {
      const int b = b0slot + lane;
      al = P.alive[b] > 0.0f;
      csv(LB_PX, lane) = P.pos[(int64_t)b * 3 + 0];
      csv(LB_PY, lane) = P.pos[(int64_t)b * 3 + 1];
      csv(LB_PH, lane) = 0.0f;
      csv(LB_GX, lane) = la.goal ? P.goal[(int64_t)b * 2 + 0] : 0.0f;
      csv(LB_GY, lane) = la.goal ? P.goal[(int64_t)b * 2 + 1] : 0.0f;
      csv(LB_REW, lane) = P.rew_total[b];
      csv(LB_STEPS, lane) = P.member_steps[b];
      csv(LB_ALIVE, lane) = al ? 1.0f : 0.0f;
      csv(LB_ENTERED, lane) = al ? 1.0f : 0.0f;
    }
    const bool some = __ballot(al) != 0;
    if (lane == 0) *any_alive = some;
  }
  __syncthreads();
  if (*any_alive == 0) return;
  for (int idx = tid; idx < S * E; idx += 256) {
    const int n = idx / S, i = idx - n * S;
    s[i * E + n] = P.s_glob[(int64_t)(b0slot + n) * S + i];
  }
  for (int idx = tid; idx < D * E; idx += 256) {
    const int n = idx / D, i = idx - n * D;
    msum[i * E + n] = P.mo_sum[(int64_t)(b0slot + n) * D + i];
    msq[i * E + n] = P.mo_sumsq[(int64_t)(b0slot + n) * D + i];
  }
  __syncthreads();

  const WT* wrow = reinterpret_cast<const WT*>(P.weights) +
                   (int64_t)(m - la.wrow0) * la.row_stride;
  const int odim = sh.dims[sh.n_layers];
  const uint64_t seed0 = P.seed_dev ? *P.seed_dev : 0;
  const float ac_std = P.ac_std_dev ? *P.ac_std_dev : 0.0f;
  const float leak = la.leak;
  const float* b0v = P.b0;

  for (int t = 1; t <= W.n_steps; ++t) {
    // the thread id the products index by, opaque per step: their lane
    // invariants are recomputed here instead of being hoisted out of the
    // step loop and spilled
    int tl = tid;
    asm volatile("" : "+v"(tl));
    // ---- observation: loco_build_obs's expression, division and clamp
    // included, goal-relative dims from the current position
    for (int idx = tid; idx < D * E; idx += 256) {
      const int i = idx / E, n = idx - i * E;
      float raw;
      if (i < S) raw = s[idx];
      else raw = (csv(i == S ? LB_GX : LB_GY, n) - csv(i == S ? LB_PX : LB_PY, n)) * 0.1f;
      bufe[idx] = fclampf((raw - P.obmean[i]) / P.obstd[i], -la.ob_clip, la.ob_clip);
    }
    __syncthreads();
    // ---- forward: bias and tanh as mlp_layers applies them
    float *x = bufe, *y = bufo;
    for (int l = 0; l < sh.n_layers; ++l) {
      const WT* Bs = wrow + sh.boff[l];
      loco_batch_product<WT, true>(wrow + sh.woff[l], sh.dims[l], sh.dims[l + 1], x, E, part,
                                   tl, [=](int o, int n, float v) {
                                     y[o * E + n] = tanhf(lb_weight(Bs, o) + v);
                                   });
      __syncthreads();
      float* sw = x; x = y; y = sw;
    }
    // ---- action: loco_decode_action's four modes per column, its tie rule,
    // its noise keys and counters
    const uint64_t seed = seed0 + (uint64_t)(W.salt_base + t);
    for (int idx = tid; idx < A * E; idx += 256) {
      const int k = idx / E, n = idx - k * E;
      const int b = b0slot + n;
      float a;
      if (la.act_mode == 2 || la.act_mode == 3) {
        a = la.act_mode == 2 ? x[(1 + k) * E + n] : x[k * E + n];
        const float std_o = la.act_mode == 2 ? x[n] : fabsf(x[(A + k) * E + n]);
        if (b < la.noiseless_from && std_o != 0.0f)
          a += std_o * es_actnoise(seed, (uint64_t)b * odim + k);
        a = fclampf(a, -1.0f, 1.0f);
      } else if (la.bins > 1) {
        int best = 0;
        float bv = x[(k * la.bins) * E + n];
        for (int j = 1; j < la.bins; ++j) {
          const float v = x[(k * la.bins + j) * E + n];
          if (v > bv) { bv = v; best = j; }
        }
        a = -1.0f + 2.0f * (float)best / (float)(la.bins - 1);
      } else {
        a = x[idx];
        if (ac_std != 0.0f && b < la.noiseless_from)
          a += ac_std * es_actnoise(seed, (uint64_t)b * A + k);
        a = fclampf(a, -1.0f, 1.0f);
      }
      abuf[idx] = a;
    }
    __syncthreads();
    // ---- dynamics: pre = s A + a B (+ b0), then tanh and the leak; the lane
    // that owns (o, n) also takes the column's moments of the new state
    loco_batch_product<uint16_t, false>(P.Am, S, S, s, E, part, tl,
                                        [=](int o, int n, float v) { bufe[o * E + n] = v; });
    __syncthreads();
    loco_batch_product<float, false>(P.Bm, A, S, abuf, E, part, tl, [=](int o, int n, float v) {
#pragma clang fp contract(off)
      const int idx = o * E + n;
      const float sn = (1.0f - leak) * s[idx] + leak * tanhf(b0v[o] + (bufe[idx] + v));
      if (cs[LB_ALIVE * LB_MAXE + n] > 0.0f) {
        s[idx] = sn;
        msum[idx] = msum[idx] + sn;
        msq[idx] = msq[idx] + sn * sn;
      }
    });
    __syncthreads();
    // ---- vfwd, vy, h, |a|^2 per column: 16 partitions of the rows, added in
    // a fixed order (lane groups, then waves)
    {
      const int n = lane & 15, p = tid >> 4;
      float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f, p3 = 0.0f;
      if (n < E) {
        for (int o = p; o < S; o += 16) {
          const float sn = s[o * E + n];
          p0 = fmaf(sn, P.wv[o], p0);
          p1 = fmaf(sn, P.wy[o], p1);
          p2 = fmaf(sn, P.wh[o], p2);
        }
        for (int k = p; k < A; k += 16) {
          const float a = abuf[k * E + n];
          p0 = fmaf(0.5f * a, P.wa[k], p0);
          p3 = fmaf(a, a, p3);
        }
      }
#pragma unroll
      for (int off = 16; off < 64; off <<= 1) {
        p0 += __shfl_xor(p0, off, 64);
        p1 += __shfl_xor(p1, off, 64);
        p2 += __shfl_xor(p2, off, 64);
        p3 += __shfl_xor(p3, off, 64);
      }
      if (lane < 16) {
        float* rw = red + wave * 4 * LB_MAXE;
        rw[0 * LB_MAXE + n] = p0;
        rw[1 * LB_MAXE + n] = p1;
        rw[2 * LB_MAXE + n] = p2;
        rw[3 * LB_MAXE + n] = p3;
      }
    }
    __syncthreads();
    // ---- bookkeeping of a live column (loco_dyn_finish_n's op order)
    if (wave == 0) {
      bool al = false;
      if (lane < E && csv(LB_ALIVE, lane) > 0.0f) {
#pragma clang fp contract(off)
        float r4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float v = 0.0f;
          for (int w = 0; w < LB_WAVES; ++w) v += red[(w * 4 + q) * LB_MAXE + lane];
          r4[q] = v;
        }
        LocoWaveSlot st;
        st.px = csv(LB_PX, lane); st.py = csv(LB_PY, lane); st.ph = csv(LB_PH, lane);
        st.gx = csv(LB_GX, lane); st.gy = csv(LB_GY, lane);
        st.rew_total = csv(LB_REW, lane); st.member_steps = csv(LB_STEPS, lane);
        const bool done = loco_wave_book(la, st, r4[0], r4[1], r4[2], r4[3]);
        csv(LB_PX, lane) = st.px; csv(LB_PY, lane) = st.py; csv(LB_PH, lane) = st.ph;
        csv(LB_REW, lane) = st.rew_total; csv(LB_STEPS, lane) = st.member_steps;
        if (la.goal) {  // goal-relative dims of the moments, from the new position
          const float rel0 = (st.gx - st.px) * 0.1f, rel1 = (st.gy - st.py) * 0.1f;
          msum[S * E + lane] = msum[S * E + lane] + rel0;
          msq[S * E + lane] = msq[S * E + lane] + rel0 * rel0;
          msum[(S + 1) * E + lane] = msum[(S + 1) * E + lane] + rel1;
          msq[(S + 1) * E + lane] = msq[(S + 1) * E + lane] + rel1 * rel1;
        }
        al = !done;
        csv(LB_ALIVE, lane) = al ? 1.0f : 0.0f;
      }
      const bool some = __ballot(al) != 0;
      if (lane == 0) *any_alive = some;
    }
    __syncthreads();
    if (*any_alive == 0) break;
  }

  // ---- written once, for the columns that entered alive; behv is the
  // position of the last step the slot took alive
  for (int idx = tid; idx < S * E; idx += 256) {
    const int n = idx / S, i = idx - n * S;
    if (csv(LB_ENTERED, n) > 0.0f) P.s_glob[(int64_t)(b0slot + n) * S + i] = s[i * E + n];
  }
  for (int idx = tid; idx < D * E; idx += 256) {
    const int n = idx / D, i = idx - n * D;
    if (csv(LB_ENTERED, n) > 0.0f) {
      P.mo_sum[(int64_t)(b0slot + n) * D + i] = msum[i * E + n];
      P.mo_sumsq[(int64_t)(b0slot + n) * D + i] = msq[i * E + n];
    }
  }
  if (tid < E && csv(LB_ENTERED, tid) > 0.0f) {
    const int b = b0slot + tid;
    for (int q = 0; q < 3; ++q) {
      const float v = csv(LB_PX + q, tid);
      P.pos[(int64_t)b * 3 + q] = v;
      P.behv[(int64_t)b * 3 + q] = v;
    }
    P.rew_total[b] = csv(LB_REW, tid);
    P.member_steps[b] = csv(LB_STEPS, tid);
    P.alive[b] = csv(LB_ALIVE, tid);
  }
}

// ---- host side --------------------------------------------------------------
// LDS bytes a block may have: what the device reports, or gfx950's 160 KB
// where there is no device to ask (a check on a build machine).
static int loco_batch_lds_limit() {
  int dev = 0, v = 0;
  if (hipGetDevice(&dev) == hipSuccess &&
      hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) ==
          hipSuccess && v > 0)
    return v;
  (void)hipGetLastError();
  return 160 * 1024;
}

// The coverage, the one place it is decided: 0 and the carve, or -117.
static int loco_batch_geometry(const MlpShape& sh, int S, int A, int eps,
                               LocoBatchCarve* cv) {
  if (eps < 1 || eps > LB_MAXE || S < 1 || A < 1) return -117;
  const int E = eps, D = sh.dims[0];
  int we = S, wo = 0, pf = 0;
  auto product = [&](int O) {
    int G, KS;
    loco_batch_split(O, &G, &KS);
    pf = std::max(pf, G * (KS - 1) * loco_batch_part_rows(O, G));
  };
  for (int l = 0; l <= sh.n_layers; ++l) {
    int& w = (l & 1) ? wo : we;
    w = std::max(w, sh.dims[l]);
    if (l > 0) product(sh.dims[l]);
  }
  product(S);  // A and B
  int64_t off = (int64_t)S * E;
  auto take = [&](int64_t n) { const int64_t o = off; off += (n + 3) & ~(int64_t)3; return (int)o; };
  off = (off + 3) & ~(int64_t)3;
  cv->bufe = take((int64_t)we * E);
  cv->bufo = take((int64_t)wo * E);
  cv->msum = take((int64_t)D * E);
  cv->msq = take((int64_t)D * E);
  cv->abuf = take((int64_t)A * E);
  cv->part = take((int64_t)pf * E);
  cv->cs = take(LB_CS_FLOATS);
  cv->total = (int)off;
  return off * 4 > loco_batch_lds_limit() ? -117 : 0;
}

static int loco_batch_launch(bool f32, const LocoLaunch& L, int32_t n_steps,
                             int32_t member_base, int32_t n_members, int32_t salt_base,
                             int32_t wrow0, int32_t eps, void* stream) {
  LocoBatchArgs W;
  W.sh = L.sh; W.la = L.la; W.P = L.P;
  W.la.wrow0 = wrow0;
  const int rc = loco_batch_geometry(W.sh, W.la.S, W.la.A, eps, &W.cv);
  if (rc) return rc;
  if (member_base < 0 || member_base % eps || (n_members > 0 && n_members % eps)) return -117;
  if (n_steps <= 0 || n_members <= 0) return 0;
  W.member_base = member_base; W.n_steps = n_steps; W.salt_base = salt_base;
  const dim3 grid((unsigned)(n_members / eps)), block(64 * LB_WAVES);
  const unsigned lds = (unsigned)W.cv.total * 4;
  const void* fn = f32 ? (const void*)loco_batch_episode_kernel<float>
                       : (const void*)loco_batch_episode_kernel<uint16_t>;
  // above 64 KB the kernel's limit is raised, once per kernel to the most it
  // has been asked for
  static unsigned raised[2] = {65536, 65536};
  if (lds > raised[f32]) {
    const hipError_t e =
        hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    raised[f32] = lds;
  }
  if (f32)
    loco_batch_episode_kernel<float><<<grid, block, lds, (hipStream_t)stream>>>(W);
  else
    loco_batch_episode_kernel<uint16_t><<<grid, block, lds, (hipStream_t)stream>>>(W);
  ES_CHECK_LAUNCH();
  return 0;
}

// What a launch with this net, env and eps would return for the shapes alone
// (0, one of mlp_shape_init's codes, -103, -104 or -117), without launching.
extern "C" int es_loco_batch_check(const int32_t* dims_host, int32_t ndims,
                                   int64_t row_stride, int32_t sdim, int32_t adim,
                                   int32_t goal_flag, int32_t f32, int32_t eps) {
  (void)f32;  // both row types need the same LDS
  MlpShape sh;
  int rc = mlp_shape_init(&sh, dims_host, ndims, row_stride);
  if (rc) return rc;
  if (adim > 64 || sdim > ES_MAXDIM) return -103;
  if (sh.dims[0] != sdim + (goal_flag ? 2 : 0)) return -104;
  LocoBatchCarve cv;
  return loco_batch_geometry(sh, sdim, adim, eps, &cv);
}

// es_loco_wave_episode's argument list; eps here is also the number of
// columns of a block, and member_base and n_members (slots) are multiples of
// it. n_steps <= 0 or n_members <= 0 is a no-op returning 0.
#define LOCO_BATCH_ENTRY(NAME, F32)                                                       \
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
              : loco_batch_launch(F32, L, n_steps, member_base, n_members, salt_base,     \
                                  wrow0, eps, stream);                                    \
  }

LOCO_BATCH_ENTRY(es_loco_batch_episode, false)
LOCO_BATCH_ENTRY(es_loco_batch_episode_f32, true)
