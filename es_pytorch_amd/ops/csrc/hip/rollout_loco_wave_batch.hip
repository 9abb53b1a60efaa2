// Whole-episode rollout of the synthetic locomotion envs for SMALL envs and
// nets (state, action and every layer at most 64 wide) and eps_per_policy =
// E <= 16: a wavefront per MEMBER, the member's E episodes as the columns of
// v_mfma_f32_16x16x4_f32 products, everything a step touches in registers.
//
// rollout_loco_wave.hip gives every slot a wave and so copies a member's row
// into LDS E times and walks the scalar forward E times;
// rollout_loco_batch.hip has the E episodes side by side but is a 256-thread
// block per member with block barriers and activations in LDS. Here:
//
//  * Work split. A 256-thread block is four independent waves; wave w of
//    block g owns member member_base / eps + g * MPB + w and its slots b =
//    m * eps + e for the whole launch. MPB is 4, 2 or 1: the most member
//    regions that fit WAVE_LDS_BUDGET beside the env block. The
//    __syncthreads() behind the env-block staging, ahead of every return, is
//    the only block barrier. The step loop runs while a ballot over the
//    per-column alive flag is non-zero; every branch around an MFMA or a
//    cross-lane operation is decided by the shapes (kernel arguments) or by
//    such a ballot.
//  * Operands. Lane l = 16 g + n supplies A[m = l % 16][k = l / 16] and
//    B[k = l / 16][n = l % 16] and holds D[4 g + r][n] in accumulator
//    register r. Outputs are M, inputs K, the episode is column n.
//  * Vectors live in registers as tiles: a vector of up to 64 rows is four
//    tiles of four registers, row 16 t + 4 g + r of column n in register r of
//    tile t of lane (g, n). A product leaves its output like that, and the
//    next product takes register r of tile t as the B operand of its MFMA
//    (t, r) as it stands: the K order is permuted, not the data. The four
//    inputs of that MFMA are rows {16 t + 4 g + r : g = 0..3}, so lane (g, m)
//    supplies W[input 16 t + 4 g + r][output 16 T + m] as its A operand. The
//    observation, the hidden layers, the state s, the action a and the
//    moments all use this layout; the dynamics A^T s + B^T a are the same
//    product on the env block. The order of every sum is fixed by the shapes.
//  * Weights. Each wave copies its member's row into its LDS region once,
//    transposed: a layer is stored output-major, the inputs of one output
//    contiguous, inputs and outputs padded to multiples of 16 with zeros
//    (the bias too, kept as fp32), so rows behind I and O contribute exact
//    zeros with no mask in the loop and tanh(0) = 0 carries them forward.
//    Lane (g, m) reads its inputs 16 t + 4 g .. + 3 of output 16 T + m with
//    one ds_read_b64 (bf16) or ds_read_b128 (fp32) for the four MFMAs
//    (t, 0..3). The row pitch is the padded input count plus 16 BYTES:
//    Ipad / 2 + 4 dwords for bf16, Ipad + 4 for fp32, in both cases 4 * odd.
//    A lane's dword address is m * pitch + (2 or 4) * g + const; with pitch
//    = 4 * odd the sixteen m of a lane group fall on the sixteen distinct
//    multiples of 4 modulo 64, so the 32 lanes of a half-wave b64 read and
//    the 16 lanes of a quarter-wave b128 read cover all 64 banks once. A
//    pitch of Ipad alone (a multiple of 16 inputs) would put the sixteen m
//    on one or two banks at 64 wide.
//  * The env block - A (bf16) and B (fp32) in the same operand layout, b0,
//    wv, wy, wh, wa, obmean, obstd padded with zeros (obstd with ones) - is
//    staged once per block by all 256 threads.
//  * The action decode of the plain head stays in registers (output k is
//    action k). The binned head and act_mode 2 and 3 pass the net output
//    through a per-wave strip of 16 columns x 68 floats, wave-local, and end
//    with the action back in operand layout; the strip is part of a member's
//    region only where the last layer is wider than the action.
//  * vfwd, vy, h and |a|^2 are sums over rows: within a lane ascending over
//    tiles then registers, then __shfl_xor 16 and 32 with a + b on both
//    sides, so the four lanes of a column end on the same bits and each runs
//    loco_wave_book for its column. A dead column is still multiplied but
//    every update of what it owns is selected away; a slot that enters dead
//    writes nothing. Columns behind E are dead columns of zeros.
//  * Numerics are those of the other kernels: weights exact bf16 (or fp32),
//    a bf16 weight becomes its fp32 operand by a 16-bit shift, activations
//    and state fp32, products exact and accumulated in fp32.
//
// Arguments and return codes are es_loco_batch_episode's. -118: eps outside
// 1..16, member_base or n_members no multiple of eps, a state, an action or a
// layer wider than 64, or a member region that does not fit the LDS budget
// beside the env block; nothing is launched.
#include "loco_env.h"
#include "wave_mlp.h"

typedef float lwb_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t lwb_u32x2 __attribute__((ext_vector_type(2)));

#define LWB_MAXE 16       // columns of an MFMA tile
#define LWB_T 4           // tiles of a vector (64 rows)
#define LWB_STRIP_P 68    // floats of a strip column: 64 + 4, 4 * odd
#define LWB_STRIP_BYTES (LWB_MAXE * LWB_STRIP_P * 4)

__host__ __device__ __forceinline__ int lwb_pad(int n) { return (n + 15) & ~15; }
// bytes from one output's inputs to the next's
__host__ __device__ __forceinline__ int lwb_pitch(int I, int esz) { return lwb_pad(I) * esz + 16; }

// The env block in LDS (byte offsets), carved the same way by host and kernel.
struct LwbEnv {
  int At, Bt, b0, wv, wy, wh, wa, mean, std, bytes;
};
__host__ __device__ __forceinline__ LwbEnv lwb_env_carve(int S, int A, int D) {
  const int Sp = lwb_pad(S), Ap = lwb_pad(A), Dp = lwb_pad(D);
  LwbEnv e;
  e.At = 0;
  e.Bt = e.At + Sp * lwb_pitch(S, 2);
  e.b0 = e.Bt + Sp * lwb_pitch(A, 4);
  e.wv = e.b0 + Sp * 4;
  e.wy = e.wv + Sp * 4;
  e.wh = e.wy + Sp * 4;
  e.wa = e.wh + Sp * 4;
  e.mean = e.wa + Ap * 4;
  e.std = e.mean + Dp * 4;
  e.bytes = e.std + Dp * 4;
  return e;
}

struct LocoWaveBatchArgs {
  MlpShape sh;
  LocoArgs la;
  LocoPtrs P;
  int member_base, n_members, n_steps, salt_base;  // member_base, n_members: slots
  int mpb;           // members per block
  int env_bytes;     // LDS bytes of the env block, a multiple of 16
  int region_bytes;  // LDS bytes of one member's region, a multiple of 16
  int woff[ES_MAXL], boff[ES_MAXL];  // byte offsets of a layer's W and bias in a region
  int strip_off;     // of the decode strip, -1 where the head needs none
};

__device__ __forceinline__ lwb_f32x4 lwb_ld4(const char* p) {
  return *reinterpret_cast<const lwb_f32x4*>(p);
}

// The A operands of MFMAs (t, 0..3) of one output tile: four consecutive
// inputs of this lane's output, one LDS read.
__device__ __forceinline__ void lwb_frag(const char* p, float (&w)[4], uint16_t) {
  const lwb_u32x2 v = *reinterpret_cast<const lwb_u32x2*>(p);
  w[0] = __uint_as_float(v.x << 16);
  w[1] = __uint_as_float(v.x & 0xFFFF0000u);
  w[2] = __uint_as_float(v.y << 16);
  w[3] = __uint_as_float(v.y & 0xFFFF0000u);
}
__device__ __forceinline__ void lwb_frag(const char* p, float (&w)[4], float) {
  const lwb_f32x4 v = lwb_ld4(p);
  w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
}

// acc[T] += M^T x for T < nTo over the input tiles t < nTi of x (nTi >= 1).
// M is in LDS in operand layout, `lanep` this lane's base in it (output m,
// inputs 4 g). Input tiles outermost, so the nTo accumulators are independent
// chains; two fragment sets swap roles, the reads of tile t + 1 issued ahead
// of the MFMAs of tile t.
template <typename MT, int nTo>
__device__ __forceinline__ void lwb_product_n(const char* lanep, int pitch, int nTi,
                                              const lwb_f32x4 (&x)[LWB_T],
                                              lwb_f32x4 (&acc)[LWB_T]) {
  auto load = [&](float (&w)[LWB_T][4], int t) {
#pragma unroll
    for (int T = 0; T < LWB_T; ++T)
      if (T < nTo) lwb_frag(lanep + T * 16 * pitch + t * 16 * (int)sizeof(MT), w[T], MT());
  };
  auto mma = [&](const float (&w)[LWB_T][4], const lwb_f32x4& xt) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int T = 0; T < LWB_T; ++T)
        if (T < nTo)
          acc[T] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[T][r], xt[r], acc[T], 0, 0, 0);
  };
  float wa[LWB_T][4], wb[LWB_T][4];
  load(wa, 0);
  if (nTi > 1) load(wb, 1);
  mma(wa, x[0]);
  if (nTi > 1) {
    if (nTi > 2) load(wa, 2);
    mma(wb, x[1]);
    if (nTi > 2) {
      if (nTi > 3) load(wb, 3);
      mma(wa, x[2]);
      if (nTi > 3) mma(wb, x[3]);
    }
  }
}

// The output tile count is a template argument: each count gets straight runs
// of MFMAs, not an MFMA behind a guard of its own.
template <typename MT>
__device__ __forceinline__ void lwb_product(const char* lanep, int pitch, int nTi, int nTo,
                                            const lwb_f32x4 (&x)[LWB_T],
                                            lwb_f32x4 (&acc)[LWB_T]) {
  if (nTo == 1) lwb_product_n<MT, 1>(lanep, pitch, nTi, x, acc);
  else if (nTo == 2) lwb_product_n<MT, 2>(lanep, pitch, nTi, x, acc);
  else if (nTo == 3) lwb_product_n<MT, 3>(lanep, pitch, nTi, x, acc);
  else lwb_product_n<MT, 4>(lanep, pitch, nTi, x, acc);
}

// writes of this wave's lanes to its LDS, visible to its other lanes
__device__ __forceinline__ void lwb_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename WT>
__device__ __forceinline__ void loco_wave_batch_episode_body(const LocoWaveBatchArgs& W) {
  extern __shared__ __attribute__((aligned(16))) char lwb_smem[];
  const MlpShape& sh = W.sh;
  const LocoArgs& la = W.la;
  const LocoPtrs& P = W.P;
  const int S = la.S, A = la.A, D = la.D, E = la.eps;
  const int Sp = lwb_pad(S), Ap = lwb_pad(A), Dp = lwb_pad(D);
  const LwbEnv ev = lwb_env_carve(S, A, D);
  const int pitchA = lwb_pitch(S, 2), pitchB = lwb_pitch(A, 4);

  // ---- env block: staged by the whole block, read by each of its waves
  {
    const int tid = threadIdx.x;
    uint16_t* At = reinterpret_cast<uint16_t*>(lwb_smem + ev.At);
    float* Bt = reinterpret_cast<float*>(lwb_smem + ev.Bt);
    for (int idx = tid; idx < Sp * Sp; idx += 64 * WAVE_WAVES) {
      const int i = idx / Sp, o = idx - i * Sp;
      At[o * (pitchA / 2) + i] = (i < S && o < S) ? P.Am[i * S + o] : (uint16_t)0;
    }
    for (int idx = tid; idx < Ap * Sp; idx += 64 * WAVE_WAVES) {
      const int k = idx / Sp, o = idx - k * Sp;
      Bt[o * (pitchB / 4) + k] = (k < A && o < S) ? P.Bm[k * S + o] : 0.0f;
    }
    auto vec = [&](int off, const float* src, int n, int np, float fill) {
      if (tid < np) reinterpret_cast<float*>(lwb_smem + off)[tid] = tid < n ? src[tid] : fill;
    };
    vec(ev.b0, P.b0, S, Sp, 0.0f);
    vec(ev.wv, P.wv, S, Sp, 0.0f);
    vec(ev.wy, P.wy, S, Sp, 0.0f);
    vec(ev.wh, P.wh, S, Sp, 0.0f);
    vec(ev.wa, P.wa, A, Ap, 0.0f);
    vec(ev.mean, P.obmean, D, Dp, 0.0f);
    vec(ev.std, P.obstd, D, Dp, 1.0f);
  }
  __syncthreads();
  // no block barrier from here on

  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
  const int mrel = blockIdx.x * W.mpb + wave;  // member of the launch
  if (wave >= W.mpb || mrel * E >= W.n_members) return;
  const int m = W.member_base / E + mrel;
  const bool col = n < E;
  const int b = m * E + (col ? n : 0);  // this column's slot
  bool alive = col && P.alive[b] > 0.0f;
  const bool entered = alive;  // a slot that enters dead keeps everything it owns
  if (__ballot(alive) == 0) return;

  // ---- the member's row, global -> this wave's region, in operand layout
  char* region = lwb_smem + W.env_bytes + wave * W.region_bytes;
  {
    const WT* row = reinterpret_cast<const WT*>(P.weights) +
                    (int64_t)(m - la.wrow0) * la.row_stride;
    for (int l = 0; l < sh.n_layers; ++l) {
      const int I = sh.dims[l], O = sh.dims[l + 1], Ip = lwb_pad(I), Op = lwb_pad(O);
      const int pe = lwb_pitch(I, (int)sizeof(WT)) / (int)sizeof(WT);
      WT* wl = reinterpret_cast<WT*>(region + W.woff[l]);
      float* bl = reinterpret_cast<float*>(region + W.boff[l]);
      const WT* wg = row + sh.woff[l];
      if (lane < Op) {
        for (int i = 0; i < Ip; ++i)
          wl[lane * pe + i] = (i < I && lane < O) ? wg[i * O + lane] : (WT)0;
        bl[lane] = lane < O ? clw_weight(row + sh.boff[l], lane) : 0.0f;
      }
    }
    lwb_wave_sync();
  }

  // ---- the member's E slots, in registers: row 16 t + 4 g + r of column n
  lwb_f32x4 s[LWB_T], ms[LWB_T], mq[LWB_T];
#pragma unroll
  for (int t = 0; t < LWB_T; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 16 * t + 4 * g + r;
      s[t][r] = (entered && i < S) ? P.s_glob[(int64_t)b * S + i] : 0.0f;
      ms[t][r] = (entered && i < D) ? P.mo_sum[(int64_t)b * D + i] : 0.0f;
      mq[t][r] = (entered && i < D) ? P.mo_sumsq[(int64_t)b * D + i] : 0.0f;
    }
  LocoWaveSlot st;
  st.px = entered ? P.pos[(int64_t)b * 3 + 0] : 0.0f;
  st.py = entered ? P.pos[(int64_t)b * 3 + 1] : 0.0f;
  st.ph = 0.0f;
  st.gx = (entered && la.goal) ? P.goal[(int64_t)b * 2 + 0] : 0.0f;
  st.gy = (entered && la.goal) ? P.goal[(int64_t)b * 2 + 1] : 0.0f;
  st.rew_total = entered ? P.rew_total[b] : 0.0f;
  st.member_steps = entered ? P.member_steps[b] : 0.0f;

  const int odim = sh.dims[sh.n_layers];
  const uint64_t seed0 = P.seed_dev ? *P.seed_dev : 0;
  const float ac_std = P.ac_std_dev ? *P.ac_std_dev : 0.0f;
  const bool gauss = la.act_mode == 2 || la.act_mode == 3;
  const bool binned = !gauss && la.bins > 1;
  const bool noisy = col && b < la.noiseless_from;
  const uint64_t ctr0 = (uint64_t)b * (uint64_t)(gauss ? odim : A);
  const int nD = Dp >> 4, nS = Sp >> 4, nA = Ap >> 4, nOut = lwb_pad(odim) >> 4;
  const int vo = 16 * g;  // byte offset of this lane's four rows in a padded fp32 vector
  const char* envp = lwb_smem;
  const char* laneA = envp + ev.At + n * pitchA + g * 8;
  const char* laneB = envp + ev.Bt + n * pitchB + g * 16;
  float* strip = reinterpret_cast<float*>(region + (W.strip_off < 0 ? 0 : W.strip_off)) +
                 n * LWB_STRIP_P;

  for (int step = 1; step <= W.n_steps; ++step) {
    if (__ballot(alive) == 0) break;
    // ---- observation: loco_build_obs's expression, division and clamp
    // included, goal-relative rows S and S + 1 from the current position
    lwb_f32x4 x[LWB_T];
#pragma unroll
    for (int t = 0; t < LWB_T; ++t) {
      x[t] = lwb_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      if (t < nD) {
        const lwb_f32x4 mean = lwb_ld4(envp + ev.mean + 64 * t + vo);
        const lwb_f32x4 sd = lwb_ld4(envp + ev.std + 64 * t + vo);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 16 * t + 4 * g + r;
          float raw = s[t][r];
          if (la.goal) {
            if (i == S) raw = (st.gx - st.px) * 0.1f;
            if (i == S + 1) raw = (st.gy - st.py) * 0.1f;
          }
          x[t][r] = fclampf((raw - mean[r]) / sd[r], -la.ob_clip, la.ob_clip);
        }
      }
    }
    // ---- forward: bias and tanh as mlp_layers applies them
    for (int l = 0; l < sh.n_layers; ++l) {
      const int nTi = lwb_pad(sh.dims[l]) >> 4, nTo = lwb_pad(sh.dims[l + 1]) >> 4;
      const int pitch = lwb_pitch(sh.dims[l], (int)sizeof(WT));
      lwb_f32x4 acc[LWB_T];
#pragma unroll
      for (int T = 0; T < LWB_T; ++T) acc[T] = lwb_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      lwb_product<WT>(region + W.woff[l] + n * pitch + g * 4 * (int)sizeof(WT), pitch, nTi,
                      nTo, x, acc);
      const char* bp = region + W.boff[l] + vo;
#pragma unroll
      for (int T = 0; T < LWB_T; ++T) {
        x[T] = lwb_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (T < nTo) {
          const lwb_f32x4 bias = lwb_ld4(bp + 64 * T);
#pragma unroll
          for (int r = 0; r < 4; ++r) x[T][r] = tanhf(bias[r] + acc[T][r]);
        }
      }
    }
    // ---- action: loco_wave_decode's four modes per column with its tie rule,
    // its noise keys and counters (lane there = action k here, b the
    // column's slot); rows behind A are 0
    if (gauss || binned) {
      lwb_wave_sync();  // the previous step's reads are done
#pragma unroll
      for (int T = 0; T < LWB_T; ++T)
        if (T < nOut) *reinterpret_cast<lwb_f32x4*>(strip + 16 * T + 4 * g) = x[T];
      lwb_wave_sync();
    }
    const uint64_t seed = seed0 + (uint64_t)(W.salt_base + step);
    lwb_f32x4 a[LWB_T];
#pragma unroll
    for (int t = 0; t < LWB_T; ++t) {
      a[t] = lwb_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      if (t < nA) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = 16 * t + 4 * g + r, kc = min(k, A - 1);
          float v, sd;
          if (gauss) {
            v = la.act_mode == 2 ? strip[1 + kc] : strip[kc];
            sd = la.act_mode == 2 ? strip[0] : fabsf(strip[A + kc]);
          } else if (binned) {
            int best = 0;
            float bv = strip[kc * la.bins];
            for (int j = 1; j < la.bins; ++j) {
              const float q = strip[kc * la.bins + j];
              if (q > bv) { bv = q; best = j; }
            }
            v = -1.0f + 2.0f * (float)best / (float)(la.bins - 1);
            sd = 0.0f;
          } else {
            v = x[t][r];
            sd = ac_std;
          }
          if (noisy && k < A && sd != 0.0f) v += sd * es_actnoise(seed, ctr0 + (uint64_t)k);
          a[t][r] = k < A ? fclampf(v, -1.0f, 1.0f) : 0.0f;
        }
      }
    }
    // ---- dynamics: pre = A^T s + B^T a, then b0, tanh and the leak
    lwb_f32x4 acc[LWB_T];
#pragma unroll
    for (int T = 0; T < LWB_T; ++T) acc[T] = lwb_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    lwb_product<uint16_t>(laneA, pitchA, nS, nS, s, acc);
    lwb_product<float>(laneB, pitchB, nA, nS, a, acc);
    {
#pragma clang fp contract(off)
      float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f, p3 = 0.0f;
#pragma unroll
      for (int T = 0; T < LWB_T; ++T) {
        if (T < nS) {
          const lwb_f32x4 b0 = lwb_ld4(envp + ev.b0 + 64 * T + vo);
          const lwb_f32x4 wv = lwb_ld4(envp + ev.wv + 64 * T + vo);
          const lwb_f32x4 wy = lwb_ld4(envp + ev.wy + 64 * T + vo);
          const lwb_f32x4 wh = lwb_ld4(envp + ev.wh + 64 * T + vo);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float sn = (1.0f - la.leak) * s[T][r] + la.leak * tanhf(b0[r] + acc[T][r]);
            p0 = fmaf(sn, wv[r], p0);
            p1 = fmaf(sn, wy[r], p1);
            p2 = fmaf(sn, wh[r], p2);
            s[T][r] = alive ? sn : s[T][r];
          }
        }
      }
#pragma unroll
      for (int t = 0; t < LWB_T; ++t) {
        if (t < nA) {
          const lwb_f32x4 wa = lwb_ld4(envp + ev.wa + 64 * t + vo);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            p0 = fmaf(0.5f * a[t][r], wa[r], p0);
            p3 = fmaf(a[t][r], a[t][r], p3);
          }
        }
      }
      // the four lane groups of a column end on the same bits
#pragma unroll
      for (int off = 16; off < 64; off <<= 1) {
        p0 += __shfl_xor(p0, off, 64);
        p1 += __shfl_xor(p1, off, 64);
        p2 += __shfl_xor(p2, off, 64);
        p3 += __shfl_xor(p3, off, 64);
      }
      // ---- bookkeeping of a live column; a dead one keeps what it owns
      LocoWaveSlot nw = st;
      const bool done = loco_wave_book(la, nw, p0, p1, p2, p3);
      if (alive) st = nw;
      // the column was alive before the step: its moments take the new
      // observation, goal-relative rows from the new position
      const float rel0 = (st.gx - st.px) * 0.1f, rel1 = (st.gy - st.py) * 0.1f;
#pragma unroll
      for (int t = 0; t < LWB_T; ++t) {
        if (t < nD) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = 16 * t + 4 * g + r;
            float ob = s[t][r];
            if (la.goal) {
              if (i == S) ob = rel0;
              if (i == S + 1) ob = rel1;
            }
            ms[t][r] = alive ? ms[t][r] + ob : ms[t][r];
            mq[t][r] = alive ? mq[t][r] + ob * ob : mq[t][r];
          }
        }
      }
      alive = alive && !done;
    }
  }

  // ---- written once, for the columns that entered alive; behv is the
  // position of the last step the slot took alive
  if (!entered) return;
#pragma unroll
  for (int t = 0; t < LWB_T; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 16 * t + 4 * g + r;
      if (i < S) P.s_glob[(int64_t)b * S + i] = s[t][r];
      if (i < D) {
        P.mo_sum[(int64_t)b * D + i] = ms[t][r];
        P.mo_sumsq[(int64_t)b * D + i] = mq[t][r];
      }
    }
  if (g == 0) {
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

// one template, named per weight type in the resource table and the profiles.
// The body is a function of its own: written into the kernel, which carries
// the target attribute, the header functions it calls (__ballot, __shfl_xor,
// __syncthreads) would not be inlined into it.
template <typename WT>
__global__ void __launch_bounds__(256) CLW_KERNEL_ATTR
loco_wave_batch_episode_kernel(LocoWaveBatchArgs W) {
  loco_wave_batch_episode_body<WT>(W);
}

// ---- host side --------------------------------------------------------------
// The coverage, the one place it is decided: 0 and the geometry of W, or -118.
static int loco_wave_batch_geometry(const MlpShape& sh, int S, int A, int eps, bool f32,
                                    LocoWaveBatchArgs* W) {
  if (eps < 1 || eps > LWB_MAXE || S < 1 || S > WAVE_MAXW || A < 1 || A > WAVE_MAXW)
    return -118;
  for (int l = 0; l <= sh.n_layers; ++l)
    if (sh.dims[l] < 1 || sh.dims[l] > WAVE_MAXW) return -118;
  const int esz = f32 ? 4 : 2;
  int off = 0;
  for (int l = 0; l < sh.n_layers; ++l) {
    const int Op = lwb_pad(sh.dims[l + 1]);
    W->woff[l] = off;
    off += Op * lwb_pitch(sh.dims[l], esz);
    W->boff[l] = off;
    off += Op * 4;
  }
  // the plain head decodes in registers; every other head is wider than A
  W->strip_off = sh.dims[sh.n_layers] != A ? off : -1;
  if (W->strip_off >= 0) off += LWB_STRIP_BYTES;
  W->region_bytes = off;
  W->env_bytes = lwb_env_carve(S, A, sh.dims[0]).bytes;
  W->mpb = wave_regions_per_block(W->region_bytes, W->env_bytes);
  return W->mpb < 0 ? -118 : 0;
}

static int loco_wave_batch_launch(bool f32, const LocoLaunch& L, int32_t n_steps,
                                  int32_t member_base, int32_t n_members, int32_t salt_base,
                                  int32_t wrow0, int32_t eps, void* stream) {
  LocoWaveBatchArgs W;
  W.sh = L.sh; W.la = L.la; W.P = L.P;
  W.la.wrow0 = wrow0;
  const int rc = loco_wave_batch_geometry(W.sh, W.la.S, W.la.A, eps, f32, &W);
  if (rc) return rc;
  if (member_base < 0 || member_base % eps || (n_members > 0 && n_members % eps)) return -118;
  if (n_steps <= 0 || n_members <= 0) return 0;
  W.member_base = member_base; W.n_members = n_members;
  W.n_steps = n_steps; W.salt_base = salt_base;
  const int members = n_members / eps;
  const dim3 grid((unsigned)((members + W.mpb - 1) / W.mpb)), block(64 * WAVE_WAVES);
  const unsigned lds = (unsigned)(W.env_bytes + W.mpb * W.region_bytes);
  if (f32)
    loco_wave_batch_episode_kernel<float><<<grid, block, lds, (hipStream_t)stream>>>(W);
  else
    loco_wave_batch_episode_kernel<uint16_t><<<grid, block, lds, (hipStream_t)stream>>>(W);
  ES_CHECK_LAUNCH();
  return 0;
}

// What a launch with this net, env and eps would return for the shapes alone
// (0, one of mlp_shape_init's codes, -103, -104 or -118), without launching.
extern "C" int es_loco_wave_batch_check(const int32_t* dims_host, int32_t ndims,
                                        int64_t row_stride, int32_t sdim, int32_t adim,
                                        int32_t goal_flag, int32_t f32, int32_t eps) {
  MlpShape sh;
  int rc = mlp_shape_init(&sh, dims_host, ndims, row_stride);
  if (rc) return rc;
  if (adim > 64 || sdim > ES_MAXDIM) return -103;
  if (sh.dims[0] != sdim + (goal_flag ? 2 : 0)) return -104;
  LocoWaveBatchArgs W;
  return loco_wave_batch_geometry(sh, sdim, adim, eps, f32 != 0, &W);
}

// es_loco_batch_episode's argument list and contract: eps is also the number
// of columns of a wave, member_base and n_members (slots) are multiples of
// it. n_steps <= 0 or n_members <= 0 is a no-op returning 0.
#define LOCO_WAVE_BATCH_ENTRY(NAME, F32)                                                  \
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
              : loco_wave_batch_launch(F32, L, n_steps, member_base, n_members,           \
                                       salt_base, wrow0, eps, stream);                    \
  }

LOCO_WAVE_BATCH_ENTRY(es_loco_wave_batch_episode, false)
LOCO_WAVE_BATCH_ENTRY(es_loco_wave_batch_episode_f32, true)
