// Shared device-side MLP forward core, used by the standalone forward kernel
// (mlp_fwd.hip) and the fused rollout-step kernel (rollout_loco.hip).
//
// Scheme (HBM-bandwidth-driven, guide §2/G13): per layer, thread t owns
// output octet oi = t % (O/8) and i-partition ip = t / (O/8); per i it loads
// W^T[i][8*oi..+7] as one 16-B uint4 (1 KiB per wave-instruction) and FMAs
// into 8 independent accumulator chains; partials reduce across i-partitions
// through LDS; bias + tanh in the epilogue. Non-8-aligned layers (the tiny
// action head) take a scalar fallback. mlp_layers_f32 is the fp32-weights
// counterpart (quads of float instead of octets of bf16).
#pragma once
#include "common.h"

#define ES_MAXL 8
#define ES_MAXDIM 2048

// Batch depth of the scalar-layer walks (es_walk_batched; the 256->17 action
// head runs there): that many rows' weight loads issue into registers before
// the first FMA of the batch, instead of the one load + s_waitcnt vmcnt(0)
// per row that hipcc emits for a plain loop (every trip a fully exposed
// memory round trip on a path all waves execute, with a barrier behind it).
// The flagship head is 18/17 trips per thread -> 3 waits instead of 18.
#define ES_HEAD_BT 8

typedef uint32_t es_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint4 es_as_uint4(es_u32x4 v) {
  uint4 w;
  w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w;
  return w;
}

// 16-B non-temporal load (the builtin wants an ext vector; HIP's uint4 is a
// struct). For rows that exactly one block reads per step: it keeps them out
// of L2 so the streams the whole grid shares stay resident.
__device__ __forceinline__ uint4 es_ld16_nt(const void* p) {
  return es_as_uint4(__builtin_nontemporal_load(reinterpret_cast<const es_u32x4*>(p)));
}

// Row-strided 16-B stream: thread reads bytes [lane, lane+16) of rows
// row0 + k*rstep (k = 0, 1, ...) of a matrix with `rbytes` bytes per row.
// Addressing is base + (int64)row * stride per lane, which the compiler
// strength-reduces inside the ring loops to one 64-bit per-lane pointer per
// stream and uniform steps (no v_mad_i64_i32 left in the loops). The
// scalar-base form of global_load (wave-uniform 64-bit base + 32-bit
// per-lane offset) was measured 2% slower on the flagship and is gone;
// the runs are in profiles/README.md, round 4.
struct EsRowStream {
  const char* lb;  // per-lane column base
  int row, rstep;
  int64_t rbytes;
  __device__ __forceinline__ EsRowStream(const void* base, int row0, int rstep_,
                                         int rbytes_, int lane_bytes)
      : lb(reinterpret_cast<const char*>(base) + lane_bytes),
        row(row0), rstep(rstep_), rbytes(rbytes_) {}
  __device__ __forceinline__ const char* at(int k) const {
    return lb + (int64_t)(row + k * rstep) * rbytes;
  }
  __device__ __forceinline__ void advance(int k) { row += k * rstep; }
  __device__ __forceinline__ es_u32x4 ld(int k) const {
    return *reinterpret_cast<const es_u32x4*>(at(k));
  }
  __device__ __forceinline__ es_u32x4 ld_nt(int k) const {
    return __builtin_nontemporal_load(reinterpret_cast<const es_u32x4*>(at(k)));
  }
};

// Guarded drain of es_walk_batched: R rows every thread owns, then the one
// row only some threads own. All R + 1 loads issue ahead of the first FMA;
// the conditional row's load is clamped to row 0 where the thread has none.
template <int R, typename W, typename LD, typename FMA>
__device__ __forceinline__ void es_walk_drain(int r0, int st, int I, LD ld, FMA fma) {
  W w[R + 1];
  const int rl = r0 + R * st;
  const bool ok = rl < I;
#pragma unroll
  for (int u = 0; u < R; ++u) w[u] = ld(r0 + u * st);
  w[R] = ld(ok ? rl : 0);
#pragma unroll
  for (int u = 0; u < R; ++u) fma(w[u], r0 + u * st);
  if (ok) fma(w[R], rl);
}

// Batched strided row walk r = i0, i0 + st, ... < I for the scalar layers.
// st and I are block-uniform and 0 <= i0 < st, so with T = ceil(I / st) every
// thread owns trips 0..T-2 and only trip T-1 depends on the thread. The
// T-1 common trips run in straight-line batches of ES_HEAD_BT loads followed
// by ES_HEAD_BT FMAs (uniform control flow, nothing for the compiler to sink
// behind a wait); the remainder and the conditional trip drain together.
template <typename W, typename LD, typename FMA>
__device__ __forceinline__ void es_walk_batched(int i0, int st, int I, LD ld, FMA fma) {
  const int T = (I + st - 1) / st;
  int t = 0;
  for (; t + ES_HEAD_BT <= T - 1; t += ES_HEAD_BT) {
    W w[ES_HEAD_BT];
#pragma unroll
    for (int u = 0; u < ES_HEAD_BT; ++u) w[u] = ld(i0 + (t + u) * st);
#pragma unroll
    for (int u = 0; u < ES_HEAD_BT; ++u) fma(w[u], i0 + (t + u) * st);
  }
  const int r0 = i0 + t * st;
  static_assert(ES_HEAD_BT == 8, "drain switch covers remainders 0..7");
  switch (T - 1 - t) {
    case 0: es_walk_drain<0, W>(r0, st, I, ld, fma); break;
    case 1: es_walk_drain<1, W>(r0, st, I, ld, fma); break;
    case 2: es_walk_drain<2, W>(r0, st, I, ld, fma); break;
    case 3: es_walk_drain<3, W>(r0, st, I, ld, fma); break;
    case 4: es_walk_drain<4, W>(r0, st, I, ld, fma); break;
    case 5: es_walk_drain<5, W>(r0, st, I, ld, fma); break;
    case 6: es_walk_drain<6, W>(r0, st, I, ld, fma); break;
    default: es_walk_drain<7, W>(r0, st, I, ld, fma); break;
  }
}

// Strided row walk r = i0, i0 + st, ... < I as a depth-4 register double
// buffer: the NEXT block's 4 loads issue before the CURRENT block's FMAs, so
// 4-8 loads stay in flight across the loop back-edge. (hipcc alone emits one
// load + s_waitcnt vmcnt(0) per iteration, measured ~5x slower on the HBM
// weight stream; a plain 4-unroll still drains vmcnt to 0 at every back-edge,
// SQ_WAIT_ANY measured at 71% of wave cycles.) ld(row) returns the loaded
// value, whose type is ld's to choose; fma(value, row) consumes it, in
// ascending row order. Rows behind the last full block take the plain tail.
template <typename LD, typename FMA>
__device__ __forceinline__ void es_walk_ring4(int i0, int st, int I, LD ld, FMA fma) {
  int i = i0;
  if (i + 3 * st < I) {
    auto c0 = ld(i), c1 = ld(i + st), c2 = ld(i + 2 * st), c3 = ld(i + 3 * st);
    for (; i + 7 * st < I; i += 4 * st) {
      const auto n0 = ld(i + 4 * st), n1 = ld(i + 5 * st), n2 = ld(i + 6 * st),
                 n3 = ld(i + 7 * st);
      fma(c0, i);
      fma(c1, i + st);
      fma(c2, i + 2 * st);
      fma(c3, i + 3 * st);
      c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    }
    fma(c0, i);
    fma(c1, i + st);
    fma(c2, i + 2 * st);
    fma(c3, i + 3 * st);
    i += 4 * st;
  }
  for (; i < I; i += st) fma(ld(i), i);
}

struct MlpShape {
  int n_layers;
  int dims[ES_MAXL + 1];
  int64_t woff[ES_MAXL];
  int64_t boff[ES_MAXL];
  int vec_ok[ES_MAXL];
  int maxdim;  // max layer width, 4-padded — LDS activation buffer extent
};

// dynamic-LDS carve sizes (bytes, 16-B aligned each; guide §6 G17)
static inline int64_t mlp_lds_bytes(int maxdim) {
  return 2 * (int64_t)maxdim * 4 + 256 * 8 * 4;  // buf[2][maxdim] + partial
}
// the pair rollout kernels' carve (ES_LOCO_PAIR_CARVE): per member the two
// activation buffers, a partial slab, the raw state (4-padded) and 64 actions
static inline int64_t mlp_pair_lds_bytes(int maxdim, int sdim) {
  return 2 * (mlp_lds_bytes(maxdim) + (((int64_t)sdim + 3) & ~3) * 4 + 64 * 4);
}

// Host-side shape builder; returns 0 on success.
static inline int mlp_shape_init(MlpShape* sh, const int32_t* dims_host, int32_t ndims,
                                 int64_t row_stride) {
  if (ndims < 2 || ndims > ES_MAXL + 1) return -100;
  sh->n_layers = ndims - 1;
  int64_t off = 0;
  sh->maxdim = 0;
  for (int l = 0; l < ndims; ++l) {
    sh->dims[l] = dims_host[l];
    if (dims_host[l] > ES_MAXDIM) return -101;
    if (dims_host[l] > sh->maxdim) sh->maxdim = dims_host[l];
  }
  sh->maxdim = (sh->maxdim + 3) & ~3;
  for (int l = 0; l < sh->n_layers; ++l) {
    sh->woff[l] = off;
    off += (int64_t)sh->dims[l] * sh->dims[l + 1];
    sh->boff[l] = off;
    off += sh->dims[l + 1];
    const int O = sh->dims[l + 1];
    sh->vec_ok[l] = (O % 8 == 0) && (O <= 8 * 256) && (sh->woff[l] % 8 == 0);
  }
  if (off > row_stride) return -102;
  return 0;
}

__device__ __forceinline__ void bf8_fma(uint4 w, const float xi, float* acc) {
  const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    acc[2 * q] = fmaf(bf2f((uint16_t)(ws[q] & 0xFFFFu)), xi, acc[2 * q]);
    acc[2 * q + 1] = fmaf(bf2f((uint16_t)(ws[q] >> 16)), xi, acc[2 * q + 1]);
  }
}

// bf8_fma on accumulator PAIRS: acc2[q] = (acc[2q], acc[2q+1]). The same
// eight fmaf, written as four two-lane fmas so the packed form does not hang
// on the vectorizer finding it (which also re-orders the block to do so).
__device__ __forceinline__ void bf8_fma_pk(es_u32x4 w, float xi, es_f32x2* acc2) {
  const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
  const es_f32x2 x2 = {xi, xi};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const es_f32x2 w2 = {__builtin_bit_cast(float, ws[q] << 16),
                         __builtin_bit_cast(float, ws[q] & 0xFFFF0000u)};
    acc2[q] = __builtin_elementwise_fma(w2, x2, acc2[q]);
  }
}

// Runs every layer; input in bufA; returns the pointer holding the final
// output (bufA or bufB). `partial` is a 256*8-float LDS scratch.
__device__ __forceinline__ float* mlp_layers(const uint16_t* __restrict__ wb,
                                             const MlpShape& sh,
                                             float* bufA, float* bufB, float* partial,
                                             int tid, int nthreads, int act_final) {
  float* x = bufA;
  float* y = bufB;
  for (int l = 0; l < sh.n_layers; ++l) {
    const int I = sh.dims[l], O = sh.dims[l + 1];
    const uint16_t* Wt = wb + sh.woff[l];
    const uint16_t* Bs = wb + sh.boff[l];
    const bool do_act = (l < sh.n_layers - 1) || act_final;

    if (sh.vec_ok[l]) {
      const int OCT = O >> 3;
      const int PART = nthreads / OCT;
      const int oi = tid % OCT, ip = tid / OCT;
      float acc[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] = 0.0f;
      if (ip < PART) {
        const uint16_t* wcol = Wt + (oi << 3);
        // depth 4: depth 8 raised VGPRs to 111 and cost a resident block per
        // CU, measured net negative. nt: each member's weights are read by
        // exactly one CU per step.
        es_walk_ring4(
            ip, PART, I, [&](int i) { return es_ld16_nt(wcol + (int64_t)i * O); },
            [&](const uint4& w, int i) { bf8_fma(w, x[i], acc); });
#pragma unroll
        for (int q = 0; q < 8; ++q) partial[(ip * OCT + oi) * 8 + q] = acc[q];
      }
      __syncthreads();
      for (int o = tid; o < O; o += nthreads) {
        float s = bf2f(Bs[o]);
        const int oo = o >> 3, j = o & 7;
        for (int p = 0; p < PART; ++p) s += partial[(p * OCT + oo) * 8 + j];
        y[o] = do_act ? tanhf(s) : s;
      }
    } else {
      // tiled scalar path (small / odd layers, e.g. the 256->17 action head):
      // thread owns (output o, i-partition ip) so the whole block shares the
      // I-dim walk — a thread-per-output loop leaves O threads issuing I
      // serial HBM-latency loads each (measured: the action head dominated
      // the fused step kernel that way).
      const int PART = nthreads / O;
      if (PART > 1) {
        const int oi = tid % O, ip = tid / O;
        float acc = 0.0f;
        if (ip < PART) {
          es_walk_batched<uint16_t>(
              ip, PART, I, [&](int r) { return Wt[(int64_t)r * O + oi]; },
              [&](uint16_t w, int r) { acc = fmaf(bf2f(w), x[r], acc); });
          partial[ip * O + oi] = acc;
        }
        __syncthreads();
        for (int o = tid; o < O; o += nthreads) {
          float s = bf2f(Bs[o]);
          for (int p = 0; p < PART; ++p) s += partial[p * O + o];
          y[o] = do_act ? tanhf(s) : s;
        }
      } else {
        for (int o = tid; o < O; o += nthreads) {
          float acc = bf2f(Bs[o]);
          es_walk_batched<uint16_t>(
              0, 1, I, [&](int r) { return Wt[(int64_t)r * O + o]; },
              [&](uint16_t w, int r) { acc = fmaf(bf2f(w), x[r], acc); });
          y[o] = do_act ? tanhf(acc) : acc;
        }
      }
    }
    __syncthreads();
    float* t = x;
    x = y;
    y = t;
  }
  return x;
}

// ---- fp32-weights forward ---------------------------------------------------
// weights_dtype = "fp32": the member rows hold float32(theta + s*eps) and the
// forward accumulates them with fp32 fmaf, so the only difference from the
// reference's fp32 forward is summation order. Same per-layer scheme as
// mlp_layers (partition the i-walk, reduce partials through LDS, bias + tanh
// in the epilogue).
//
// Tiling: QUADS. A thread owns 4 outputs and issues ONE 16-B load per row:
// the same 16 B per lane / 1 KiB per wave-instruction as the bf16 octet, and
// the same register footprint at pipeline depth 4 (8 x 16 B in flight + 4
// accumulators instead of 8). Octets with two loads per row would keep the
// (PART, OCT, 8) partial layout but double the live load registers (64
// VGPRs of weights at depth 4) for no extra bytes per wave-instruction. With
// quads QT = O/4 tiles and PART = nthreads / QT i-partitions; the partial
// layout (ip, o) is PART x O floats. A layer wider than 4 * nthreads
// (QT > nthreads, e.g. O = 2048 at 256 threads) runs PART = 1 and each
// thread sweeps tiles tid, tid + nthreads, ...; the partial slab is then O
// <= ES_MAXDIM floats, which is exactly the 256*8 floats every caller carves.
//
// A layer is quad-tiled when O % 4 == 0 and its weight block AND the member
// row are 16-B aligned (woff % 4 == 0, row_stride % 4 == 0); everything else
// takes the scalar walks, so no vector load can be misaligned. Every load is
// guarded by its own row index < I: the blob has no guard row and needs none.
static inline void mlp_shape_vec_f32(MlpShape* sh, int64_t row_stride) {
  for (int l = 0; l < sh->n_layers; ++l)
    sh->vec_ok[l] = (sh->dims[l + 1] % 4 == 0) && (sh->woff[l] % 4 == 0) &&
                    (row_stride % 4 == 0);
}

__device__ __forceinline__ void f4_fma(uint4 w, const float xi, float* acc) {
  acc[0] = fmaf(__uint_as_float(w.x), xi, acc[0]);
  acc[1] = fmaf(__uint_as_float(w.y), xi, acc[1]);
  acc[2] = fmaf(__uint_as_float(w.z), xi, acc[2]);
  acc[3] = fmaf(__uint_as_float(w.w), xi, acc[3]);
}

__device__ __forceinline__ float* mlp_layers_f32(const float* __restrict__ wb,
                                                 const MlpShape& sh,
                                                 float* bufA, float* bufB, float* partial,
                                                 int tid, int nthreads, int act_final) {
  float* x = bufA;
  float* y = bufB;
  for (int l = 0; l < sh.n_layers; ++l) {
    const int I = sh.dims[l], O = sh.dims[l + 1];
    const float* Wt = wb + sh.woff[l];
    const float* Bs = wb + sh.boff[l];
    const bool do_act = (l < sh.n_layers - 1) || act_final;

    if (sh.vec_ok[l]) {
      const int QT = O >> 2;
      const bool wide = QT > nthreads;  // block-uniform
      const int PART = wide ? 1 : nthreads / QT;
      const int ip = wide ? 0 : tid / QT;
      if (ip < PART) {
        for (int oi = wide ? tid : tid % QT; oi < QT; oi += nthreads) {
          float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
          const float* wcol = Wt + (oi << 2);
          // nt 16-B loads, depth-4 walk as in mlp_layers. The quad is
          // carried as four u32 lanes exactly like the bf16 octet: with a
          // float4-typed carried value the optimizer folds the loop-carried
          // phi(prologue load, next load) back into ONE load at the loop
          // head, i.e. load 4 -> wait -> FMA per trip with nothing in flight
          // across the back-edge (seen in the ISA). Hence es_walk_ring4
          // takes its value type from ld.
          es_walk_ring4(
              ip, PART, I, [&](int i) { return es_ld16_nt(wcol + (int64_t)i * O); },
              [&](const uint4& w, int i) { f4_fma(w, x[i], acc); });
#pragma unroll
          for (int q = 0; q < 4; ++q) partial[ip * O + (oi << 2) + q] = acc[q];
        }  // one trip unless wide: oi + nthreads >= QT
      }
      __syncthreads();
      for (int o = tid; o < O; o += nthreads) {
        float s = Bs[o];
        for (int p = 0; p < PART; ++p) s += partial[p * O + o];
        y[o] = do_act ? tanhf(s) : s;
      }
    } else {
      // scalar layers (the action head, odd widths, misaligned blocks): the
      // batched row walk of mlp_layers with W = float
      const int PART = nthreads / O;
      if (PART > 1) {
        const int oi = tid % O, ip = tid / O;
        float acc = 0.0f;
        if (ip < PART) {
          es_walk_batched<float>(
              ip, PART, I, [&](int r) { return Wt[(int64_t)r * O + oi]; },
              [&](float w, int r) { acc = fmaf(w, x[r], acc); });
          partial[ip * O + oi] = acc;
        }
        __syncthreads();
        for (int o = tid; o < O; o += nthreads) {
          float s = Bs[o];
          for (int p = 0; p < PART; ++p) s += partial[p * O + o];
          y[o] = do_act ? tanhf(s) : s;
        }
      } else {
        for (int o = tid; o < O; o += nthreads) {
          float acc = Bs[o];
          es_walk_batched<float>(
              0, 1, I, [&](int r) { return Wt[(int64_t)r * O + o]; },
              [&](float w, int r) { acc = fmaf(w, x[r], acc); });
          y[o] = do_act ? tanhf(acc) : acc;
        }
      }
    }
    __syncthreads();
    float* t = x;
    x = y;
    y = t;
  }
  return x;
}

// one row's (theta, sigma*eps) scalar pair as loaded by the batched walks
struct EsTE8 { uint16_t t; uint8_t e; };
struct EsTE16 { uint16_t t; uint16_t e; };

// theta octet (bf16) +- decoded fp8 eps octet, FMA'd into both members
__device__ __forceinline__ void bf8e_fma_pair(uint4 t, const float* e8, float xp,
                                              float xm, float* accp, float* accm) {
  const uint32_t ts[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float t0 = bf2f((uint16_t)(ts[q] & 0xFFFFu));
    const float t1 = bf2f((uint16_t)(ts[q] >> 16));
    accp[2 * q] = fmaf(t0 + e8[2 * q], xp, accp[2 * q]);
    accm[2 * q] = fmaf(t0 - e8[2 * q], xm, accm[2 * q]);
    accp[2 * q + 1] = fmaf(t1 + e8[2 * q + 1], xp, accp[2 * q + 1]);
    accm[2 * q + 1] = fmaf(t1 - e8[2 * q + 1], xm, accm[2 * q + 1]);
  }
}

// bf8e_fma_pair on accumulator PAIRS (see bf8_fma_pk): theta octet (bf16)
// +- the eps octet held as two fp8x4 words, FMA'd into both members. Lane
// for lane the same t+e / t-e roundings and fmaf as bf8e_fma_pair after
// fp8x4_decode(elo), fp8x4_decode(ehi).
__device__ __forceinline__ void bf8e_fma_pair_pk(es_u32x4 t, uint32_t elo, uint32_t ehi,
                                                 float xp, float xm, es_f32x2* ap,
                                                 es_f32x2* am) {
  const uint32_t ts[4] = {t.x, t.y, t.z, t.w};
  const es_f32x2 e2[4] = {__builtin_amdgcn_cvt_pk_f32_fp8(elo, false),
                          __builtin_amdgcn_cvt_pk_f32_fp8(elo, true),
                          __builtin_amdgcn_cvt_pk_f32_fp8(ehi, false),
                          __builtin_amdgcn_cvt_pk_f32_fp8(ehi, true)};
  const es_f32x2 xp2 = {xp, xp}, xm2 = {xm, xm};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const es_f32x2 t2 = {__builtin_bit_cast(float, ts[q] << 16),
                         __builtin_bit_cast(float, ts[q] & 0xFFFF0000u)};
    ap[q] = __builtin_elementwise_fma(t2 + e2[q], xp2, ap[q]);
    am[q] = __builtin_elementwise_fma(t2 - e2[q], xm2, am[q]);
  }
}

// The scalar layer of mlp_layers_pair_fp8 on weights staged in LDS (Tl bf16
// theta, El fp8 eps, element-ordered): its two arms, PART > 1 and PART == 1,
// statement for statement. A copy and not a shared lambda or template: every
// form of sharing tried moved the register allocation of the per-step kernel,
// whose assembly a staged level must leave alone; and the pointer's address
// space has to be fixed at compile time (a run-time choice between LDS and
// global gives a generic pointer and flat loads).
template <typename BIAS>
__device__ __forceinline__ void mlp_pair_fp8_scalar_staged(
    const uint16_t* Tl, const uint8_t* El, int I, int O, const float* xp,
    const float* xm, float* yp, float* ym, float* partial, float* partm, int tid,
    int nthreads, bool do_act, BIAS bias_pm) {
  const int PART = nthreads / O;
  if (PART > 1) {
    const int oi = tid % O, ip = tid / O;
    float accp = 0.0f, accm = 0.0f;
    if (ip < PART) {
      es_walk_batched<EsTE8>(
          ip, PART, I, [&](int r) { return EsTE8{Tl[r * O + oi], El[r * O + oi]}; },
          [&](EsTE8 w, int r) {
            const float tw = bf2f(w.t), ew = fp8_byte(w.e);
            accp = fmaf(tw + ew, xp[r], accp);
            accm = fmaf(tw - ew, xm[r], accm);
          });
      partial[ip * O + oi] = accp;
      partm[ip * O + oi] = accm;
    }
    __syncthreads();
    for (int o = tid; o < O; o += nthreads) {
      float sp, sm;
      bias_pm(o, sp, sm);
      for (int p = 0; p < PART; ++p) {
        sp += partial[p * O + o];
        sm += partm[p * O + o];
      }
      yp[o] = do_act ? tanhf(sp) : sp;
      ym[o] = do_act ? tanhf(sm) : sm;
    }
  } else {
    for (int o = tid; o < O; o += nthreads) {
      float accp, accm;
      bias_pm(o, accp, accm);
      es_walk_batched<EsTE8>(
          0, 1, I, [&](int r) { return EsTE8{Tl[r * O + o], El[r * O + o]}; },
          [&](EsTE8 w, int r) {
            const float tw = bf2f(w.t), ew = fp8_byte(w.e);
            accp = fmaf(tw + ew, xp[r], accp);
            accm = fmaf(tw - ew, xm[r], accm);
          });
      yp[o] = do_act ? tanhf(accp) : accp;
      ym[o] = do_act ? tanhf(accm) : accm;
    }
  }
}

// mlp_layers_pair with an fp8 (OCP e4m3fn) sigma*eps blob: one nt 16-B load
// covers one octet of TWO consecutive i-rows (pheno_fp8_kernel's row-pair
// interleave), halving both the bytes and the load count of the HBM eps
// stream; theta stays bf16 (L2-resident). Same (oi, ip) tiling; the i-walk
// is by row PAIRS, so the per-thread accumulation partition differs from
// the bf16 path (documented; the fp8 path is new numerics regardless).
//
// STAGE (multi-step kernel, whose theta/eps rows cannot change during a
// launch): the caller holds copies of small operands in LDS, filled once per
// launch by mlp_pair_fp8_stage_fill, and the layers read them there instead
// of taking a global round trip behind each layer's barrier.
//   >= 1: sbias = every layer's bias start values, (tB + eB, tB - eB) per
//         output, layer after layer;
//   >= 2: the last layer's weights when it is on the scalar path (block-
//         uniform `head_staged`): sht = its bf16 theta, she = its fp8 eps,
//         element-ordered as in the blob.
// Same values, same order of operations: outputs are those of STAGE 0.
template <int STAGE = 0>
__device__ __forceinline__ void mlp_layers_pair_fp8(
    const uint16_t* __restrict__ tb, const uint8_t* __restrict__ eb8,
    const MlpShape& sh, float* bufAp, float* bufAm, float* bufBp, float* bufBm,
    float* partial, int tid, int nthreads, int act_final,
    float** xp_out, float** xm_out, const float* sbias = nullptr,
    const uint16_t* sht = nullptr, const uint8_t* she = nullptr,
    bool head_staged = false) {
  float* xp = bufAp;
  float* xm = bufAm;
  float* yp = bufBp;
  float* ym = bufBm;
  float* partm = partial + 256 * 8;
  for (int l = 0; l < sh.n_layers; ++l) {
    const int I = sh.dims[l], O = sh.dims[l + 1];
    const uint16_t* Tt = tb + sh.woff[l];
    const uint8_t* Et8 = eb8 + sh.woff[l];
    const uint16_t* TBs = tb + sh.boff[l];
    const uint8_t* EBs8 = eb8 + sh.boff[l];
    const bool do_act = (l < sh.n_layers - 1) || act_final;
    // start values of output o's two sums
    auto bias_pm = [&](int o, float& sp, float& sm) {
      if constexpr (STAGE >= 1) {
        sp = sbias[2 * o];
        sm = sbias[2 * o + 1];
      } else {
        const float tB = bf2f(TBs[o]), eB = fp8_byte(EBs8[o]);
        sp = tB + eB;
        sm = tB - eB;
      }
    };

    if (sh.vec_ok[l]) {
      const int OCT = O >> 3;
      const int PART = nthreads / OCT;
      const int oi = tid % OCT, ip = tid / OCT;
      float accp[8], accm[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) accp[q] = accm[q] = 0.0f;
      if (ip < PART) {
        const int ro = I & 1;            // odd input dim: row 0 stays plain
        const int I2 = (I - ro) >> 1;    // row pairs (rows ro..I-1)
        const int rs2 = 2 * O;           // bytes per row pair
        const uint16_t* tcol = Tt + (oi << 3);
        const uint8_t* ecol8 = Et8 + (int64_t)ro * O + (oi << 4);
        auto lde8 = [&](int i2) {  // 16 fp8 = octet of rows 2*i2, 2*i2+1
          return es_ld16_nt(ecol8 + (int64_t)i2 * rs2);
        };
        auto ldt = [&](int r) {
          return *reinterpret_cast<const uint4*>(tcol + (int64_t)r * O);
        };
        auto fma_pairblk = [&](const uint4& e16, const uint4& ta, const uint4& tb_,
                               int r0) {
          float e8[8];
          fp8x4_decode(e16.x, e8);
          fp8x4_decode(e16.y, e8 + 4);
          bf8e_fma_pair(ta, e8, xp[r0], xm[r0], accp, accm);
          fp8x4_decode(e16.z, e8);
          fp8x4_decode(e16.w, e8 + 4);
          bf8e_fma_pair(tb_, e8, xp[r0 + 1], xm[r0 + 1], accp, accm);
        };
        if (ro && ip == 0) {
          // row 0 (plain element-ordered fp8): every oi-octet lane of the
          // ip==0 partition consumes it so the partial layout is unchanged
          float e8[8];
          const uint8_t* p0 = Et8 + (oi << 3);
          fp8x4_decode(*reinterpret_cast<const uint32_t*>(p0), e8);
          fp8x4_decode(*reinterpret_cast<const uint32_t*>(p0 + 4), e8 + 4);
          bf8e_fma_pair(ldt(0), e8, xp[0], xm[0], accp, accm);
        }
        int i2 = ip;
        // Set ring. The loaded rows live in named register SETS that change
        // role over an unrolled loop of whole turns (here: 2 sets of 2 row
        // pairs, period 2): each sub-trip issues the loads of the free set,
        // then consumes the oldest, so there is nothing to rotate by copy
        // and a load is first waited for one sub-trip after it issues. (A
        // "next = load; consume cur; cur = next" loop compiles to a copy of
        // the just-loaded registers, hence a wait for the trip's own loads
        // at the bottom of every trip.) What it takes to make the compiler
        // keep that shape: the FMAs are written as two-lane fmas
        // (bf8e_fma_pair_pk), because the vectorizer, left to find the
        // packed form, re-orders the block and sinks a sub-trip's FMAs below
        // the next refill of their set; a sched_barrier between sub-trips;
        // one loop exit (a multi-exit loop is restructured with copies on
        // the back edge). Every lane owns nmin or nmin + 1 row pairs; the
        // turn count is the block-uniform minimum, and the 0..4 row pairs a
        // lane has left behind the held set load ahead of the drain's FMAs,
        // so no row takes a serialized tail load once the ring is in use.
        // Per-thread FMA order (ascending row into the same accumulators)
        // and the t+e / t-e roundings are those of the tail loop below. A
        // 4-wide (8-row) copy-rotated pipeline was measured and lost; the
        // numbers are in ROADMAP.md.
        const int nmin = I2 / PART;
        if (nmin >= 2) {
          const int T = (nmin - 2) >> 2;
          const int rem = (I2 - 1 - ip) / PART + 1 - 4 * T - 2;
          // one stream step = one row pair: 2*O fp8 bytes, two bf16 rows
          EsRowStream es(Et8 + (int64_t)ro * O, ip, PART, 2 * O, oi << 4);
          EsRowStream ta(Tt + (int64_t)ro * O, ip, PART, 4 * O, oi << 4);
          EsRowStream tb(Tt + (int64_t)(ro + 1) * O, ip, PART, 4 * O, oi << 4);
          const float* xqp = xp + ro + 2 * ip;
          const float* xqm = xm + ro + 2 * ip;
          es_f32x2 a2p[4], a2m[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            a2p[q] = es_f32x2{accp[2 * q], accp[2 * q + 1]};
            a2m[q] = es_f32x2{accm[2 * q], accm[2 * q + 1]};
          }
          struct Slot { es_u32x4 e, a, b; };
          auto ldslot = [&](Slot& s, int k) {
            s.e = es.ld_nt(k);
            s.a = ta.ld(k);
            s.b = tb.ld(k);
          };
          auto eatslot = [&](const Slot& s, int k) {
            const float* qp = xqp + 2 * k * PART;
            const float* qm = xqm + 2 * k * PART;
            bf8e_fma_pair_pk(s.a, s.e.x, s.e.y, qp[0], qm[0], a2p, a2m);
            bf8e_fma_pair_pk(s.b, s.e.z, s.e.w, qp[1], qm[1], a2p, a2m);
          };
          struct Set { Slot s[2]; };
          auto fill = [&](Set& w) {
            ldslot(w.s[0], 0);
            ldslot(w.s[1], 1);
            es.advance(2);
            ta.advance(2);
            tb.advance(2);
          };
          auto eat = [&](const Set& w) {
            eatslot(w.s[0], 0);
            eatslot(w.s[1], 1);
            xqp += 4 * PART;
            xqm += 4 * PART;
          };
          Set c, n;
          fill(c);
          // the fences keep a sub-trip's work out of the next one, where
          // the set it reads is refilled
          for (int t = T; t > 0; --t) {
            fill(n); eat(c);
            __builtin_amdgcn_sched_barrier(0);
            fill(c); eat(n);
            __builtin_amdgcn_sched_barrier(0);
          }
          // drain: the 0..4 row pairs left load into fresh names, each two
          // slots ahead of its FMAs, so no more is live than in the loop.
          // (Zeroed first: an undefined "not loaded" value is hoisted out
          // of the layer loop as 48 live registers.)
          Slot f[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) f[k].e = f[k].a = f[k].b = es_u32x4{0u, 0u, 0u, 0u};
#pragma unroll
          for (int k = 0; k < 2; ++k)
            if (k < rem) ldslot(f[k], k);
          __builtin_amdgcn_sched_barrier(0);
          eat(c);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            __builtin_amdgcn_sched_barrier(0);
            if (k + 2 < 4 && k + 2 < rem) ldslot(f[k + 2], k + 2);
            __builtin_amdgcn_sched_barrier(0);
            if (k < rem) eatslot(f[k], k);
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            accp[2 * q] = a2p[q].x; accp[2 * q + 1] = a2p[q].y;
            accm[2 * q] = a2m[q].x; accm[2 * q + 1] = a2m[q].y;
          }
          i2 = I2;  // every owned row pair is consumed
        }
        for (; i2 < I2; i2 += PART)
          fma_pairblk(lde8(i2), ldt(ro + 2 * i2), ldt(ro + 2 * i2 + 1), ro + 2 * i2);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          partial[(ip * OCT + oi) * 8 + q] = accp[q];
          partm[(ip * OCT + oi) * 8 + q] = accm[q];
        }
      }
      __syncthreads();
      for (int o = tid; o < O; o += nthreads) {
        float sp, sm;
        bias_pm(o, sp, sm);
        const int oo = o >> 3, j = o & 7;
        for (int p = 0; p < PART; ++p) {
          sp += partial[(p * OCT + oo) * 8 + j];
          sm += partm[(p * OCT + oo) * 8 + j];
        }
        yp[o] = do_act ? tanhf(sp) : sp;
        ym[o] = do_act ? tanhf(sm) : sm;
      }
    } else {
      // scalar path (small / odd layers): plain element-ordered fp8
      bool staged = false;
      if constexpr (STAGE >= 2) staged = head_staged && l == sh.n_layers - 1;
      const int PART = nthreads / O;
      if (staged) {
        if constexpr (STAGE >= 2)
          mlp_pair_fp8_scalar_staged(sht, she, I, O, xp, xm, yp, ym, partial, partm, tid,
                                     nthreads, do_act, bias_pm);
      } else if (PART > 1) {
        const int oi = tid % O, ip = tid / O;
        float accp = 0.0f, accm = 0.0f;
        if (ip < PART) {
          es_walk_batched<EsTE8>(
              ip, PART, I,
              [&](int r) {
                return EsTE8{Tt[(int64_t)r * O + oi], Et8[(int64_t)r * O + oi]};
              },
              [&](EsTE8 w, int r) {
                const float tw = bf2f(w.t), ew = fp8_byte(w.e);
                accp = fmaf(tw + ew, xp[r], accp);
                accm = fmaf(tw - ew, xm[r], accm);
              });
          partial[ip * O + oi] = accp;
          partm[ip * O + oi] = accm;
        }
        __syncthreads();
        for (int o = tid; o < O; o += nthreads) {
          float sp, sm;
          bias_pm(o, sp, sm);
          for (int p = 0; p < PART; ++p) {
            sp += partial[p * O + o];
            sm += partm[p * O + o];
          }
          yp[o] = do_act ? tanhf(sp) : sp;
          ym[o] = do_act ? tanhf(sm) : sm;
        }
      } else {
        for (int o = tid; o < O; o += nthreads) {
          float accp, accm;
          bias_pm(o, accp, accm);
          es_walk_batched<EsTE8>(
              0, 1, I,
              [&](int r) {
                return EsTE8{Tt[(int64_t)r * O + o], Et8[(int64_t)r * O + o]};
              },
              [&](EsTE8 w, int r) {
                const float tw = bf2f(w.t), ew = fp8_byte(w.e);
                accp = fmaf(tw + ew, xp[r], accp);
                accm = fmaf(tw - ew, xm[r], accm);
              });
          yp[o] = do_act ? tanhf(accp) : accp;
          ym[o] = do_act ? tanhf(accm) : accm;
        }
      }
    }
    __syncthreads();
    if constexpr (STAGE >= 1) sbias += 2 * O;
    float* t = xp; xp = yp; yp = t;
    t = xm; xm = ym; ym = t;
  }
  *xp_out = xp;
  *xm_out = xm;
}

// The stage of mlp_layers_pair_fp8<STAGE>: sizes (host) and the fill (once
// per launch, every thread of the block; the caller's barrier follows).
static inline int64_t mlp_pair_fp8_bias_floats(const MlpShape& sh) {
  int64_t n = 0;
  for (int l = 0; l < sh.n_layers; ++l) n += 2 * (int64_t)sh.dims[l + 1];
  return n;
}
// elements of the last layer's weights if that layer is on the scalar path
static inline int64_t mlp_pair_fp8_head_elems(const MlpShape& sh) {
  const int l = sh.n_layers - 1;
  return sh.vec_ok[l] ? 0 : (int64_t)sh.dims[l] * sh.dims[l + 1];
}

__device__ __forceinline__ void mlp_pair_fp8_stage_fill(
    const uint16_t* __restrict__ tb, const uint8_t* __restrict__ eb8,
    const MlpShape& sh, float* sbias, uint16_t* sht, uint8_t* she, bool head_staged,
    int tid, int nthreads) {
  for (int l = 0; l < sh.n_layers; ++l) {
    const int O = sh.dims[l + 1];
    const uint16_t* TBs = tb + sh.boff[l];
    const uint8_t* EBs8 = eb8 + sh.boff[l];
    for (int o = tid; o < O; o += nthreads) {
      const float tB = bf2f(TBs[o]), eB = fp8_byte(EBs8[o]);
      sbias[2 * o] = tB + eB;
      sbias[2 * o + 1] = tB - eB;
    }
    sbias += 2 * O;
  }
  if (head_staged) {
    const int l = sh.n_layers - 1;
    const int n = sh.dims[l] * sh.dims[l + 1];
    const uint16_t* Tt = tb + sh.woff[l];
    const uint8_t* Et8 = eb8 + sh.woff[l];
    for (int k = tid; k < n; k += nthreads) {
      sht[k] = Tt[k];
      she[k] = Et8[k];
    }
  }
}

__device__ __forceinline__ float es_actnoise(uint64_t seed, uint64_t ctr) {
  esrng::f32x4 v = esrng::normal4(ctr, seed, 0xACu);
  return v.x;
}

// ---- antithetic-pair forward -----------------------------------------------
// ES structure exploit: the +noise and -noise members of a pair share the
// SAME perturbation row. Instead of streaming two materialized bf16 blobs
// bf16(theta+sigma*eps) and bf16(theta-sigma*eps) from HBM (2 x n bytes per
// pair per step — the measured dominant cost of the whole framework), the
// pair forward streams ONE bf16(sigma*eps) row (HBM, nt loads) plus the
// bf16(theta) row that every pair shares (regular loads -> L2-resident
// across the grid), and forms W+/W- in registers. HBM weight traffic per
// step halves; effective weights are bf16(theta) +- bf16(sigma*eps), i.e.
// two bf16 roundings instead of one (parity tests use a matching torch
// reference).
__device__ __forceinline__ void bf8_fma_pair(uint4 t, uint4 e, float xp, float xm,
                                             float* accp, float* accm) {
  const uint32_t ts[4] = {t.x, t.y, t.z, t.w};
  const uint32_t es_[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float t0 = bf2f((uint16_t)(ts[q] & 0xFFFFu));
    const float e0 = bf2f((uint16_t)(es_[q] & 0xFFFFu));
    const float t1 = bf2f((uint16_t)(ts[q] >> 16));
    const float e1 = bf2f((uint16_t)(es_[q] >> 16));
    accp[2 * q] = fmaf(t0 + e0, xp, accp[2 * q]);
    accm[2 * q] = fmaf(t0 - e0, xm, accm[2 * q]);
    accp[2 * q + 1] = fmaf(t1 + e1, xp, accp[2 * q + 1]);
    accm[2 * q + 1] = fmaf(t1 - e1, xm, accm[2 * q + 1]);
  }
}

// Dual-member mlp_layers: one theta stream + one sigma*eps stream drive BOTH
// members' forwards. Same (oi, ip) tiling, depth-4 pipelining and partial
// layout as mlp_layers, with per-member accumulator/partial sets. `partial`
// needs 2 x 256*8 floats; bufAp/bufAm/bufBp/bufBm are maxdim floats each.
// Returns the +/- output pointers via xp_out/xm_out.
__device__ __forceinline__ void mlp_layers_pair(
    const uint16_t* __restrict__ tb, const uint16_t* __restrict__ eb,
    const MlpShape& sh, float* bufAp, float* bufAm, float* bufBp, float* bufBm,
    float* partial, int tid, int nthreads, int act_final,
    float** xp_out, float** xm_out) {
  float* xp = bufAp;
  float* xm = bufAm;
  float* yp = bufBp;
  float* ym = bufBm;
  float* partm = partial + 256 * 8;
  for (int l = 0; l < sh.n_layers; ++l) {
    const int I = sh.dims[l], O = sh.dims[l + 1];
    const uint16_t* Tt = tb + sh.woff[l];
    const uint16_t* Et = eb + sh.woff[l];
    const uint16_t* TBs = tb + sh.boff[l];
    const uint16_t* EBs = eb + sh.boff[l];
    const bool do_act = (l < sh.n_layers - 1) || act_final;

    if (sh.vec_ok[l]) {
      const int OCT = O >> 3;
      const int PART = nthreads / OCT;
      const int oi = tid % OCT, ip = tid / OCT;
      float accp[8], accm[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) accp[q] = accm[q] = 0.0f;
      if (ip < PART) {
        const uint16_t* tcol = Tt + (oi << 3);
        const uint16_t* ecol = Et + (oi << 3);
        // eps rows are touched by exactly one block -> nt; theta is shared
        // by the whole grid -> regular load, stays L2/MALL-resident
        auto lde = [&](int i) { return es_ld16_nt(ecol + (int64_t)i * O); };
        auto ldt = [&](int i) {
          return *reinterpret_cast<const uint4*>(tcol + (int64_t)i * O);
        };
        // es_walk_ring4 written out: it loads four theta, then four eps, and
        // the helper's one-value-per-row ld would bundle them per row, which
        // is a different kernel (118 instead of 168 VGPRs; see ROADMAP.md)
        int i = ip;
        const int step4 = PART * 4;
        if (i + 3 * PART < I) {
          uint4 t0 = ldt(i), t1 = ldt(i + PART), t2 = ldt(i + 2 * PART),
                t3 = ldt(i + 3 * PART);
          uint4 e0 = lde(i), e1 = lde(i + PART), e2 = lde(i + 2 * PART),
                e3 = lde(i + 3 * PART);
          for (; i + 7 * PART < I; i += step4) {
            const uint4 nt0 = ldt(i + 4 * PART), nt1 = ldt(i + 5 * PART),
                        nt2 = ldt(i + 6 * PART), nt3 = ldt(i + 7 * PART);
            const uint4 ne0 = lde(i + 4 * PART), ne1 = lde(i + 5 * PART),
                        ne2 = lde(i + 6 * PART), ne3 = lde(i + 7 * PART);
            bf8_fma_pair(t0, e0, xp[i], xm[i], accp, accm);
            bf8_fma_pair(t1, e1, xp[i + PART], xm[i + PART], accp, accm);
            bf8_fma_pair(t2, e2, xp[i + 2 * PART], xm[i + 2 * PART], accp, accm);
            bf8_fma_pair(t3, e3, xp[i + 3 * PART], xm[i + 3 * PART], accp, accm);
            t0 = nt0; t1 = nt1; t2 = nt2; t3 = nt3;
            e0 = ne0; e1 = ne1; e2 = ne2; e3 = ne3;
          }
          bf8_fma_pair(t0, e0, xp[i], xm[i], accp, accm);
          bf8_fma_pair(t1, e1, xp[i + PART], xm[i + PART], accp, accm);
          bf8_fma_pair(t2, e2, xp[i + 2 * PART], xm[i + 2 * PART], accp, accm);
          bf8_fma_pair(t3, e3, xp[i + 3 * PART], xm[i + 3 * PART], accp, accm);
          i += step4;
        }
        for (; i < I; i += PART)
          bf8_fma_pair(ldt(i), lde(i), xp[i], xm[i], accp, accm);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          partial[(ip * OCT + oi) * 8 + q] = accp[q];
          partm[(ip * OCT + oi) * 8 + q] = accm[q];
        }
      }
      __syncthreads();
      for (int o = tid; o < O; o += nthreads) {
        const float tB = bf2f(TBs[o]), eB = bf2f(EBs[o]);
        float sp = tB + eB, sm = tB - eB;
        const int oo = o >> 3, j = o & 7;
        for (int p = 0; p < PART; ++p) {
          sp += partial[(p * OCT + oo) * 8 + j];
          sm += partm[(p * OCT + oo) * 8 + j];
        }
        yp[o] = do_act ? tanhf(sp) : sp;
        ym[o] = do_act ? tanhf(sm) : sm;
      }
    } else {
      // dual tiled scalar path (small / odd layers, e.g. the action head)
      const int PART = nthreads / O;
      if (PART > 1) {
        const int oi = tid % O, ip = tid / O;
        float accp = 0.0f, accm = 0.0f;
        if (ip < PART) {
          es_walk_batched<EsTE16>(
              ip, PART, I,
              [&](int r) {
                return EsTE16{Tt[(int64_t)r * O + oi], Et[(int64_t)r * O + oi]};
              },
              [&](EsTE16 w, int r) {
                const float tw = bf2f(w.t), ew = bf2f(w.e);
                accp = fmaf(tw + ew, xp[r], accp);
                accm = fmaf(tw - ew, xm[r], accm);
              });
          partial[ip * O + oi] = accp;
          partm[ip * O + oi] = accm;
        }
        __syncthreads();
        for (int o = tid; o < O; o += nthreads) {
          const float tB = bf2f(TBs[o]), eB = bf2f(EBs[o]);
          float sp = tB + eB, sm = tB - eB;
          for (int p = 0; p < PART; ++p) {
            sp += partial[p * O + o];
            sm += partm[p * O + o];
          }
          yp[o] = do_act ? tanhf(sp) : sp;
          ym[o] = do_act ? tanhf(sm) : sm;
        }
      } else {
        for (int o = tid; o < O; o += nthreads) {
          const float tB = bf2f(TBs[o]), eB = bf2f(EBs[o]);
          float accp = tB + eB, accm = tB - eB;
          es_walk_batched<EsTE16>(
              0, 1, I,
              [&](int r) {
                return EsTE16{Tt[(int64_t)r * O + o], Et[(int64_t)r * O + o]};
              },
              [&](EsTE16 w, int r) {
                const float tw = bf2f(w.t), ew = bf2f(w.e);
                accp = fmaf(tw + ew, xp[r], accp);
                accm = fmaf(tw - ew, xm[r], accm);
              });
          yp[o] = do_act ? tanhf(accp) : accp;
          ym[o] = do_act ? tanhf(accm) : accm;
        }
      }
    }
    __syncthreads();
    float* t = xp; xp = yp; yp = t;
    t = xm; xm = ym; ym = t;
  }
  *xp_out = xp;
  *xm_out = xm;
}
