// What the wave-per-slot kernels share (rollout_classic_wave.hip,
// rollout_tag_wave.hip): the launch geometry and what it covers, a weight row
// copied into a wave's own LDS region and an MLP of layers at most 64 wide
// walked inside the wave, activations in registers.
#pragma once
#include "mlp_core.h"

#define WAVE_MAXW 64           // widest layer the lane mapping covers
#define WAVE_LDS_BUDGET 65536  // dynamic LDS of a block
#define WAVE_WAVES 4           // waves of a block

// Coverage, the one place it is decided. A wave's LDS region holds its rows,
// each padded to 16 B; a block holds the regions of 4, 2 or 1 waves.
//
// Elements of a row of sh, or -116 where a layer is wider than WAVE_MAXW.
static inline int wave_row_elems(const MlpShape& sh) {
  for (int l = 0; l <= sh.n_layers; ++l)
    if (sh.dims[l] > WAVE_MAXW) return -116;
  return (int)(sh.boff[sh.n_layers - 1] + sh.dims[sh.n_layers]);
}

static inline int wave_row_bytes(int n_elems, bool f32) {
  return (n_elems * (f32 ? 4 : 2) + 15) & ~15;
}

// Regions of region_bytes a block runs (the most that fit WAVE_LDS_BUDGET
// beside shared_bytes that all its waves read), or -116 where one alone does
// not fit.
static inline int wave_regions_per_block(int region_bytes, int shared_bytes = 0) {
  const int room = WAVE_LDS_BUDGET - shared_bytes;
  if (region_bytes > room) return -116;
  return 4 * region_bytes <= room ? 4 : 2 * region_bytes <= room ? 2 : 1;
}

// Keeps the compiler from pairing the lanes' scalar fp32 operations into
// packed ones in these kernels.
#define CLW_KERNEL_ATTR __attribute__((target("no-packed-fp32-ops")))

__device__ __forceinline__ float clw_weight(const uint16_t* w, int k) { return bf2f(w[k]); }
__device__ __forceinline__ float clw_weight(const float* w, int k) { return w[k]; }

__device__ __forceinline__ float clw_readlane(float v, int lane_uniform) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane_uniform));
}

// The slot's row, global -> this wave's LDS region: 16-B chunks where the row
// starts 16-B aligned, elements otherwise and behind the last whole chunk.
// Reads n_params elements of the row and nothing else.
template <typename WT>
__device__ __forceinline__ void wave_row_to_lds(const WT* __restrict__ src, WT* dst,
                                                int n_params, int lane) {
  constexpr int PER = 16 / (int)sizeof(WT);
  int done = 0;
  if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {  // wave-uniform
    const int nvec = n_params / PER;
    for (int c = lane; c < nvec; c += 64)
      reinterpret_cast<es_u32x4*>(dst)[c] = reinterpret_cast<const es_u32x4*>(src)[c];
    done = nvec * PER;
  }
  for (int k = done + lane; k < n_params; k += 64) dst[k] = src[k];
  // the forward's reads are other lanes' writes
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The forward of one wave on a row held in LDS (wl, laid out as the blob's
// row: per layer W^T[i][o], then the bias). Lane i < dims[0] passes input i
// in x; on return lane o < dims[n_layers] holds output o, and every lane l
// holds output l % OP of the last layer where that is below its width.
//
// Layer I -> O, O <= 64: OP = the power of two >= O, P = 64 / OP. Lane l owns
// output o = l % OP and input partition p = l / OP and sums
// fmaf(w[i][o], x[i], acc) over i = p, p + P, ... ascending; the P partials
// meet in a butterfly at lane offsets OP, 2 OP, ... < 64 (a + b on both
// sides of every exchange, so all P lanes end on the same bits), then bias
// and tanhf. The order of every sum is fixed by the shape alone.
//
// Activations stay in registers: x[i] is read from lane i, with readlane
// when P == 1 (i is then wave-uniform) and with a bpermute otherwise. A 64-float
// LDS strip per wave was the alternative; it costs the same LDS instruction
// per input as the bpermute and a write, a fence and 1 KB a block on top.
//
// Every lane runs all ceil(I / P) trips. A trip behind a lane's last input
// reads row I - 1 and drops the product; a lane with o >= O computes output
// O - 1 over again: it reads inside the row, and since exchange partners
// share o nothing of it reaches an output below O.
template <typename WT>
__device__ __forceinline__ float wave_mlp_layers(const WT* wl, const MlpShape& sh, float x,
                                                 int lane, int act_final) {
  for (int l = 0; l < sh.n_layers; ++l) {
    const int I = sh.dims[l], O = sh.dims[l + 1];
    const WT* Wt = wl + (int)sh.woff[l];
    const WT* Bs = wl + (int)sh.boff[l];
    const bool do_act = (l < sh.n_layers - 1) || act_final;
    const int lg = O <= 1 ? 0 : 32 - __clz(O - 1);  // OP = 1 << lg
    const int OP = 1 << lg, P = 64 >> lg;
    const int o = min(lane & (OP - 1), O - 1), p = lane >> lg;
    float acc = 0.0f;
    // Trips go in hand-written fours, the four LDS reads and the four
    // cross-lane reads ahead of the four fmaf: the cross-lane operations are
    // convergent, and the compiler unrolls no loop of unknown length over one.
    if (P == 1) {
      auto wx = [&](int i, float& w, float& xi) {
        w = clw_weight(Wt, i * O + o);
        xi = clw_readlane(x, i);
      };
      int i = 0;
      for (; i + 4 <= I; i += 4) {
        float w[4], xi[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) wx(i + u, w[u], xi[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = fmaf(w[u], xi[u], acc);
      }
      for (; i < I; ++i) {
        float w, xi;
        wx(i, w, xi);
        acc = fmaf(w, xi, acc);
      }
    } else {
      const int T = (I + P - 1) >> (6 - lg);
      auto wx = [&](int k, float& w, float& xi) {  // returns: the trip has an input
        const int i = p + (k << (6 - lg));
        const int ic = min(i, I - 1);
        w = clw_weight(Wt, ic * O + o);
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
        for (int u = 0; u < 4; ++u) acc = ok[u] ? fmaf(w[u], xi[u], acc) : acc;
      }
      for (; k < T; ++k) {
        float w, xi;
        const bool ok = wx(k, w, xi);
        acc = ok ? fmaf(w, xi, acc) : acc;
      }
      for (int off = OP; off < 64; off <<= 1) acc += __shfl_xor(acc, off, 64);
    }
    const float s = clw_weight(Bs, o) + acc;
    x = do_act ? tanhf(s) : s;
  }
  return x;
}
