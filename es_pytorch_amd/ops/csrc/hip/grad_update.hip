// K5 + K6 in one launch, with the POPULATION spread over the grid as well as
// the parameters — the update of a generation for small nets and large
// populations, where grad.hip's grid (n_params alone) leaves most CUs idle.
//
//   g[t]   = sum_p fits[p] * table[offsets[p] + t]          t in [0, n_params)
//   theta, m, v <- Adam / SGD step on g, the arithmetic of update.hip
//
// Grid (X, Y): blockIdx.x picks a chunk of GU_CHUNK = 256 parameters,
// blockIdx.y a contiguous slice of the population rows. A block is four waves;
// every wave covers the whole chunk (lane l owns floats 4l..4l+3 of it, so a
// wave reads 1 KB contiguous per row) and walks its own contiguous quarter of
// the block's rows in ascending order with GU_DEPTH rows in flight. The four
// accumulators meet in LDS, summed in wave order, and the block stores its
// partial. A ticket per column (an int32 atomicAdd, as rank_count_kernel uses)
// tells the block that stored last; that block sums the column's Y partials in
// ascending y — so the result does not depend on which block it was — writes
// g, applies the optimizer to its chunk and puts the ticket back to 0. No
// block waits for another, and no floating-point atomic is used: (X, Y) and
// every slice bound are a function of (n_pop, n_params) alone, so every rank
// of a multi-GPU run computes the same bits.
#include "common.h"

#define GU_THREADS 256
#define GU_CHUNK 256        // parameters per block: 64 lanes x 4 floats
#define GU_DEPTH 8          // rows in flight per wave
#define GU_STAGE 256        // (fit, offset) rows a wave stages in LDS per tile
#define GU_MIN_BLOCKS 512   // the plan grows Y until the grid has this many
#define GU_MIN_WAVE_ROWS 8  // ... while every wave keeps this many rows

typedef float gu_f32x4 __attribute__((ext_vector_type(4)));

// a value that is the same in every lane of the wave, moved to scalar registers
__device__ __forceinline__ uint32_t gu_uniform(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
}
__device__ __forceinline__ int64_t gu_uniform(int64_t x) {
  const uint64_t u = (uint64_t)x;
  return (int64_t)(((uint64_t)gu_uniform((uint32_t)(u >> 32)) << 32) |
                   gu_uniform((uint32_t)u));
}
__device__ __forceinline__ float gu_uniform(float x) {
  return __uint_as_float(gu_uniform(__float_as_uint(x)));
}

// One wave's walk over `cnt` >= 1 staged rows. r[0..DEPTH) is a ring of rows
// in flight: in a turn of DEPTH steps, step k consumes r[k] (row i + k) and
// refills it with row i + DEPTH + k — every index is static after unrolling,
// so the sets only change role and nothing is copied. VEC: the chunk lies
// wholly inside n_params and a lane reads its 4 floats as one 16-byte load at
// 4-byte alignment; otherwise four dword loads at indices clamped into the
// row (a lane past n_params accumulates values that are never stored).
// `chunk` is the table shifted to the block's first parameter (wave-uniform),
// `valid` the parameters of the chunk inside n_params (1..256).
template <bool Q, bool VEC>
__device__ __forceinline__ void gu_walk(gu_f32x4& acc, const float* __restrict__ chunk,
                                        const float* s_fit, const int64_t* s_off, int cnt,
                                        int lane, int valid, float qstd, float qinv) {
  int l4 = 4 * lane;
  int e[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) e[j] = min(4 * lane + j, valid - 1);
  // A step is use-then-refill. The compiler would otherwise issue a turn's
  // refills ahead of its uses: a second ring, and a wait and a copy per row
  // (ROADMAP round 4). This empty statement makes the lane offsets of the
  // refill depend on the accumulators of the use, which fixes the order.
  auto order = [&]() {
    if (VEC) asm volatile("" : "+v"(acc), "+v"(l4));
    else asm volatile("" : "+v"(acc), "+v"(e[0]), "+v"(e[1]), "+v"(e[2]), "+v"(e[3]));
  };
  auto load = [&](int i) {
    const float* row = chunk + gu_uniform(s_off[i]);
    gu_f32x4 x;
    if (VEC) {
      __builtin_memcpy(&x, row + l4, sizeof(x));
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = row[e[j]];
    }
    return x;
  };
  auto use = [&](int i, const gu_f32x4& x) {
    const float f = gu_uniform(s_fit[i]);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      acc[j] = fmaf(f, Q ? e4m3_roundtrip(qstd * x[j]) * qinv : x[j], acc[j]);
  };
  auto use_if = [&](int i, const gu_f32x4& x) {
    const bool live = i < cnt;
    const float f = gu_uniform(s_fit[live ? i : 0]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float y = fmaf(f, Q ? e4m3_roundtrip(qstd * x[j]) * qinv : x[j], acc[j]);
      acc[j] = live ? y : acc[j];
    }
  };

  // past the end of the rows the last row is fetched again and never used
  const int last = cnt - 1;
  gu_f32x4 r[GU_DEPTH];
#pragma unroll
  for (int k = 0; k < GU_DEPTH; ++k) r[k] = load(min(k, last));
  int i = 0;
  // whole turns: every row consumed and every row fetched exists
  for (; i + 2 * GU_DEPTH <= cnt; i += GU_DEPTH) {
#pragma unroll
    for (int k = 0; k < GU_DEPTH; ++k) {
      use(i + k, r[k]);
      order();
      r[k] = load(i + GU_DEPTH + k);
    }
  }
  // at most 2 * DEPTH - 1 rows are left: two straight-line turns, the second
  // of which only consumes. No branch: a step past the end keeps acc by a
  // select, so the ring stays in the registers it has.
#pragma unroll
  for (int k = 0; k < GU_DEPTH; ++k) {
    use_if(i + k, r[k]);
    order();
    r[k] = load(min(i + GU_DEPTH + k, last));
  }
  i += GU_DEPTH;
#pragma unroll
  for (int k = 0; k < GU_DEPTH; ++k) use_if(i + k, r[k]);
}

// OPT 0: Adam (m, v moments). OPT 1: SGD (v the momentum buffer; m, b2, eps
// unused). partials (Y, X, GU_CHUNK) fp32 and ticket (X,) int32, all zero
// before the first launch, are touched only when Y > 1.
template <bool Q, int OPT>
__global__ void __launch_bounds__(GU_THREADS)
grad_update_kernel(float* __restrict__ theta, float* __restrict__ m, float* __restrict__ v,
                   float* __restrict__ g, float* partials, int* ticket,
                   const float* __restrict__ table, const float* __restrict__ fits,
                   const int64_t* __restrict__ offsets, int64_t n_pop, int64_t n_params,
                   float qstd, float a, float b1, float b2, float eps, float l2,
                   float gscale) {
  __shared__ float s_fit[4][GU_STAGE];
  __shared__ int64_t s_off[4][GU_STAGE];
  __shared__ __attribute__((aligned(16))) float s_acc[4][GU_CHUNK];
  __shared__ int s_last;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = (int)gu_uniform((uint32_t)(tid >> 6));  // scalar: so are the row bounds
  const int64_t X = gridDim.x, Y = gridDim.y;
  const int64_t base = (int64_t)blockIdx.x * GU_CHUNK;
  const float qinv = Q ? 1.0f / qstd : 0.0f;

  // the block's rows [r0, r0 + len), the wave's [w0, w1): empty when the
  // population is smaller than the number of waves
  const int64_t r0 = n_pop * blockIdx.y / Y;
  const int64_t len = n_pop * (blockIdx.y + 1) / Y - r0;
  const int64_t w0 = r0 + len * wave / 4;
  const int64_t w1 = r0 + len * (wave + 1) / 4;
  int64_t longest = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) longest = max(longest, len * (w + 1) / 4 - len * w / 4);
  const int64_t n_tiles = (longest + GU_STAGE - 1) / GU_STAGE;

  // ---- phase A: the block's partial gather
  const int valid = (int)min((int64_t)GU_CHUNK, n_params - base);
  const float* chunk = table + base;
  gu_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int64_t tile = 0; tile < n_tiles; ++tile) {
    const int64_t p0 = w0 + tile * GU_STAGE;
    const int cnt = (int)max((int64_t)0, min((int64_t)GU_STAGE, w1 - p0));
    __syncthreads();                    // the previous tile is consumed
    for (int i = lane; i < cnt; i += 64) {
      s_fit[wave][i] = fits[p0 + i];
      s_off[wave][i] = offsets[p0 + i];
    }
    __syncthreads();
    if (cnt > 0) {
      if (valid == GU_CHUNK)
        gu_walk<Q, true>(acc, chunk, s_fit[wave], s_off[wave], cnt, lane, valid, qstd, qinv);
      else
        gu_walk<Q, false>(acc, chunk, s_fit[wave], s_off[wave], cnt, lane, valid, qstd, qinv);
    }
  }
  *reinterpret_cast<gu_f32x4*>(&s_acc[wave][4 * lane]) = acc;
  __syncthreads();
  // thread tid now owns parameter base + tid
  float gsum = ((s_acc[0][tid] + s_acc[1][tid]) + s_acc[2][tid]) + s_acc[3][tid];

  // ---- phase B: the block that stores its column's last partial finishes it
  if (Y > 1) {
    partials[((int64_t)blockIdx.y * X + blockIdx.x) * GU_CHUNK + tid] = gsum;
    __threadfence();
    __syncthreads();
    if (tid == 0) {
      __threadfence();
      s_last = atomicAdd(&ticket[blockIdx.x], 1) == (int)Y - 1;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();                    // the other blocks' partials are visible
    const float* col = partials + (int64_t)blockIdx.x * GU_CHUNK + tid;
    const int64_t stride = X * GU_CHUNK;
    gsum = 0.0f;
    int64_t y = 0;
    // 16 loads in flight, the adds still in ascending y
    for (; y + 16 <= Y; y += 16) {
      float p[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) p[u] = col[(y + u) * stride];
#pragma unroll
      for (int u = 0; u < 16; ++u) gsum += p[u];
    }
    for (; y < Y; ++y) gsum += col[y * stride];
    if (tid == 0) ticket[blockIdx.x] = 0;  // the next launch needs no memset
  }

  const int64_t t = base + tid;
  if (t >= n_params) return;
  g[t] = gsum;
  // update.hip's expressions, in its order
  const float th = theta[t];
  const float gg = l2 * th - gsum * gscale;
  if (OPT == 0) {
    const float mn = b1 * m[t] + (1.0f - b1) * gg;
    const float vn = b2 * v[t] + (1.0f - b2) * gg * gg;
    m[t] = mn;
    v[t] = vn;
    theta[t] = th - a * mn / (sqrtf(vn) + eps);
  } else {
    const float vn = b1 * v[t] + (1.0f - b1) * gg;
    v[t] = vn;
    theta[t] = th - a * vn;
  }
}

// The grid of es_grad_update for a shape, and the floats its `partials` needs:
// X = ceil(n_params / 256) columns; Y the smallest power of two with
// X * Y >= 512, halved while a wave would keep fewer than 8 rows
// (n_pop < 4 * 8 * Y); Y = 1 when the population is tiny or X already large.
// A function of the two sizes alone — never of the device. -120: a size < 1 or
// more columns than a grid holds.
extern "C" int es_grad_update_plan(int64_t n_pop, int64_t n_params, int32_t* Y,
                                   int64_t* workspace_floats) {
  if (n_pop < 1 || n_params < 1) return -120;
  const int64_t X = (n_params + GU_CHUNK - 1) / GU_CHUNK;
  if (X > 0x7fffffff) return -120;
  int64_t y = 1;
  while (X * y < GU_MIN_BLOCKS) y <<= 1;
  while (y > 1 && n_pop < 4 * GU_MIN_WAVE_ROWS * y) y >>= 1;
  if (Y) *Y = (int32_t)y;
  if (workspace_floats) *workspace_floats = X * y * GU_CHUNK;
  return 0;
}

// theta, m, v, g (n_params,) fp32; partials fp32 of the size
// es_grad_update_plan gives, ticket (ceil(n_params / 256),) int32, zero before
// the first launch (every launch leaves it zero); table, fits, offsets, n_pop, n_params,
// qstd as es_grad_gather. opt 0: Adam with a = the bias-corrected lr, b1, b2,
// eps as es_adam_step. opt 1: SGD with a = lr, b1 = momentum, v the momentum
// buffer as es_sgd_step; m, b2, eps ignored. -120: a size < 1 or another opt.
extern "C" int es_grad_update(void* theta, void* m, void* v, void* g, void* partials,
                              void* ticket, const void* table, const void* fits,
                              const void* offsets, int64_t n_pop, int64_t n_params,
                              float qstd, int32_t opt, float a_or_lr, float b1_or_momentum,
                              float b2, float eps, float l2, float gscale, void* stream) {
  int32_t Y = 0;
  if (opt < 0 || opt > 1) return -120;
  const int rc = es_grad_update_plan(n_pop, n_params, &Y, nullptr);
  if (rc != 0) return rc;
  const dim3 grid((unsigned)((n_params + GU_CHUNK - 1) / GU_CHUNK), (unsigned)Y);
  const bool q = qstd > 0.0f;
#define ES_LAUNCH_GU(QF, OPT)                                                        \
  grad_update_kernel<QF, OPT><<<grid, dim3(GU_THREADS), 0, (hipStream_t)stream>>>(   \
      (float*)theta, (float*)m, (float*)v, (float*)g, (float*)partials, (int*)ticket, \
      (const float*)table, (const float*)fits, (const int64_t*)offsets, n_pop,       \
      n_params, qstd, a_or_lr, b1_or_momentum, b2, eps, l2, gscale)
  if (opt == 0) { if (q) ES_LAUNCH_GU(true, 0); else ES_LAUNCH_GU(false, 0); }
  else { if (q) ES_LAUNCH_GU(true, 1); else ES_LAUNCH_GU(false, 1); }
#undef ES_LAUNCH_GU
  ES_CHECK_LAUNCH();
  return 0;
}
