// The tail of a generation on the device: novelty scoring (fused kNN against
// the behaviour archive) and rank shaping (stable ranks by counting, then the
// centered / double-positive / two-objective transform), both in fp64 where
// the host is.
//
// es_novelty_knn    out[b] = mean of the min(k, N) smallest Euclidean
//                   distances from behaviour b to the N archive rows. The
//                   (B, N) distance matrix exists nowhere: each lane keeps its
//                   behaviour's k best squared distances in registers while the
//                   archive streams through LDS.
// es_rank_tail      rf[p], ri[p] of the all-gathered (R, 2*O + 1) fp64 rows:
//                   what CenteredRanker / DoublePositiveCenteredRanker, alone
//                   or inside a MultiObjectiveRanker, hand to es_grad_gather.
//
// Both return -119 for arguments outside what they serve and launch nothing.
// Fitnesses and behaviours are finite; NaN is not served.
#include <math.h>

#include "common.h"

// every rounding below is specified: no fused multiply-add anywhere in here
#pragma clang fp contract(off)

#define TL_THREADS 256
#define TL_TILE 1024                    // archive rows / fitness values per LDS tile
#define TL_PER_THREAD (TL_TILE / TL_THREADS)
#define TL_WAVE_ROWS (TL_TILE / 4)      // rows of a tile one wave walks
#define TL_MAXK 32

typedef double tl_f64x2 __attribute__((ext_vector_type(2)));

// ----------------------------------------------------------------- novelty
// One pass of compare-exchange down an ascending list: v takes its place and
// the largest entry falls off the end. Static indices only, so the list stays
// in registers.
template <int KP>
__device__ __forceinline__ void tl_insert(double (&t)[KP], double v) {
#pragma unroll
  for (int i = 0; i < KP; ++i) {
    const double lo = fmin(t[i], v);
    v = fmax(t[i], v);
    t[i] = lo;
  }
}

// Insert behind a wave-uniform guard: after the first rows almost no candidate
// beats any lane's current k-th distance, and the whole pass is skipped.
template <int KP>
__device__ __forceinline__ void tl_offer(double (&t)[KP], double v) {
  if (__any(v < t[KP - 1])) tl_insert<KP>(t, v);
}

// Block = 64 behaviours (lane l of every wave holds behaviour 64*blockIdx.x + l)
// x 4 waves, each walking its own quarter of every archive tile. The tile's
// rows are read as one broadcast 16-byte LDS load per row; tile t+1 waits in
// registers while tile t is consumed.
template <int KP>
__global__ void __launch_bounds__(TL_THREADS)
novelty_knn_kernel(double* __restrict__ out, const float* __restrict__ behv,
                   int64_t behv_stride, int64_t B,
                   const tl_f64x2* __restrict__ archive, int64_t N, int k) {
  // the archive tile (16 KB), then the merge area [3][KP][64] (up to 48 KB)
  constexpr int MERGE = 3 * KP * 64;
  constexpr int LDS_F64 = 2 * TL_TILE > MERGE ? 2 * TL_TILE : MERGE;
  __shared__ __attribute__((aligned(16))) double s_raw[LDS_F64];
  tl_f64x2* s_tile = reinterpret_cast<tl_f64x2*>(s_raw);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const double inf = __builtin_huge_val();

  // lanes past B compute on the last behaviour and do not store
  const int64_t b = (int64_t)blockIdx.x * 64 + lane;
  const int64_t bc = b < B ? b : B - 1;
  const double bx = (double)behv[bc * behv_stride];
  const double by = (double)behv[bc * behv_stride + 1];

  double t[KP];
#pragma unroll
  for (int i = 0; i < KP; ++i) t[i] = inf;

  // rows past N count as +inf: they never pass the guard
  auto load_tile = [&](int64_t tile, tl_f64x2 (&r)[TL_PER_THREAD]) {
#pragma unroll
    for (int j = 0; j < TL_PER_THREAD; ++j) {
      const int64_t row = tile * TL_TILE + j * TL_THREADS + tid;
      tl_f64x2 v;
      v.x = inf;
      v.y = inf;
      if (row < N) v = archive[row];
      r[j] = v;
    }
  };

  const int64_t n_tiles = (N + TL_TILE - 1) / TL_TILE;
  tl_f64x2 nx[TL_PER_THREAD];
  load_tile(0, nx);
  for (int64_t tile = 0; tile < n_tiles; ++tile) {
    __syncthreads();                    // the previous tile is consumed
#pragma unroll
    for (int j = 0; j < TL_PER_THREAD; ++j) s_tile[j * TL_THREADS + tid] = nx[j];
    __syncthreads();
    if (tile + 1 < n_tiles) load_tile(tile + 1, nx);
    const tl_f64x2* rows = s_tile + wave * TL_WAVE_ROWS;
#pragma unroll 4
    for (int r = 0; r < TL_WAVE_ROWS; ++r) {
      const tl_f64x2 a = rows[r];       // same address in all lanes: a broadcast
      const double dx = a.x - bx;
      const double dy = a.y - by;
      tl_offer<KP>(t, dx * dx + dy * dy);
    }
  }

  // waves 1..3 hand their lists to wave 0 as [wave][i][lane] (conflict-free)
  __syncthreads();
  if (wave > 0) {
#pragma unroll
    for (int i = 0; i < KP; ++i) s_raw[((wave - 1) * KP + i) * 64 + lane] = t[i];
  }
  __syncthreads();
  if (wave > 0) return;
  for (int w = 0; w < 3; ++w) {
#pragma unroll
    for (int i = 0; i < KP; ++i) tl_offer<KP>(t, s_raw[(w * KP + i) * 64 + lane]);
  }

  // the list is ascending, so this is the sum smallest first
  const int m = (int64_t)k < N ? k : (int)N;
  double sum = 0.0;
#pragma unroll
  for (int i = 0; i < KP; ++i)
    if (i < m) sum += sqrt(t[i]);
  if (b < B) out[b] = sum / (double)m;
}

// out (B,) fp64; behv fp32, behaviour b at behv[b*behv_stride .. +1]; archive
// (N, 2) contiguous fp64, 16-byte aligned. k in 1..32 (KP: the smallest of 4,
// 8, 16, 32 that holds k).
extern "C" int es_novelty_knn(void* out, const void* behv, int64_t behv_stride, int64_t B,
                              const void* archive, int64_t N, int32_t k, void* stream) {
  if (k < 1 || k > TL_MAXK || N < 1 || B < 1) return -119;
  if (((uintptr_t)archive & 15) != 0) return -119;
  const int64_t blocks = (B + 63) / 64;
  if (blocks > 0x7fffffff) return -119;
#define ES_LAUNCH_KNN(KP)                                                            \
  novelty_knn_kernel<KP><<<dim3((unsigned)blocks), dim3(TL_THREADS), 0,              \
                           (hipStream_t)stream>>>(                                   \
      (double*)out, (const float*)behv, behv_stride, B, (const tl_f64x2*)archive, N, k)
  if (k <= 4) ES_LAUNCH_KNN(4);
  else if (k <= 8) ES_LAUNCH_KNN(8);
  else if (k <= 16) ES_LAUNCH_KNN(16);
  else ES_LAUNCH_KNN(32);
#undef ES_LAUNCH_KNN
  ES_CHECK_LAUNCH();
  return 0;
}

// -------------------------------------------------------------------- rank
// Fitness of member i in column o: the + half then the - half of the rows.
template <int O>
__device__ __forceinline__ double tl_fit(const double* __restrict__ rows, int64_t R,
                                         int64_t i, int o) {
  return i < R ? rows[i * (2 * O + 1) + o] : rows[(i - R) * (2 * O + 1) + O + o];
}

// counts[o*n + i] += #{j in this slice's tiles : x_j < x_i, or x_j == x_i and
// j < i}: numpy's stable argsort rank once every slice has added its share.
// Grid (ceil(n/256), S); a thread owns member i and its O columns and walks the
// tiles blockIdx.y, blockIdx.y + S, ... Tiles are 256-aligned and the block's
// members contiguous, so only the tile that holds them needs the index rule.
template <int O>
__global__ void __launch_bounds__(TL_THREADS)
rank_count_kernel(int* __restrict__ counts, const double* __restrict__ rows, int64_t R) {
  __shared__ __attribute__((aligned(16))) double s_x[O][TL_TILE];
  const int tid = threadIdx.x;
  const int64_t n = 2 * R;
  const int64_t i = (int64_t)blockIdx.x * TL_THREADS + tid;
  const int64_t ic = i < n ? i : n - 1;
  const int64_t own = blockIdx.x / TL_PER_THREAD;   // the tile of this block's members
  const int64_t n_tiles = (n + TL_TILE - 1) / TL_TILE;
  const double inf = __builtin_huge_val();

  double xi[O];
  int c[O];
#pragma unroll
  for (int o = 0; o < O; ++o) {
    xi[o] = tl_fit<O>(rows, R, ic, o);
    c[o] = 0;
  }

  for (int64_t tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
    __syncthreads();
    // values past n are +inf: neither below nor equal to a finite fitness, and
    // the last tile is never wholly below a block's members
#pragma unroll
    for (int q = 0; q < TL_PER_THREAD; ++q) {
      const int64_t j = tile * TL_TILE + q * TL_THREADS + tid;
#pragma unroll
      for (int o = 0; o < O; ++o)
        s_x[o][q * TL_THREADS + tid] = j < n ? tl_fit<O>(rows, R, j, o) : inf;
    }
    __syncthreads();
    if (tile < own) {                   // every j < i
#pragma unroll 8
      for (int j = 0; j < TL_TILE; ++j)
#pragma unroll
        for (int o = 0; o < O; ++o) c[o] += s_x[o][j] <= xi[o];
    } else if (tile > own) {            // every j > i
#pragma unroll 8
      for (int j = 0; j < TL_TILE; ++j)
#pragma unroll
        for (int o = 0; o < O; ++o) c[o] += s_x[o][j] < xi[o];
    } else {
      const int me = (int)(ic - tile * TL_TILE);
#pragma unroll 8
      for (int j = 0; j < TL_TILE; ++j)
#pragma unroll
        for (int o = 0; o < O; ++o) {
          const double xj = s_x[o][j];
          c[o] += (xj < xi[o]) | ((xj == xi[o]) & (j < me));
        }
    }
  }
  if (i < n) {
#pragma unroll
    for (int o = 0; o < O; ++o) atomicAdd(&counts[o * n + i], c[o]);
  }
}

// The shaping of rankers.py on float32 arrays, one rounding per step.
__device__ __forceinline__ float tl_shape(int c, float denom, int mode) {
  float y = __fdiv_rn((float)c, denom);
  y = y - 0.5f;
  if (mode == 1 && y > 0.0f) y = y * 2.0f;
  return y;
}

template <int O>
__global__ void __launch_bounds__(TL_THREADS)
rank_finish_kernel(float* __restrict__ rf, int64_t* __restrict__ ri,
                   const int* __restrict__ counts, const double* __restrict__ rows,
                   int64_t R, float w0, float w1, int mode) {
  const int64_t p = (int64_t)blockIdx.x * TL_THREADS + threadIdx.x;
  if (p >= R) return;
  const int64_t n = 2 * R;
  const float denom = (float)(n - 1);
  float v[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int64_t i = p + h * R;
    const float y0 = tl_shape(counts[i], denom, mode);
    if (O == 1) {
      v[h] = y0;
    } else {
      const float y1 = tl_shape(counts[n + i], denom, mode);
      const float a = y0 * w0;
      const float bb = y1 * w1;
      v[h] = a + bb;
    }
  }
  rf[p] = v[0] - v[1];
  ri[p] = (int64_t)rows[p * (2 * O + 1) + 2 * O];
}

static int tl_cu_count() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
        v > 0)
      cus = v;
    else
      return 256;
  }
  return cus;
}

// rf (R,) fp32, ri (R,) int64, counts (O*2R,) int32 workspace (cleared here with
// a memset on `stream`, so not for graph capture), rows (R, 2*O + 1) fp64.
// mode 0 centered, 1 double-positive; w0, w1 weigh the two columns of O == 2.
// j_split > 0 forces that many slices of the j walk; 0 picks the smallest that
// puts two blocks on every CU, at most one slice per tile.
extern "C" int es_rank_tail(void* rf, void* ri, void* counts, const void* rows, int64_t R,
                            int32_t O, float w0, float w1, int32_t mode, int32_t j_split,
                            void* stream) {
  if (R < 1 || O < 1 || O > 2 || mode < 0 || mode > 1 || j_split < 0) return -119;
  const int64_t n = 2 * R;
  if (n > 0x7fffffff) return -119;      // counts are int32
  const int64_t blocks = (n + TL_THREADS - 1) / TL_THREADS;
  const int64_t n_tiles = (n + TL_TILE - 1) / TL_TILE;
  int64_t S = j_split;
  if (S == 0) S = (2 * (int64_t)tl_cu_count() + blocks - 1) / blocks;
  if (S > n_tiles) S = n_tiles;
  if (S > 65535) S = 65535;             // gridDim.y
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)O * n * sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  const dim3 cgrid((unsigned)blocks, (unsigned)S);
  const dim3 fgrid((unsigned)((R + TL_THREADS - 1) / TL_THREADS));
  if (O == 1) {
    rank_count_kernel<1><<<cgrid, dim3(TL_THREADS), 0, st>>>((int*)counts,
                                                             (const double*)rows, R);
    rank_finish_kernel<1><<<fgrid, dim3(TL_THREADS), 0, st>>>(
        (float*)rf, (int64_t*)ri, (const int*)counts, (const double*)rows, R, w0, w1, mode);
  } else {
    rank_count_kernel<2><<<cgrid, dim3(TL_THREADS), 0, st>>>((int*)counts,
                                                             (const double*)rows, R);
    rank_finish_kernel<2><<<fgrid, dim3(TL_THREADS), 0, st>>>(
        (float*)rf, (int64_t*)ri, (const int*)counts, (const double*)rows, R, w0, w1, mode);
  }
  ES_CHECK_LAUNCH();
  return 0;
}
