// K2 — batched antithetic perturbation ("pheno") kernel.
//
// Materializes the whole population's perturbed parameter sets in one launch:
//   out[b][t] = bf16( theta[t] + sign[b] * std * table[offset[b] + t] )
// vs the reference's one-at-a-time host pheno (src/core/policy.py:61-67).
//
// `theta` is stored in the engine's FORWARD layout (per layer: W^T then b) so
// every access here and in mlp_fwd/grad is coalesced; the flat<->forward
// permutation lives host-side in the engine. sign[b] = +1/-1 for antithetic
// pairs and 0 for the noiseless-evaluation slot (then out = theta exactly).
#include "common.h"
#include "mlp_core.h"

__global__ void pheno_bf16_kernel(uint16_t* __restrict__ out, const float* __restrict__ theta,
                                  const float* __restrict__ table,
                                  const int64_t* __restrict__ offsets,
                                  const float* __restrict__ signs, int64_t n_params,
                                  int64_t row_stride, float std) {
  int64_t b = blockIdx.y;
  const float s = signs[b] * std;
  const float* noise = table + offsets[b];
  uint16_t* ob = out + b * row_stride;
  // thread owns 8 consecutive elements: theta reads as 2x float4 and the
  // bf16 row (16 B-aligned via row_stride padding) writes as ONE 16 B store;
  // the noise slice has arbitrary 4 B alignment, so its 8 loads stay scalar
  // (independent -> pipelined). 2 B/lane stores were the bottleneck before.
  typedef uint16_t u16x8 __attribute__((ext_vector_type(8)));
  const int64_t stride8 = (int64_t)gridDim.x * blockDim.x * 8;
  int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  for (; t + 7 < n_params; t += stride8) {
    const float4 th0 = *reinterpret_cast<const float4*>(theta + t);
    const float4 th1 = *reinterpret_cast<const float4*>(theta + t + 4);
    float nz[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) nz[k] = noise[t + k];
    u16x8 v;
    v[0] = f2bf(th0.x + s * nz[0]);
    v[1] = f2bf(th0.y + s * nz[1]);
    v[2] = f2bf(th0.z + s * nz[2]);
    v[3] = f2bf(th0.w + s * nz[3]);
    v[4] = f2bf(th1.x + s * nz[4]);
    v[5] = f2bf(th1.y + s * nz[5]);
    v[6] = f2bf(th1.z + s * nz[6]);
    v[7] = f2bf(th1.w + s * nz[7]);
    *reinterpret_cast<u16x8*>(ob + t) = v;
  }
  for (; t < n_params; ++t) ob[t] = f2bf(theta[t] + s * noise[t]);
}

// ---- fp32 member rows (weights_dtype = "fp32") ------------------------------
//   out[b][t] = fmaf(sign[b] * std, table[offset[b] + t], theta[t])
// One rounding per element, written as an explicit fmaf so the result does
// not depend on the compiler's contraction setting; a sign-0 row is theta
// bit for bit. Thread owns 4 consecutive elements: theta reads as one float4
// and the row (16-B aligned: row_stride % 4 == 0) writes as ONE 16-B store;
// the noise loads stay scalar (arbitrary 4-B alignment), as above. Elements
// [n_params, row_stride) are not written.
__global__ void pheno_f32_kernel(float* __restrict__ out, const float* __restrict__ theta,
                                 const float* __restrict__ table,
                                 const int64_t* __restrict__ offsets,
                                 const float* __restrict__ signs, int64_t n_params,
                                 int64_t row_stride, float std) {
  const int64_t b = blockIdx.y;
  const float s = signs[b] * std;
  const float* noise = table + offsets[b];
  float* ob = out + b * row_stride;
  const int64_t stride4 = (int64_t)gridDim.x * blockDim.x * 4;
  int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  for (; t + 3 < n_params; t += stride4) {
    const float4 th = *reinterpret_cast<const float4*>(theta + t);
    float nz[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) nz[k] = noise[t + k];
    float4 v;
    v.x = fmaf(s, nz[0], th.x);
    v.y = fmaf(s, nz[1], th.y);
    v.z = fmaf(s, nz[2], th.z);
    v.w = fmaf(s, nz[3], th.w);
    *reinterpret_cast<float4*>(ob + t) = v;
  }
  for (; t < n_params; ++t) ob[t] = fmaf(s, noise[t], theta[t]);
}

// Same argument list as es_pheno_bf16; out is float*, row_stride in elements.
extern "C" int es_pheno_f32(void* out, const void* theta, const void* table,
                            const void* offsets, const void* signs, int64_t n_pop,
                            int64_t n_params, int64_t row_stride, float std, void* stream) {
  if (row_stride < n_params || row_stride % 4 != 0) return -102;
  int threads = 256;
  int bx = (int)std::min<int64_t>((n_params + threads * 4 - 1) / (threads * 4), 1024);
  dim3 grid(bx, (unsigned)n_pop);
  pheno_f32_kernel<<<grid, dim3(threads), 0, (hipStream_t)stream>>>(
      (float*)out, (const float*)theta, (const float*)table, (const int64_t*)offsets,
      (const float*)signs, n_params, row_stride, std);
  ES_CHECK_LAUNCH();
  return 0;
}

// ---- fp8 sigma*eps blob -----------------------------------------------------
// The antithetic-pair rollout's dominant cost is streaming the per-pair
// sigma*eps rows from HBM. fp8 (OCP e4m3fn) halves those bytes AND halves
// the load count (one 16-B load covers 16 elements = one octet of TWO
// consecutive i-rows), while the +-e antithetic cancellation stays exact
// (both members decode the SAME quantized e). Weight blocks of vectorizable
// layers are stored ROW-PAIR INTERLEAVED so the 16-B load is contiguous:
//   byte(i, o) = woff + (i & ~1)*O + (o>>3)*16 + (i & 1)*8 + (o & 7)
// scalar-path layers and biases stay element-ordered (1 byte per element).
__device__ __forceinline__ int64_t fp8_src_elem(const MlpShape& sh, int64_t b) {
  for (int l = 0; l < sh.n_layers; ++l) {
    if (b < sh.boff[l]) {  // weight block l (b >= woff[l] by construction)
      if (!sh.vec_ok[l]) return b;  // scalar-path layer: plain layout
      const int O = sh.dims[l + 1];
      // odd input dim: row 0 stays plain; rows 1.. are pair-interleaved
      const int ro = sh.dims[l] & 1;
      const int64_t rel = b - sh.woff[l] - (int64_t)ro * O;
      if (rel < 0) return b;  // inside the plain row 0
      const int64_t pairblk = rel / (2 * O);
      const int within = (int)(rel % (2 * O));
      const int col = (within >> 4) * 8 + (within & 7);
      const int half = (within >> 3) & 1;
      return sh.woff[l] + (ro + 2 * pairblk + half) * (int64_t)O + col;
    }
    const int64_t bias_end = sh.boff[l] + sh.dims[l + 1];
    if (b < bias_end) return b;  // bias: plain
  }
  return b;
}

__global__ void pheno_fp8_kernel(uint8_t* __restrict__ out, const float* __restrict__ table,
                                 const int64_t* __restrict__ offsets, MlpShape sh,
                                 int64_t n_params, int64_t row_stride, float std) {
  const int64_t b = blockIdx.y;
  const float* noise = table + offsets[b];
  uint8_t* ob = out + b * row_stride;
  // one thread per 4 output bytes -> one uint32 store
  const int64_t stride4 = (int64_t)gridDim.x * blockDim.x * 4;
  for (int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
       t < row_stride; t += stride4) {
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t byte = t + k;
      v[k] = 0.0f;
      if (byte < n_params) v[k] = std * noise[fp8_src_elem(sh, byte)];
    }
    *reinterpret_cast<uint32_t*>(ob + t) = fp8x4_encode(v[0], v[1], v[2], v[3]);
  }
}

extern "C" int es_pheno_fp8(void* out, const void* table, const void* offsets,
                            const int32_t* dims_host, int32_t ndims, int64_t n_pop,
                            int64_t n_params, int64_t row_stride, float std,
                            void* stream) {
  MlpShape sh;
  int rc = mlp_shape_init(&sh, dims_host, ndims, row_stride);
  if (rc) return rc;
  int threads = 256;
  int bx = (int)std::min<int64_t>((row_stride + threads * 4 - 1) / (threads * 4), 1024);
  dim3 grid(bx, (unsigned)n_pop);
  pheno_fp8_kernel<<<grid, dim3(threads), 0, (hipStream_t)stream>>>(
      (uint8_t*)out, (const float*)table, (const int64_t*)offsets, sh, n_params,
      row_stride, std);
  ES_CHECK_LAUNCH();
  return 0;
}

extern "C" int es_pheno_bf16(void* out, const void* theta, const void* table,
                             const void* offsets, const void* signs, int64_t n_pop,
                             int64_t n_params, int64_t row_stride, float std, void* stream) {
  int threads = 256;
  int bx = (int)std::min<int64_t>((n_params + threads * 8 - 1) / (threads * 8), 1024);
  dim3 grid(bx, (unsigned)n_pop);
  pheno_bf16_kernel<<<grid, dim3(threads), 0, (hipStream_t)stream>>>(
      (uint16_t*)out, (const float*)theta, (const float*)table, (const int64_t*)offsets,
      (const float*)signs, n_params, row_stride, std);
  ES_CHECK_LAUNCH();
  return 0;
}
