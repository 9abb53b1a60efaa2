// What the PursuitTag episode kernels share (rollout_tag.hip: a workgroup
// per game; rollout_tag_wave.hip: a wavefront per game): the game's
// constants, a policy's launch arguments and their checks.
#pragma once
#include "mlp_core.h"

#define TAG_OB 8        // own p, own v, other p, other v
#define TAG_AC 2
#define TAG_ARENA 5.0f  // BatchedPursuitTag.ARENA

struct TagPolicy {
  const void* weights;  // member rows of the kernel's weight type, row_stride apart
  const float* obmean;
  const float* obstd;
  const float* ac_std_dev;
  int64_t row_stride;
  float ob_clip;
  MlpShape sh;
};

// f32: the rows are float32 and a layer is quad-tiled only where its 16-B
// loads are aligned for THIS policy's stride (mlp_shape_vec_f32).
static inline int tag_policy_init(TagPolicy* P, bool f32, const void* weights,
                                  const void* obmean, const void* obstd,
                                  const void* ac_std_dev, const int32_t* dims_host,
                                  int32_t ndims, int64_t row_stride, float ob_clip) {
  int rc = mlp_shape_init(&P->sh, dims_host, ndims, row_stride);
  if (rc) return rc;
  if (f32) mlp_shape_vec_f32(&P->sh, row_stride);
  if (P->sh.dims[0] != TAG_OB) return -110;
  if (P->sh.dims[P->sh.n_layers] < TAG_AC) return -111;
  P->weights = weights;
  P->obmean = (const float*)obmean;
  P->obstd = (const float*)obstd;
  P->ac_std_dev = (const float*)ac_std_dev;
  P->row_stride = row_stride;
  P->ob_clip = ob_clip;
  return 0;
}
