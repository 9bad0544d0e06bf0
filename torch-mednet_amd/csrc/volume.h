// What the inference and evaluation passes share (predict.hip, blend.hip, metrics.hip, components.hip): the limits of a volume, the
// row plan of the two-launch passes, grids, the extent check, voxel coordinates, the workgroup reduction and the per-voxel output
// arithmetic.  Every function is a pure function of its arguments: the same inputs give the same grids and the same bits.
#pragma once
#include "common.h"

namespace mednet {

constexpr int VOLUME_MAX_EXTENT = 2048;     // per axis
constexpr size_t VOLUME_MAX_ROWS = 2048;    // workgroups of a row-planned pass: at most 256 CUs x 8
constexpr size_t VOLUME_PER_ROW = 4096;     // voxels of a row until the row limit is reached: 256 threads x 16

// ---------------------------------------------------------------------------------------------- grids and the row plan
// workgroups for `items` at `per_block` items each, at least 1 and at most `cap` (a capped grid is walked in grid strides)
static inline size_t grid_blocks(size_t items, size_t per_block, size_t cap = ~(size_t)0) {
  return std::max<size_t>(1, std::min(cap, (items + per_block - 1) / per_block));
}

// Row r (one workgroup, one partial row in the workspace) takes the voxels [r * share, min(vox, (r + 1) * share)); share is a
// multiple of 256 and at most 2^33 / 2048 = 2^22 voxels, so 32-bit counters per workgroup cannot overflow.
struct RowPlan {
  unsigned rows;
  size_t share;
};
static inline RowPlan row_plan(size_t vox) {
  const unsigned rows = (unsigned)grid_blocks(vox, VOLUME_PER_ROW, VOLUME_MAX_ROWS);
  return {rows, align_up((vox + rows - 1) / rows, 256)};
}
// the device half: the row of this workgroup
template <typename I>
__device__ __forceinline__ void row_range(I vox, I share, I& begin, I& end) {
  begin = (I)blockIdx.x * share;
  end = begin + share;
  if (end > vox) end = vox;
}

// ---------------------------------------------------------------------------------------------- extents
static inline bool extents_ok(int d, int h, int w) {
  return d >= 1 && d <= VOLUME_MAX_EXTENT && h >= 1 && h <= VOLUME_MAX_EXTENT && w >= 1 && w <= VOLUME_MAX_EXTENT;
}
#define VOLUME_REQUIRE_EXTENTS(who, d, h, w) \
  MEDNET_REQUIRE(extents_ok(d, h, w), MEDNET_E_SHAPE, who ": extents %d x %d x %d outside 1 .. %d", d, h, w, VOLUME_MAX_EXTENT)

// bit k of a mirror mask reverses patch axis k
static inline int mirror_check(const char* who, int mirror) {
  MEDNET_REQUIRE(mirror >= 0 && mirror <= 7, MEDNET_E_UNSUPPORTED, "%s: mirror mask %d (supported: 0..7, bit k reverses axis k)", who,
                 mirror);
  return MEDNET_OK;
}

// ---------------------------------------------------------------------------------------------- voxel coordinates
// linear index (x fastest) -> coordinates; I is the caller's index type (size_t; int64_t in components.hip)
struct Zyx { int z, y, x; };
struct Czyx { int c, z, y, x; };
template <typename I>
__device__ __forceinline__ Zyx voxel_zyx(I i, int h, int w) {
  const I row = i / (I)w;
  return {(int)(row / (I)h), (int)(row % (I)h), (int)(i - row * (I)w)};
}
// with the channel as the slowest coordinate
__device__ __forceinline__ Czyx voxel_czyx(size_t i, int d, int h, int w) {
  const Zyx p = voxel_zyx(i, h, w);  // p.z holds c * d + z
  return {p.z / d, p.z % d, p.y, p.x};
}

// ---------------------------------------------------------------------------------------------- workgroup reduction
// fixed-order tree over the 256 threads of a workgroup; the result is valid in every thread
template <typename T, typename OP>
__device__ __forceinline__ T block_tree(T v, T* buf, OP op) {
  buf[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) buf[threadIdx.x] = op(buf[threadIdx.x], buf[threadIdx.x + s]);
    __syncthreads();
  }
  const T r = buf[0];
  __syncthreads();
  return r;
}

// ---------------------------------------------------------------------------------------------- per-voxel output arithmetic
// np.clip(v, 0, 255).astype(uint8): truncation
__device__ __forceinline__ uint8_t heat_to_u8(float v) { return (uint8_t)(int)fminf(fmaxf(v, 0.f), 255.f); }

// arg-max over class planes `stride` apart; the first maximum on ties, like torch.argmax
__device__ __forceinline__ int argmax_first(const float* __restrict__ planes, size_t stride, int ncls) {
  int best = 0;
  float bv = planes[0];
  for (int k = 1; k < ncls; ++k) {
    const float v = planes[(size_t)k * stride];
    if (v > bv) {
      bv = v;
      best = k;
    }
  }
  return best;
}

// One softmax over the classes of a voxel: max-subtracted, expf, one reciprocal.  value(k) is class k's logit (read again in every
// pass: the planes come from cache, they are not held), emit(k, p) takes its probability.
template <typename VALUE, typename EMIT>
__device__ __forceinline__ void plane_softmax(int ncls, VALUE value, EMIT emit) {
  float m = value(0);
  for (int k = 1; k < ncls; ++k) m = fmaxf(m, value(k));
  float s = 0.f;
  for (int k = 0; k < ncls; ++k) s += expf(value(k) - m);
  const float inv = 1.f / s;
  for (int k = 0; k < ncls; ++k) emit(k, expf(value(k) - m) * inv);
}

}  // namespace mednet
