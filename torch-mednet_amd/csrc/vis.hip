// Validation sample logging: everything `log_samples` (segmentation.py:67-92, landmarks.py:85-123) hands to
// imshow through vis_loglabels / vis_logheatmaps (utils/plots.py:45-127), computed on the device from ONE sample where its tensors
// lie.  Every source tensor is read once; no arg-max volume, soft-max or slice copy reaches HBM.
//   pred_mip            uint8  max over the axis of argmax_c logits[nh + c]   (first maximum on ties, like torch.argmax)
//   label_mip           uint8  max over the axis of the class map (uint8 / int64)
//   input_mip           fp32   mean | max over the axis of the first input channel
//   heatmap_mip         fp32   [nh] max over the axis of the target heat maps (uint8 / fp32)
//   output_heatmap_mip  fp32   [nh] max over the axis of the RAW heat-map outputs logits[k] (landmarks.py:94 does not clip)
// The volume is viewed as [A][R][B] with R the reduced extent: axis 0 = [1][D][H*W], axis 1 = [D][H][W], axis 2 = [D*H][W][1].
//   B > 1 (axes 0, 1): lanes run along B (coalesced, 4 elements per lane where alignment allows), R is cut into segments that
//                      separate workgroups reduce into a partial buffer; a second launch combines the segments in index order.
//   B = 1 (axis 2):    one wave per line of W contiguous elements, lanes stride through it, butterfly reduction across the wave.
// Both orders are fixed by the shape alone: no atomics, two calls give the same bits.
#include <math.h>

#include "common.h"

namespace mednet {

enum { VIS_PRED = 0, VIS_LABEL = 1, VIS_INPUT = 2, VIS_HEAT0 = 3 };  // job numbering; heat targets 3 .. 3 + nh - 1, then the outputs

struct VisArgs {
  const float* logits;    // channel 0 of the sample's output; plane k at + k * stride_c
  const void* labels;     // class map, R * A * B elements
  const void* heatmaps;   // nh dense planes
  const float* input;     // first input channel
  uint8_t* pred_mip;
  uint8_t* label_mip;
  float* input_mip;
  float* heatmap_mip;
  float* output_heatmap_mip;
  float* partial;         // [jobs][nseg][A * B]
  int64_t stride_c;
  size_t A, R, B;         // the [A][R][B] view; panels are [A][B]
  int nh, ncls, label_dtype, heatmap_dtype, mode;
  int nseg, seglen;       // segments of the reduced extent (strided form)
};

template <typename T, int VEC>
struct alignas(sizeof(T) * VEC) Pack {
  T v[VEC];
};
template <typename T, int VEC>
__device__ __forceinline__ Pack<T, VEC> ldv(const T* p, size_t i) {
  return *reinterpret_cast<const Pack<T, VEC>*>(p + i);
}

// the source of a job, or false if the job is switched off
__device__ __forceinline__ bool vis_job_on(const VisArgs& a, int job) {
  if (job == VIS_PRED) return a.pred_mip != nullptr;
  if (job == VIS_LABEL) return a.label_mip != nullptr;
  if (job == VIS_INPUT) return a.input_mip != nullptr;
  return job < VIS_HEAT0 + a.nh ? a.heatmap_mip != nullptr : a.output_heatmap_mip != nullptr;
}

// ---- element streams: acc[j] = reduce over the positions `first + i * step`, i < count, of VEC adjacent elements ------------
template <typename T, int VEC>
__device__ __forceinline__ void stream_max(const T* p, size_t first, size_t step, size_t count, float* acc) {
#pragma unroll 4
  for (size_t i = 0; i < count; ++i) {
    const Pack<T, VEC> v = ldv<T, VEC>(p, first + i * step);
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = fmaxf(acc[j], (float)v.v[j]);
  }
}
template <int VEC>
__device__ __forceinline__ void stream_sum(const float* p, size_t first, size_t step, size_t count, float* acc) {
#pragma unroll 4
  for (size_t i = 0; i < count; ++i) {
    const Pack<float, VEC> v = ldv<float, VEC>(p, first + i * step);
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] += v.v[j];
  }
}
// max over the positions of the arg-max over the class planes; the planes are read once, the class index lives in registers
// (NP positions per trip: the class loop has a run-time length, so the loads of one position wait for one another; NP positions
//  keep NP independent loads in flight per class plane)
template <int VEC, int NP>
__device__ __forceinline__ void argmax_max_block(const float* cls, int64_t stride_c, int ncls, size_t first, size_t step, float* acc) {
  Pack<float, VEC> bv[NP];
  int best[NP][VEC];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    bv[p] = ldv<float, VEC>(cls, first + p * step);
#pragma unroll
    for (int j = 0; j < VEC; ++j) best[p][j] = 0;
  }
  for (int k = 1; k < ncls; ++k) {
    const float* plane = cls + (int64_t)k * stride_c;
    Pack<float, VEC> v[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) v[p] = ldv<float, VEC>(plane, first + p * step);
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        if (v[p].v[j] > bv[p].v[j]) {  // strict: the first maximum wins
          bv[p].v[j] = v[p].v[j];
          best[p][j] = k;
        }
  }
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = fmaxf(acc[j], (float)best[p][j]);
}
template <int VEC>
__device__ __forceinline__ void stream_argmax_max(const float* cls, int64_t stride_c, int ncls, size_t first, size_t step,
                                                  size_t count, float* acc) {
  size_t i = 0;
  for (; i + 4 <= count; i += 4) argmax_max_block<VEC, 4>(cls, stride_c, ncls, first + i * step, step, acc);
  for (; i < count; ++i) argmax_max_block<VEC, 1>(cls, stride_c, ncls, first + i * step, step, acc);
}

// one job's reduction of one stream; acc must hold the identity on entry
template <int VEC>
__device__ __forceinline__ void vis_reduce(const VisArgs& a, int job, size_t first, size_t step, size_t count, float* acc) {
  const size_t plane = a.A * a.R * a.B;
  if (job == VIS_PRED) {
    stream_argmax_max<VEC>(a.logits + (int64_t)a.nh * a.stride_c, a.stride_c, a.ncls, first, step, count, acc);
  } else if (job == VIS_LABEL) {
    if (a.label_dtype == MEDNET_U8) stream_max<uint8_t, VEC>((const uint8_t*)a.labels, first, step, count, acc);
    else stream_max<int64_t, VEC>((const int64_t*)a.labels, first, step, count, acc);
  } else if (job == VIS_INPUT) {
    if (a.mode == MEDNET_MIP_MEAN) stream_sum<VEC>(a.input, first, step, count, acc);
    else stream_max<float, VEC>(a.input, first, step, count, acc);
  } else if (job < VIS_HEAT0 + a.nh) {
    const size_t k = (size_t)(job - VIS_HEAT0);
    if (a.heatmap_dtype == MEDNET_U8) stream_max<uint8_t, VEC>((const uint8_t*)a.heatmaps + k * plane, first, step, count, acc);
    else stream_max<float, VEC>((const float*)a.heatmaps + k * plane, first, step, count, acc);
  } else {
    stream_max<float, VEC>(a.logits + (int64_t)(job - VIS_HEAT0 - a.nh) * a.stride_c, first, step, count, acc);
  }
}

__device__ __forceinline__ float vis_identity(const VisArgs& a, int job) {
  if (job == VIS_PRED || job == VIS_LABEL) return 0.f;  // class indices are >= 0
  if (job == VIS_INPUT && a.mode == MEDNET_MIP_MEAN) return 0.f;
  return -INFINITY;
}
__device__ __forceinline__ bool vis_is_sum(const VisArgs& a, int job) { return job == VIS_INPUT && a.mode == MEDNET_MIP_MEAN; }

// the finished value `v` of panel element `o` of a job goes to its panel
__device__ __forceinline__ void vis_store(const VisArgs& a, int job, size_t o, float v) {
  const size_t panel = a.A * a.B;
  if (job == VIS_PRED) a.pred_mip[o] = (uint8_t)(int)v;
  else if (job == VIS_LABEL) a.label_mip[o] = (uint8_t)(int)v;
  else if (job == VIS_INPUT) a.input_mip[o] = vis_is_sum(a, job) ? v / (float)a.R : v;
  else if (job < VIS_HEAT0 + a.nh) a.heatmap_mip[(size_t)(job - VIS_HEAT0) * panel + o] = v;
  else a.output_heatmap_mip[(size_t)(job - VIS_HEAT0 - a.nh) * panel + o] = v;
}

// ---- axes 0 and 1: grid (column tiles, segments, jobs); a thread owns VEC adjacent columns of one segment ---------------------
template <int VEC>
__global__ __launch_bounds__(256) void vis_mip_strided_kernel(const VisArgs a) {
  const int job = blockIdx.z;
  if (!vis_job_on(a, job)) return;
  const size_t bv = a.B / VEC, col = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (col >= a.A * bv) return;
  const size_t ai = col / bv, b = (col % bv) * VEC;
  const size_t r0 = (size_t)blockIdx.y * a.seglen, r1 = r0 + a.seglen < a.R ? r0 + a.seglen : a.R;
  float acc[VEC];
  const float id = vis_identity(a, job);
#pragma unroll
  for (int j = 0; j < VEC; ++j) acc[j] = id;
  vis_reduce<VEC>(a, job, (ai * a.R + r0) * a.B + b, a.B, r1 - r0, acc);
  float* dst = a.partial + ((size_t)job * a.nseg + blockIdx.y) * (a.A * a.B) + ai * a.B + b;
#pragma unroll
  for (int j = 0; j < VEC; ++j) dst[j] = acc[j];
}

// segments in index order -> the panels; grid (panel tiles, jobs)
__global__ __launch_bounds__(256) void vis_mip_combine_kernel(const VisArgs a) {
  const int job = blockIdx.y;
  if (!vis_job_on(a, job)) return;
  const size_t panel = a.A * a.B, o = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= panel) return;
  const float* src = a.partial + (size_t)job * a.nseg * panel + o;
  float v = src[0];
  if (vis_is_sum(a, job)) {
    for (int s = 1; s < a.nseg; ++s) v += src[(size_t)s * panel];
  } else {
    for (int s = 1; s < a.nseg; ++s) v = fmaxf(v, src[(size_t)s * panel]);
  }
  vis_store(a, job, o, v);
}

// ---- axis 2: grid (lines / 4, jobs); one wave per line of R contiguous elements -----------------------------------------------
template <int VEC>
__global__ __launch_bounds__(256) void vis_mip_rows_kernel(const VisArgs a) {
  const int job = blockIdx.y;
  if (!vis_job_on(a, job)) return;
  const size_t line = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
  if (line >= a.A) return;
  const size_t lane = threadIdx.x & 63, nv = a.R / VEC;  // (VEC > 1 only when R % VEC == 0)
  float acc[VEC];
  const float id = vis_identity(a, job);
#pragma unroll
  for (int j = 0; j < VEC; ++j) acc[j] = id;
  const size_t count = lane < nv ? (nv - lane + 63) / 64 : 0;
  vis_reduce<VEC>(a, job, line * a.R + lane * VEC, (size_t)64 * VEC, count, acc);
  float v = acc[0];
  const bool sum = vis_is_sum(a, job);
#pragma unroll
  for (int j = 1; j < VEC; ++j) v = sum ? v + acc[j] : fmaxf(v, acc[j]);
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {  // butterfly: every lane ends with the same value, summed in the same order
    const float o = __shfl_xor(v, m, 64);
    v = sum ? v + o : fmaxf(v, o);
  }
  if (lane == 0) vis_store(a, job, line, v);
}

static inline bool aligned_to(const void* p, size_t bytes) { return ((uintptr_t)p % bytes) == 0; }

// segments of the reduced extent R for a panel of `cols` lane-columns: enough workgroups to fill the chip, never more than 64
static inline void vis_segments(size_t R, size_t cols, int* nseg, int* seglen) {
  size_t want = (65536 + cols - 1) / cols;
  if (want > 64) want = 64;
  if (want > R) want = R;
  if (want < 1) want = 1;
  const size_t len = (R + want - 1) / want;
  *seglen = (int)len;
  *nseg = (int)((R + len - 1) / len);
}

static inline void vis_view(int d, int h, int w, int axis, size_t* A, size_t* R, size_t* B) {
  if (axis == 0) *A = 1, *R = (size_t)d, *B = (size_t)h * w;
  else if (axis == 1) *A = (size_t)d, *R = (size_t)h, *B = (size_t)w;
  else *A = (size_t)d * h, *R = (size_t)w, *B = 1;
}

}  // namespace mednet

using namespace mednet;

extern "C" size_t mednet_sample_panels_ws_bytes(int d, int h, int w, int num_heatmaps, int axis) {
  if (d <= 0 || h <= 0 || w <= 0 || num_heatmaps < 0 || axis < 0 || axis > 1) return 0;  // (axis 2 reduces inside a wave)
  size_t A, R, B;
  vis_view(d, h, w, axis, &A, &R, &B);
  int nseg, seglen;
  vis_segments(R, A * ((B + 3) / 4), &nseg, &seglen);  // (the scalar form has more columns, never more segments)
  return (size_t)(VIS_HEAT0 + 2 * num_heatmaps) * nseg * A * B * sizeof(float);
}

extern "C" int mednet_sample_panels(const float* logits, int64_t stride_c, int num_heatmaps, int num_classes, const void* labels,
                                    int label_dtype, const void* heatmaps, int heatmap_dtype, const float* input,
                                    uint8_t* pred_mip, uint8_t* label_mip, float* input_mip, float* heatmap_mip,
                                    float* output_heatmap_mip, int d, int h, int w, int axis, int image_mode, void* ws,
                                    size_t ws_bytes, mednet_stream stream) {
  MEDNET_REQUIRE(d > 0 && h > 0 && w > 0, MEDNET_E_SHAPE, "sample_panels: bad volume %dx%dx%d", d, h, w);
  MEDNET_REQUIRE(axis >= 0 && axis <= 2, MEDNET_E_SHAPE, "sample_panels: mip axis %d (0, 1 or 2 of the D x H x W volume)", axis);
  MEDNET_REQUIRE(image_mode == MEDNET_MIP_MEAN || image_mode == MEDNET_MIP_MAX, MEDNET_E_UNSUPPORTED,
                 "sample_panels: image mode %d (MEDNET_MIP_MEAN or MEDNET_MIP_MAX)", image_mode);
  MEDNET_REQUIRE(num_heatmaps >= 0 && num_heatmaps <= 4096, MEDNET_E_SHAPE, "sample_panels: %d heat maps", num_heatmaps);
  const int nh = num_heatmaps;
  if (nh == 0) heatmap_mip = output_heatmap_mip = nullptr;
  MEDNET_REQUIRE(!pred_mip || (logits && num_classes >= 1 && num_classes <= 256), MEDNET_E_SHAPE,
                 "sample_panels: pred_mip needs the logits and 1..256 classes (got %d)", num_classes);
  MEDNET_REQUIRE(!output_heatmap_mip || logits, MEDNET_E_SHAPE, "sample_panels: output_heatmap_mip needs the logits");
  MEDNET_REQUIRE(!label_mip || (labels && (label_dtype == MEDNET_U8 || label_dtype == MEDNET_I64)), MEDNET_E_DTYPE,
                 "sample_panels: label_mip needs uint8 or int64 labels (dtype %d)", label_dtype);
  MEDNET_REQUIRE(!heatmap_mip || (heatmaps && (heatmap_dtype == MEDNET_U8 || heatmap_dtype == MEDNET_F32)), MEDNET_E_DTYPE,
                 "sample_panels: heatmap_mip needs uint8 or fp32 heat maps (dtype %d)", heatmap_dtype);
  MEDNET_REQUIRE(!input_mip || input, MEDNET_E_SHAPE, "sample_panels: input_mip needs the input");
  if (!pred_mip && !label_mip && !input_mip && !heatmap_mip && !output_heatmap_mip) return MEDNET_OK;

  VisArgs a;
  a.logits = logits, a.labels = labels, a.heatmaps = heatmaps, a.input = input;
  a.pred_mip = pred_mip, a.label_mip = label_mip, a.input_mip = input_mip, a.heatmap_mip = heatmap_mip;
  a.output_heatmap_mip = output_heatmap_mip, a.partial = (float*)ws, a.stride_c = stride_c;
  a.nh = nh, a.ncls = num_classes, a.label_dtype = label_dtype, a.heatmap_dtype = heatmap_dtype, a.mode = image_mode;
  vis_view(d, h, w, axis, &a.A, &a.R, &a.B);
  const unsigned jobs = (unsigned)(VIS_HEAT0 + 2 * nh);
  // 4 elements per lane: the vectorised extent and every plane start must be a multiple of 4 elements of each type read
  const size_t lanes_extent = axis == 2 ? a.R : a.B, plane = a.A * a.R * a.B;
  const bool uses_logits = pred_mip || output_heatmap_mip;
  const bool vec = lanes_extent % 4 == 0 && plane % 4 == 0 && (!uses_logits || (stride_c % 4 == 0 && aligned_to(logits, 16))) &&
                   (!label_mip || aligned_to(labels, label_dtype == MEDNET_U8 ? 4 : 32)) &&
                   (!heatmap_mip || aligned_to(heatmaps, heatmap_dtype == MEDNET_U8 ? 4 : 16)) &&
                   (!input_mip || aligned_to(input, 16));
  hipStream_t s = (hipStream_t)stream;
  if (axis == 2) {
    a.nseg = 1, a.seglen = (int)a.R;
    const dim3 grid((unsigned)((a.A + 3) / 4), jobs);
    if (vec) hipLaunchKernelGGL(vis_mip_rows_kernel<4>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(vis_mip_rows_kernel<1>, grid, dim3(256), 0, s, a);
    return check_launch("sample_panels");
  }
  const size_t cols = a.A * (vec ? a.B / 4 : a.B);
  vis_segments(a.R, a.A * ((a.B + 3) / 4), &a.nseg, &a.seglen);  // the same plan for both forms: what _ws_bytes sized
  const size_t need = (size_t)jobs * a.nseg * a.A * a.B * sizeof(float);
  MEDNET_REQUIRE(ws && ws_bytes >= need && aligned_to(ws, 4), MEDNET_E_WORKSPACE,
                 "sample_panels: workspace of %zu bytes, %zu needed", ws_bytes, need);
  const dim3 grid((unsigned)((cols + 255) / 256), (unsigned)a.nseg, jobs);
  if (vec) hipLaunchKernelGGL(vis_mip_strided_kernel<4>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(vis_mip_strided_kernel<1>, grid, dim3(256), 0, s, a);
  const int rc = check_launch("sample_panels");
  if (rc != MEDNET_OK) return rc;
  hipLaunchKernelGGL(vis_mip_combine_kernel, dim3((unsigned)((a.A * a.B + 255) / 256), jobs), dim3(256), 0, s, a);
  return check_launch("sample_panels (combine)");
}
