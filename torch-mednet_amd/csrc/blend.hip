// Blended sliding-window inference (additive to ABI 3): the accumulate-style stitch next to predict.hip's crop-stitch.
//   blend_accumulate  every patch adds window-weighted probabilities (or logits) and heat maps to fp32 accumulators over the whole
//                     volume, and its weights to a weight sum; overlapping windows, test-time mirroring
//   blend_finalize    one pass over the voxels: accumulators / weight sum -> uint8 result (the reference's layout), probabilities
//                     (fp32 / fp16), float heat maps
//   heatmap_peaks     per-channel maximum of the stitched float heat maps and its flat index (landmark positions)
// No atomics anywhere: every voxel of a launch has ONE owning thread, which adds the contributions in row order, so the same
// patches give the same bits whatever the batch size ("Blended inference").
#include "volume.h"

namespace mednet {

// does the patch of row j hold the volume voxel (gz, gy, gx)?  q: the voxel's coordinate inside that patch
__device__ __forceinline__ bool blend_covers(const int* __restrict__ pos, int j, int gz, int gy, int gx, int ov0, int ov1, int ov2,
                                             int pd, int ph, int pw, int& qz, int& qy, int& qx) {
  qz = gz - (pos[j * 3] - ov0);
  qy = gy - (pos[j * 3 + 1] - ov1);
  qx = gx - (pos[j * 3 + 2] - ov2);
  return qz >= 0 && qz < pd && qy >= 0 && qy < ph && qx >= 0 && qx < pw;
}

// One thread per (row, patch voxel), x fastest: a wave reads 64 consecutive logits of a patch line and touches 64 consecutive
// accumulators of a volume line (scalar 4-byte accesses: pos - ov gives a line no 16-byte alignment).  predict_assemble_kernel's
// ownership idiom, inverted: the thread leaves its voxel to any EARLIER row of the launch whose patch holds it; otherwise it owns the
// voxel and adds the contributions of every row j >= b that holds it, in row order.  Across launches stream order continues the
// same order, so a voxel's sums are taken in patch order whatever the batch size.
__global__ __launch_bounds__(256) void blend_accumulate_kernel(const float* __restrict__ logits, const int* __restrict__ pos,
                                                               float* __restrict__ acc, float* __restrict__ wsum,
                                                               const float* __restrict__ win0, const float* __restrict__ win1,
                                                               const float* __restrict__ win2, int nh, int ncls, int d, int h, int w,
                                                               int pd, int ph, int pw, int ov0, int ov1, int ov2, int mirror,
                                                               int class_mode) {
  const size_t pvox = (size_t)pd * ph * pw;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= pvox) return;
  const int b = blockIdx.y, batch = (int)gridDim.y;
  const auto [z, y, x] = voxel_zyx(i, ph, pw);
  const int gz = pos[b * 3] - ov0 + z, gy = pos[b * 3 + 1] - ov1 + y, gx = pos[b * 3 + 2] - ov2 + x;
  if (gz < 0 || gz >= d || gy < 0 || gy >= h || gx < 0 || gx >= w) return;  // padding in front, overhang behind
  int qz, qy, qx;
  for (int j = 0; j < b; ++j)
    if (blend_covers(pos, j, gz, gy, gx, ov0, ov1, ov2, pd, ph, pw, qz, qy, qx)) return;
  const size_t vox = (size_t)d * h * w, dst = ((size_t)gz * h + gy) * w + gx;
  float ws = wsum[dst];
  for (int j = b; j < batch; ++j) {
    if (!blend_covers(pos, j, gz, gy, gx, ov0, ov1, ov2, pd, ph, pw, qz, qy, qx)) continue;
    // the weight belongs to the UNMIRRORED patch coordinate; the logits of a mirrored pass are read at the reversed index (the flip back)
    const float wt = (win0[qz] * win1[qy]) * win2[qx];
    const int rz = (mirror & 1) ? pd - 1 - qz : qz, ry = (mirror & 2) ? ph - 1 - qy : qy, rx = (mirror & 4) ? pw - 1 - qx : qx;
    const float* src = logits + (size_t)j * (nh + ncls) * pvox + ((size_t)rz * ph + ry) * pw + rx;
    ws += wt;
    for (int k = 0; k < nh; ++k) acc[(size_t)k * vox + dst] = fmaf(wt, src[(size_t)k * pvox], acc[(size_t)k * vox + dst]);
    const float* cls = src + (size_t)nh * pvox;
    float* a = acc + (size_t)nh * vox + dst;
    if (class_mode == MEDNET_BLEND_LOGITS) {
      for (int k = 0; k < ncls; ++k) a[(size_t)k * vox] = fmaf(wt, cls[(size_t)k * pvox], a[(size_t)k * vox]);
    } else {  // one softmax per voxel per patch
      // (captures by value: by reference the compiler forms the plane addresses with four more instructions per thread)
      plane_softmax(ncls, [=](int k) { return cls[(size_t)k * pvox]; },
                    [=](int k, float p) { a[(size_t)k * vox] = fmaf(wt, p, a[(size_t)k * vox]); });
    }
  }
  wsum[dst] = ws;
}

// A probability is its fp32 value, stored as it is or rounded once to fp16.  The empty asm keeps that fp32 value a value of its own:
// hipcc otherwise folds `expf(..) * inv` and the fp16 store into one v_fma_mixlo_f16, which rounds the exact product, and the fp16
// output is then no longer the fp32 output rounded.
template <typename TP>
__device__ __forceinline__ void st_prob(TP* p, size_t i, float v) {
  asm volatile("" : "+v"(v));
  st(p, i, v);
}

template <typename TP>
__global__ __launch_bounds__(256) void blend_finalize_kernel(const float* __restrict__ acc, const float* __restrict__ wsum,
                                                             uint8_t* __restrict__ result, TP* __restrict__ prob,
                                                             float* __restrict__ heat, int nh, int ncls, size_t vox, int class_mode) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= vox) return;
  const float ws = wsum[i];
  const bool live = ws != 0.f;  // (grid_positions' grid covers every voxel; an uncovered one reads 0, not NaN)
  for (int k = 0; k < nh; ++k) {
    const float v = live ? acc[(size_t)k * vox + i] / ws : 0.f;
    if (heat) heat[(size_t)k * vox + i] = v;
    if (result) result[(size_t)k * vox + i] = heat_to_u8(v);
  }
  const float* a = acc + (size_t)nh * vox + i;
  // arg-max of the class accumulators (softmax and the division by ws > 0 keep the order)
  if (result) result[(size_t)nh * vox + i] = (uint8_t)(live ? argmax_first(a, vox, ncls) : 0);
  if (!prob) return;
  if (!live) {
    for (int k = 0; k < ncls; ++k) st(prob, (size_t)k * vox + i, 0.f);
  } else if (class_mode == MEDNET_BLEND_LOGITS) {  // softmax of the blended logits
    plane_softmax(ncls, [&](int k) { return a[(size_t)k * vox] / ws; }, [&](int k, float p) { st_prob(prob, (size_t)k * vox + i, p); });
  } else {
    for (int k = 0; k < ncls; ++k) st_prob(prob, (size_t)k * vox + i, a[(size_t)k * vox] / ws);
  }
}

// ---- heat-map peaks: the larger value wins, the lower index on ties; a NaN never enters (every comparison with it is false)
struct Peak {
  float v;
  long long i;
};
constexpr long long PEAK_NONE = 0x7fffffffffffffffLL;  // nothing seen yet (a channel of NaNs only ends as index -1, value -inf)

__device__ __forceinline__ Peak peak_better(Peak a, Peak b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }
__device__ __forceinline__ int peak_lo(long long i) { return (int)(unsigned)(i & 0xffffffffLL); }
__device__ __forceinline__ int peak_hi(long long i) { return (int)(i >> 32); }
__device__ __forceinline__ long long peak_idx(int hi, int lo) { return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo); }
template <int CTRL>
__device__ __forceinline__ Peak peak_dpp(Peak p) {  // the reduction steps of lane_class_sum (common.h) with peak_better for +
  Peak o;
  o.v = dpp_f32<CTRL>(p.v);
  o.i = peak_idx(__builtin_amdgcn_update_dpp(0, peak_hi(p.i), CTRL, 0xF, 0xF, true),
                 __builtin_amdgcn_update_dpp(0, peak_lo(p.i), CTRL, 0xF, 0xF, true));
  return peak_better(p, o);
}
// xor16_sum / xor32_sum's swap: fed the value and a copy, one register ends up with the even rows' (lower half's) value in both
// places and the other with the odd rows' (upper half's); peak_better of the two is the same in both lanes of a pair
#define MEDNET_PEAK_SWAP(NAME, INSN)                                                        \
  __device__ __forceinline__ Peak NAME(Peak p) {                                            \
    float av = p.v, bv = p.v;                                                               \
    int alo = peak_lo(p.i), blo = alo, ahi = peak_hi(p.i), bhi = ahi;                       \
    MEDNET_SWAP_PAIR(INSN, av, bv);                                                         \
    MEDNET_SWAP_PAIR(INSN, alo, blo);                                                       \
    MEDNET_SWAP_PAIR(INSN, ahi, bhi);                                                       \
    return peak_better(Peak{av, peak_idx(ahi, alo)}, Peak{bv, peak_idx(bhi, blo)});         \
  }
MEDNET_PEAK_SWAP(peak_xor16, "v_permlane16_swap_b32")
MEDNET_PEAK_SWAP(peak_xor32, "v_permlane32_swap_b32")
#undef MEDNET_PEAK_SWAP

// best of a 256-thread workgroup, valid in thread 0; all lanes active
__device__ __forceinline__ Peak peak_block(Peak p) {
  p = peak_dpp<0xB1>(p);
  p = peak_dpp<0x4E>(p);
  p = peak_dpp<0x124>(p);
  p = peak_dpp<0x128>(p);
  p = peak_xor16(p);
  p = peak_xor32(p);
  __shared__ float sv[4];
  __shared__ long long si[4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
    sv[wid] = p.v;
    si[wid] = p.i;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 1; k < 4; ++k) p = peak_better(p, Peak{sv[k], si[k]});
  return p;
}

// stage 1: block (x, channel) scans VOLUME_PER_ROW voxels of its channel -> one partial
__global__ __launch_bounds__(256) void heatmap_peaks_partial_kernel(const float* __restrict__ heat, size_t vox, unsigned blocks,
                                                                    long long* __restrict__ pidx, float* __restrict__ pval) {
  const int k = blockIdx.y;
  size_t i0, i1;
  row_range(vox, VOLUME_PER_ROW, i0, i1);
  Peak p{-__builtin_inff(), PEAK_NONE};
  for (size_t i = i0 + threadIdx.x; i < i1; i += 256) p = peak_better(p, Peak{heat[(size_t)k * vox + i], (long long)i});
  p = peak_block(p);
  if (threadIdx.x == 0) {
    pidx[(size_t)k * blocks + blockIdx.x] = p.i;
    pval[(size_t)k * blocks + blockIdx.x] = p.v;
  }
}

// stage 2: one workgroup per channel over its partials
__global__ __launch_bounds__(256) void heatmap_peaks_final_kernel(const long long* __restrict__ pidx, const float* __restrict__ pval,
                                                                  unsigned blocks, long long* __restrict__ out_index,
                                                                  float* __restrict__ out_value) {
  const int k = blockIdx.x;
  Peak p{-__builtin_inff(), PEAK_NONE};
  for (unsigned j = threadIdx.x; j < blocks; j += 256) p = peak_better(p, Peak{pval[(size_t)k * blocks + j], pidx[(size_t)k * blocks + j]});
  p = peak_block(p);
  if (threadIdx.x == 0) {
    out_index[k] = p.i == PEAK_NONE ? -1 : p.i;
    out_value[k] = p.v;
  }
}

}  // namespace mednet

using namespace mednet;

static int class_mode_check(const char* who, int class_mode) {
  MEDNET_REQUIRE(class_mode == MEDNET_BLEND_PROBABILITIES || class_mode == MEDNET_BLEND_LOGITS, MEDNET_E_UNSUPPORTED,
                 "%s: class mode %d (supported: 0 probabilities, 1 logits)", who, class_mode);
  return MEDNET_OK;
}

extern "C" int mednet_blend_accumulate(const float* logits, const int* pos, float* acc, float* wsum, const float* win0,
                                       const float* win1, const float* win2, int batch, int num_heatmaps, int num_classes, int d,
                                       int h, int w, int pd, int ph, int pw, int ov0, int ov1, int ov2, int mirror, int class_mode,
                                       mednet_stream stream) {
  MEDNET_REQUIRE(logits && pos && acc && wsum && win0 && win1 && win2, MEDNET_E_SHAPE, "blend_accumulate: null pointer");
  MEDNET_REQUIRE(batch > 0 && batch <= 65535 && num_heatmaps >= 0 && num_classes >= 1 && d > 0 && h > 0 && w > 0 && pd > 0 && ph > 0 &&
                     pw > 0 && ov0 >= 0 && ov1 >= 0 && ov2 >= 0,
                 MEDNET_E_SHAPE, "blend_accumulate: bad shape (batch %d, channels %d + %d, volume %dx%dx%d, patch %dx%dx%d, overlap %d %d %d)",
                 batch, num_heatmaps, num_classes, d, h, w, pd, ph, pw, ov0, ov1, ov2);
  if (const int rc = mirror_check("blend_accumulate", mirror)) return rc;
  if (const int rc = class_mode_check("blend_accumulate", class_mode)) return rc;
  hipLaunchKernelGGL(blend_accumulate_kernel, dim3(grid_blocks((size_t)pd * ph * pw, 256), batch), dim3(256), 0, (hipStream_t)stream, logits, pos,
                     acc, wsum, win0, win1, win2, num_heatmaps, num_classes, d, h, w, pd, ph, pw, ov0, ov1, ov2, mirror, class_mode);
  return check_launch("blend_accumulate");
}

extern "C" int mednet_blend_finalize(const float* acc, const float* wsum, uint8_t* result_u8, void* prob, int prob_dtype, float* heat,
                                     int num_heatmaps, int num_classes, int d, int h, int w, int class_mode, mednet_stream stream) {
  MEDNET_REQUIRE(acc && wsum, MEDNET_E_SHAPE, "blend_finalize: null pointer");
  MEDNET_REQUIRE(result_u8 || prob || heat, MEDNET_E_SHAPE, "blend_finalize: no output asked for (result, prob and heat are all null)");
  MEDNET_REQUIRE(num_heatmaps >= 0 && num_classes >= 1 && d > 0 && h > 0 && w > 0, MEDNET_E_SHAPE,
                 "blend_finalize: bad shape (channels %d + %d, volume %dx%dx%d)", num_heatmaps, num_classes, d, h, w);
  MEDNET_REQUIRE(!prob || prob_dtype == MEDNET_F32 || prob_dtype == MEDNET_F16, MEDNET_E_DTYPE,
                 "blend_finalize: probability type %d (supported: f32, f16)", prob_dtype);
  if (const int rc = class_mode_check("blend_finalize", class_mode)) return rc;
  const size_t vox = (size_t)d * h * w;
  const dim3 grid(grid_blocks(vox, 256));
  hipStream_t s = (hipStream_t)stream;
  if (prob && prob_dtype == MEDNET_F16)
    hipLaunchKernelGGL(blend_finalize_kernel<f16>, grid, dim3(256), 0, s, acc, wsum, result_u8, (f16*)prob, heat, num_heatmaps, num_classes,
                       vox, class_mode);
  else
    hipLaunchKernelGGL(blend_finalize_kernel<float>, grid, dim3(256), 0, s, acc, wsum, result_u8, (float*)prob, heat, num_heatmaps,
                       num_classes, vox, class_mode);
  return check_launch("blend_finalize");
}

extern "C" size_t mednet_heatmap_peaks_ws_bytes(int num_heatmaps, size_t voxels) {
  if (num_heatmaps <= 0 || voxels == 0) return 0;
  return (size_t)num_heatmaps * grid_blocks(voxels, VOLUME_PER_ROW) * (sizeof(long long) + sizeof(float));
}

extern "C" int mednet_heatmap_peaks(const float* heat, int num_heatmaps, size_t voxels, int64_t* out_index, float* out_value, void* ws,
                                    size_t ws_bytes, mednet_stream stream) {
  MEDNET_REQUIRE(heat && out_index && out_value && ws, MEDNET_E_SHAPE, "heatmap_peaks: null pointer");
  MEDNET_REQUIRE(num_heatmaps > 0 && num_heatmaps <= 65535 && voxels > 0, MEDNET_E_SHAPE, "heatmap_peaks: bad shape (%d channels, %zu voxels)",
                 num_heatmaps, voxels);
  MEDNET_REQUIRE(ws_bytes >= mednet_heatmap_peaks_ws_bytes(num_heatmaps, voxels), MEDNET_E_WORKSPACE,
                 "heatmap_peaks: workspace %zu < %zu bytes", ws_bytes, mednet_heatmap_peaks_ws_bytes(num_heatmaps, voxels));
  MEDNET_REQUIRE((uintptr_t)ws % sizeof(long long) == 0, MEDNET_E_WORKSPACE, "heatmap_peaks: workspace not 8-byte aligned");
  const size_t blocks = grid_blocks(voxels, VOLUME_PER_ROW);
  long long* pidx = (long long*)ws;
  float* pval = (float*)(pidx + (size_t)num_heatmaps * blocks);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(heatmap_peaks_partial_kernel, dim3((unsigned)blocks, num_heatmaps), dim3(256), 0, s, heat, voxels, (unsigned)blocks,
                     pidx, pval);
  const int rc = check_launch("heatmap_peaks(partials)");
  if (rc != MEDNET_OK) return rc;
  hipLaunchKernelGGL(heatmap_peaks_final_kernel, dim3(num_heatmaps), dim3(256), 0, s, (const long long*)pidx, (const float*)pval,
                     (unsigned)blocks, (long long*)out_index, out_value);
  return check_launch("heatmap_peaks");
}
