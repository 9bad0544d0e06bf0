// Fused per-voxel losses: soft Dice, weighted cross-entropy, weighted heat-map regression.
//
// The reference builds Dice from ~8 full-size intermediates (softmax, one-hot, two permuted copies, product, sums:
// loss.py:116,81-86,10-21,43-47).  Here forward is ONE pass over logits+labels that keeps the per-channel sums in
// registers, and backward is ONE pass using the closed form
//     dL/dp[c,v] = mask * ( -2 w_c t / (C D'_c) + 2 w_c I_c [D_c >= eps] / (C D'_c^2) ),  D' = max(D, eps)
//     softmax: dL/dz_c = p_c (g_c - sum_k p_k g_k)      sigmoid: dL/dz_c = g_c p_c (1 - p_c)
// Logits are planar fp32 (NCDHW or a channel slice of it: element strides stride_n/stride_c, unit voxel stride), so a
// wave reads 64 consecutive voxels of each channel plane: C coalesced 256-B rows per wave-instruction group.
#include <limits.h>
#include "common.h"
#include "conv.h"
#include "loss_blocks.inc"

namespace mednet {

constexpr int LOSS_BLOCK_VOX = 256 * 8;  // voxels per workgroup

static inline unsigned loss_blocks(size_t spatial) { return (unsigned)((spatial + LOSS_BLOCK_VOX - 1) / LOSS_BLOCK_VOX); }

// ---- the class losses: DiceLoss, weighted nn.CrossEntropyLoss, and their sum in one pass each way (KIND = MEDNET_CLASS_*) ---------
// One kernel pair; the per-voxel arithmetic is loss_blocks.inc's, which the fused heads of head_loss.hip run too.
//   Dice       partial[n][block][c][2] = {sum p*t*mask, sum (p+t)*mask};  `weight` unused
//   CE         partial[n][block][2] = {sum w_y * nll, sum w_y};  `sigmoid` unused
//   Dice + CE  (softmax only, no ignore_index) the Dice rows [n][block][c][2], then the CE rows [n][block][2]
// (the label is made opaque once it is an int: left alone, a uint8 label is compared with every class as the byte it was, against
//  constants held in one VGPR per class -- 6 registers and a wave per SIMD at 8 classes)
template <int KIND, int MAXC, typename TL>
__global__ __launch_bounds__(256) void class_loss_fwd_kernel(const float* __restrict__ lg, const TL* __restrict__ lab, int64_t lab_sn,
                                                             const float* __restrict__ weight, float* __restrict__ partial, int c,
                                                             size_t spatial, int64_t sn, int64_t sc, int sigmoid, int ignore) {
  __shared__ float scratch[4];
  const int n = blockIdx.y;
  ClassSums<MAXC> sums;
  const size_t v0 = (size_t)blockIdx.x * LOSS_BLOCK_VOX;
  for (int it = 0; it < 8; ++it) {
    const size_t v = v0 + (size_t)it * 256 + threadIdx.x;
    if (v < spatial) {
      const size_t base = (size_t)n * sn + v;
      int y = label_at(lab, (size_t)n * lab_sn + v, ignore);
      asm volatile("" : "+v"(y));  // (a 32-bit value of its own: the note above the kernel)
      class_fwd_voxel<KIND, MAXC>(sums, [&](int k) { return lg[base + (size_t)k * sc]; }, y, c, sigmoid, ignore, weight);
    }
  }
  class_fwd_writeout<KIND, MAXC>(sums, partial, c, scratch);
}

// single workgroup: fp64 fixed-order combine, then the scalar.  dice_combine: the combine of the Dice rows (on thread 0 -> mean(1 - dice)),
// shared by dice_finalize_kernel and dice_ce_finalize_kernel; it ends on a barrier, so `sh` is free again when it returns
__device__ __forceinline__ float dice_combine(const float* __restrict__ partial, const float* __restrict__ weight,
                                              float* __restrict__ saved, float* __restrict__ dice_out, int c, int nblocks, float eps,
                                              double (*sh)[256], double* dice_s) {
  for (int k = 0; k < c; ++k) {
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) {
      a += (double)partial[((size_t)i * c + k) * 2];
      b += (double)partial[((size_t)i * c + k) * 2 + 1];
    }
    sh[0][threadIdx.x] = a;
    sh[1][threadIdx.x] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) {
        sh[0][threadIdx.x] += sh[0][threadIdx.x + s];
        sh[1][threadIdx.x] += sh[1][threadIdx.x + s];
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const float I = (float)sh[0][0], D = (float)sh[1][0];
      saved[2 * k] = I;
      saved[2 * k + 1] = D;
      const float wI = weight ? weight[k] * I : I;
      const float dice = 2.f * wI / fmaxf(D, eps);
      if (dice_out) dice_out[k] = dice;
      dice_s[k] = (double)(1.f - dice);
    }
    __syncthreads();
  }
  float s = 0.f;
  if (threadIdx.x == 0) {
    for (int k = 0; k < c; ++k) s += (float)dice_s[k];
    s = s / (float)c;
  }
  return s;
}
__global__ __launch_bounds__(256) void dice_finalize_kernel(const float* __restrict__ partial,
                                                            const float* __restrict__ weight, float* __restrict__ loss,
                                                            float* __restrict__ saved, float* __restrict__ dice_out,
                                                            int c, int nblocks, float eps) {
  __shared__ double sh[2][256];
  __shared__ double dice_s[64];
  const float s = dice_combine(partial, weight, saved, dice_out, c, nblocks, eps, sh, dice_s);
  if (threadIdx.x == 0 && loss) *loss = s;
}

// one store per logit; saved = [c][2] {I, D} (Dice forms), then sum w_y (CE forms), as the finalize kernels leave them
template <int KIND, int MAXC, typename TL>
__global__ __launch_bounds__(256) void class_loss_bwd_kernel(const float* __restrict__ lg, const TL* __restrict__ lab, int64_t lab_sn,
                                                             const float* __restrict__ weight, const float* __restrict__ saved,
                                                             const float* __restrict__ dloss, float* __restrict__ dlg, int c,
                                                             size_t spatial, int64_t sn, int64_t sc, float eps, int sigmoid, int ignore) {
  const int n = blockIdx.y;
  ClassCoefRegs<MAXC> coef;
  coef.template fill<KIND>(c, weight, saved, eps, *dloss);
  const size_t v0 = (size_t)blockIdx.x * LOSS_BLOCK_VOX;
  for (int it = 0; it < 8; ++it) {
    const size_t v = v0 + (size_t)it * 256 + threadIdx.x;
    if (v < spatial) {
      const size_t base = (size_t)n * sn + v;
      int y = label_at(lab, (size_t)n * lab_sn + v, ignore);
      asm volatile("" : "+v"(y));  // (as in class_loss_fwd_kernel)
      float p[MAXC];
#pragma unroll
      for (int k = 0; k < MAXC; ++k)
        if (k < c) p[k] = lg[base + (size_t)k * sc];
      class_logit_grad<KIND, MAXC>(p, y, c, sigmoid, ignore, coef);
#pragma unroll
      for (int k = 0; k < MAXC; ++k)
        if (k < c) dlg[base + (size_t)k * sc] = p[k];
    }
  }
}

// the combine of the CE rows (on thread 0: saved_w[0] = sum w_y, -> sum w_y nll / sum w_y), shared like dice_combine
__device__ __forceinline__ float ce_combine(const float* __restrict__ partial, float* __restrict__ saved_w, int nblocks,
                                            double (*sh)[256]) {
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 256) {
    a += (double)partial[2 * (size_t)i];
    b += (double)partial[2 * (size_t)i + 1];
  }
  sh[0][threadIdx.x] = a;
  sh[1][threadIdx.x] = b;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + s];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return 0.f;
  saved_w[0] = (float)sh[1][0];
  return (float)(sh[0][0] / sh[1][0]);
}
__global__ __launch_bounds__(256) void ce_finalize_kernel(const float* __restrict__ partial, float* __restrict__ loss,
                                                          float* __restrict__ saved, int nblocks) {
  __shared__ double sh[2][256];
  const float s = ce_combine(partial, saved, nblocks, sh);
  if (threadIdx.x == 0) *loss = s;
}
// saved = [c][2] {I, D}, then sum w_y;  loss = fl(dice + ce), one rounded fp32 add of the two finalised terms
__global__ __launch_bounds__(256) void dice_ce_finalize_kernel(const float* __restrict__ partial, const float* __restrict__ partial_ce,
                                                               const float* __restrict__ weight, float* __restrict__ loss,
                                                               float* __restrict__ saved, float* __restrict__ dice_out, int c,
                                                               int nblocks, float eps) {
  __shared__ double sh[2][256];
  __shared__ double dice_s[64];
  const float dice = dice_combine(partial, weight, saved, dice_out, c, nblocks, eps, sh, dice_s);
  const float ce = ce_combine(partial_ce, saved + 2 * c, nblocks, sh);
  if (threadIdx.x == 0) *loss = dice + ce;
}
// ---- heat-map regression: partial[(n*c + ch)][block] = sum f(out - tgt) -----------------------------------------
template <typename TT>
__global__ __launch_bounds__(256) void hm_fwd_kernel(const float* __restrict__ out, const TT* __restrict__ tgt, int64_t tgt_sn,
                                                     float* __restrict__ partial, int c, size_t spatial, int64_t sn,
                                                     int64_t sc, int kind) {
  __shared__ float scratch[4];
  const int ch = blockIdx.y, n = blockIdx.z;
  float s = 0.f;
  const size_t v0 = (size_t)blockIdx.x * LOSS_BLOCK_VOX;
  for (int it = 0; it < 8; ++it) {
    const size_t v = v0 + (size_t)it * 256 + threadIdx.x;
    if (v < spatial) {
      const float d = out[(size_t)n * sn + (size_t)ch * sc + v] - ld(tgt, (size_t)n * tgt_sn + (size_t)ch * spatial + v);
      s += kind == MEDNET_REG_L2 ? d * d : fabsf(d);
    }
  }
  s = block_sum<4>(s, scratch);
  if (threadIdx.x == 0) partial[((size_t)n * c + ch) * gridDim.x + blockIdx.x] = s;
}
// loss = sum_c w_c * (sum over n, blocks) / (N * spatial)   -- landmarks.py:129-132 evaluates channel by channel
// (16 waves, a wave per channel, four loads in flight per lane, one barrier: as one 256-thread loop over the channels with an LDS
//  tree per channel this was 111 us for the 16 heat maps)
__global__ __launch_bounds__(1024) void hm_finalize_kernel(const float* __restrict__ partial,
                                                           const float* __restrict__ cweight, float* __restrict__ loss,
                                                           int n, int c, int nblocks, double count) {
  __shared__ double chsum[256];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int ch0 = 0; ch0 < c; ch0 += 256) {  // (more than 256 channels: in rounds; the order of the final sum stays 0 .. c-1)
    for (int ch = ch0 + wv; ch < c && ch < ch0 + 256; ch += 16) {
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
      for (int nn = 0; nn < n; ++nn) {
        const float* p = partial + ((size_t)nn * c + ch) * nblocks;
        int b = lane;
        for (; b + 192 < nblocks; b += 256) {
          a0 += (double)p[b];
          a1 += (double)p[b + 64];
          a2 += (double)p[b + 128];
          a3 += (double)p[b + 192];
        }
        for (; b < nblocks; b += 64) a0 += (double)p[b];
      }
      const double a = wave_sum((a0 + a1) + (a2 + a3));
      if (lane == 0) chsum[ch - ch0] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      float total = ch0 ? *loss : 0.f;
      for (int ch = ch0; ch < c && ch < ch0 + 256; ++ch) total += (cweight ? cweight[ch] : 1.f) * (float)(chsum[ch - ch0] / count);
      *loss = total;
    }
    __syncthreads();
  }
}
template <typename TT>
__global__ __launch_bounds__(256) void hm_bwd_kernel(const float* __restrict__ out, const TT* __restrict__ tgt, int64_t tgt_sn,
                                                     const float* __restrict__ cweight, const float* __restrict__ dloss,
                                                     float* __restrict__ dout, int c, size_t spatial, int64_t sn,
                                                     int64_t sc, int kind, float inv_count) {
  const int ch = blockIdx.y, n = blockIdx.z;
  const float scale = *dloss * (cweight ? cweight[ch] : 1.f) * inv_count;
  const size_t v0 = (size_t)blockIdx.x * LOSS_BLOCK_VOX;
  for (int it = 0; it < 8; ++it) {
    const size_t v = v0 + (size_t)it * 256 + threadIdx.x;
    if (v < spatial) {
      const size_t o = (size_t)n * tgt_sn + (size_t)ch * spatial + v, os = (size_t)n * sn + (size_t)ch * sc + v;
      const float d = out[os] - ld(tgt, o);
      dout[os] = kind == MEDNET_REG_L2 ? 2.f * d * scale : (d > 0.f ? scale : (d < 0.f ? -scale : 0.f));
    }
  }
}

// (for head_mfma.hip's fused landmark head, whose partial sums have hm_fwd_kernel's / class_loss_fwd_kernel<DICE>'s layouts)
int launch_hm_finalize(const float* partial, const float* cweight, float* loss, int n, int c, int nblocks, size_t spatial,
                       hipStream_t s) {
  hipLaunchKernelGGL(hm_finalize_kernel, dim3(1), dim3(1024), 0, s, partial, cweight, loss, n, c, nblocks, (double)n * (double)spatial);
  return check_launch("heatmap_loss_finalize");
}
int launch_dice_finalize(const float* partial, const float* weight, float* loss, float* saved, int c, int nblocks, float eps,
                         hipStream_t s, float* dice_out) {
  hipLaunchKernelGGL(dice_finalize_kernel, dim3(1), dim3(256), 0, s, partial, weight, loss, saved, dice_out, c, nblocks, eps);
  return check_launch("dice_finalize");
}
// (for the fused CE heads, head_loss.hip / head_mfma.hip, whose partial rows have class_loss_fwd_kernel<CE>'s layout)
int launch_ce_finalize(const float* partial, float* loss, float* saved, int nblocks, hipStream_t s) {
  hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(256), 0, s, partial, loss, saved, nblocks);
  return check_launch("ce_finalize");
}
// (for the fused Dice + CE heads: Dice rows in class_loss_fwd_kernel<DICE>'s layout, CE rows in class_loss_fwd_kernel<CE>'s)
int launch_dice_ce_finalize(const float* partial, const float* partial_ce, const float* weight, float* loss, float* saved, int c,
                            int nblocks, float eps, hipStream_t s, float* dice_out) {
  hipLaunchKernelGGL(dice_ce_finalize_kernel, dim3(1), dim3(256), 0, s, partial, partial_ce, weight, loss, saved, dice_out, c, nblocks, eps);
  return check_launch("dice_ce_finalize");
}
int launch_class_finalize(int kind, const float* dice_partial, const float* ce_partial, const float* weight, float* loss, float* saved,
                          int c, int rows, float eps, hipStream_t s) {
  if (kind == MEDNET_CLASS_DICE_CE) return launch_dice_ce_finalize(dice_partial, ce_partial, weight, loss, saved, c, rows, eps, s, nullptr);
  if (kind == MEDNET_CLASS_CE) return launch_ce_finalize(ce_partial, loss, saved, rows, s);
  return launch_dice_finalize(dice_partial, weight, loss, saved, c, rows, eps, s, nullptr);
}

}  // namespace mednet

using namespace mednet;

extern "C" size_t mednet_loss_ws_bytes(int n, int c, size_t spatial) {
  return ((size_t)n * loss_blocks(spatial) * c * 2 + 64) * sizeof(float);
}

#define LOSS_DISPATCH_C(c, CALL)       \
  do {                                 \
    if ((c) <= 2) { CALL(2); }         \
    else if ((c) <= 4) { CALL(4); }    \
    else if ((c) <= 8) { CALL(8); }    \
    else if ((c) <= 16) { CALL(16); }  \
    else { CALL(32); }                 \
  } while (0)

// The one launch per direction of the stand-alone class losses: kind -> KIND, C -> MAXC, label type -> TL.  The entry points below
// keep their own argument checks.  labels: MEDNET_I64 (N x spatial, the reference's `.long()`) or MEDNET_U8, element stride
// label_stride_n between samples (the last channel of a uint8 label volume is consumed where it lies: no cast kernel,
// landmarks.py:70 / segmentation.py:60); the CE entry points take int64 labels only, so CE has no uint8 instantiation.
#define CLASS_LOSS_LAUNCH(KERNEL, KIND, M, ...)                                                                               \
  do {                                                                                                                        \
    if constexpr (KIND != MEDNET_CLASS_CE) {                                                                                  \
      if (label_dtype == MEDNET_U8) {                                                                                         \
        hipLaunchKernelGGL((KERNEL<KIND, M, uint8_t>), dim3(nb, n), dim3(256), 0, s, logits, (const uint8_t*)labels, label_stride_n, __VA_ARGS__); \
        break;                                                                                                                \
      }                                                                                                                       \
    }                                                                                                                         \
    hipLaunchKernelGGL((KERNEL<KIND, M, int64_t>), dim3(nb, n), dim3(256), 0, s, logits, (const int64_t*)labels, label_stride_n, __VA_ARGS__); \
  } while (0)

static int class_loss_fwd(const char* what, int kind, const float* logits, const void* labels, int label_dtype, int64_t label_stride_n,
                          const float* weight, float* loss, float* saved, float* dice_out, int n, int c, size_t spatial,
                          int64_t stride_n, int64_t stride_c, float eps, int sigmoid, int ignore_index, void* ws, mednet_stream stream) {
  hipStream_t s = (hipStream_t)stream;
  const unsigned nb = loss_blocks(spatial);
  float* partial = (float*)ws;
  for_class_kind(kind, [&](auto kind_c) {
    constexpr int KIND = decltype(kind_c)::value;
#define CALL(M) CLASS_LOSS_LAUNCH(class_loss_fwd_kernel, KIND, M, weight, partial, c, spatial, stride_n, stride_c, sigmoid, ignore_index)
    LOSS_DISPATCH_C(c, CALL);
#undef CALL
  });
  int rc = check_launch(what);
  if (rc) return rc;
  const int rows = (int)(nb * n);
  if (kind == MEDNET_CLASS_DICE_CE) return launch_dice_ce_finalize(partial, partial + (size_t)rows * c * 2, weight, loss, saved, c, rows, eps, s, dice_out);
  if (kind == MEDNET_CLASS_CE) return launch_ce_finalize(partial, loss, saved, rows, s);
  return launch_dice_finalize(partial, weight, loss, saved, c, rows, eps, s, dice_out);
}

static int class_loss_bwd(const char* what, int kind, const float* logits, const void* labels, int label_dtype, int64_t label_stride_n,
                          const float* weight, const float* saved, const float* dloss, float* dlogits, int n, int c, size_t spatial,
                          int64_t stride_n, int64_t stride_c, float eps, int sigmoid, int ignore_index, mednet_stream stream) {
  hipStream_t s = (hipStream_t)stream;
  const unsigned nb = loss_blocks(spatial);
  for_class_kind(kind, [&](auto kind_c) {
    constexpr int KIND = decltype(kind_c)::value;
#define CALL(M) CLASS_LOSS_LAUNCH(class_loss_bwd_kernel, KIND, M, weight, saved, dloss, dlogits, c, spatial, stride_n, stride_c, eps, sigmoid, ignore_index)
    LOSS_DISPATCH_C(c, CALL);
#undef CALL
  });
  return check_launch(what);
}
#undef CLASS_LOSS_LAUNCH

extern "C" int mednet_dice_fwd_lt(const float* logits, const void* labels, int label_dtype, int64_t label_stride_n, const float* weight,
                                  float* loss, float* saved, float* dice_out, int n, int c, size_t spatial, int64_t stride_n,
                                  int64_t stride_c, float eps, int sigmoid, int ignore_index, void* ws, size_t ws_bytes,
                                  mednet_stream stream) {
  MEDNET_REQUIRE(c >= 1 && c <= 32, MEDNET_E_UNSUPPORTED, "dice_fwd: C=%d (supported: 1..32)", c);
  MEDNET_REQUIRE(n > 0 && spatial > 0, MEDNET_E_SHAPE, "dice_fwd: empty input");
  MEDNET_REQUIRE(label_dtype == MEDNET_I64 || label_dtype == MEDNET_U8, MEDNET_E_DTYPE, "dice_fwd: labels are int64 or uint8 (got %d)", label_dtype);
  MEDNET_REQUIRE(ws_bytes >= mednet_loss_ws_bytes(n, c, spatial), MEDNET_E_WORKSPACE, "dice_fwd: workspace too small");
  return class_loss_fwd("dice_fwd", MEDNET_CLASS_DICE, logits, labels, label_dtype, label_stride_n, weight, loss, saved, dice_out, n, c,
                        spatial, stride_n, stride_c, eps, sigmoid, ignore_index, ws, stream);
}
extern "C" int mednet_dice_fwd(const float* logits, const int64_t* labels, const float* weight, float* loss,
                               float* saved, float* dice_out, int n, int c, size_t spatial, int64_t stride_n,
                               int64_t stride_c, float eps, int sigmoid, int ignore_index, void* ws, size_t ws_bytes,
                               mednet_stream stream) {
  return mednet_dice_fwd_lt(logits, labels, MEDNET_I64, (int64_t)spatial, weight, loss, saved, dice_out, n, c, spatial, stride_n, stride_c,
                            eps, sigmoid, ignore_index, ws, ws_bytes, stream);
}

extern "C" int mednet_dice_bwd_lt(const float* logits, const void* labels, int label_dtype, int64_t label_stride_n, const float* weight,
                                  const float* saved, const float* dloss, float* dlogits, int n, int c, size_t spatial,
                                  int64_t stride_n, int64_t stride_c, float eps, int sigmoid, int ignore_index, mednet_stream stream) {
  MEDNET_REQUIRE(c >= 1 && c <= 32, MEDNET_E_UNSUPPORTED, "dice_bwd: C=%d (supported: 1..32)", c);
  MEDNET_REQUIRE(label_dtype == MEDNET_I64 || label_dtype == MEDNET_U8, MEDNET_E_DTYPE, "dice_bwd: labels are int64 or uint8 (got %d)", label_dtype);
  return class_loss_bwd("dice_bwd", MEDNET_CLASS_DICE, logits, labels, label_dtype, label_stride_n, weight, saved, dloss, dlogits, n, c,
                        spatial, stride_n, stride_c, eps, sigmoid, ignore_index, stream);
}
extern "C" int mednet_dice_bwd(const float* logits, const int64_t* labels, const float* weight, const float* saved,
                               const float* dloss, float* dlogits, int n, int c, size_t spatial, int64_t stride_n,
                               int64_t stride_c, float eps, int sigmoid, int ignore_index, mednet_stream stream) {
  return mednet_dice_bwd_lt(logits, labels, MEDNET_I64, (int64_t)spatial, weight, saved, dloss, dlogits, n, c, spatial, stride_n, stride_c,
                            eps, sigmoid, ignore_index, stream);
}

extern "C" int mednet_ce_fwd(const float* logits, const int64_t* labels, const float* weight, float* loss, float* saved,
                             int n, int c, size_t spatial, int64_t stride_n, int64_t stride_c, int ignore_index,
                             void* ws, size_t ws_bytes, mednet_stream stream) {
  MEDNET_REQUIRE(c >= 1 && c <= 32, MEDNET_E_UNSUPPORTED, "ce_fwd: C=%d (supported: 1..32)", c);
  MEDNET_REQUIRE(ws_bytes >= mednet_loss_ws_bytes(n, c, spatial), MEDNET_E_WORKSPACE, "ce_fwd: workspace too small");
  return class_loss_fwd("ce_fwd", MEDNET_CLASS_CE, logits, labels, MEDNET_I64, (int64_t)spatial, weight, loss, saved, nullptr, n, c, spatial,
                        stride_n, stride_c, 0.f, 0, ignore_index, ws, stream);
}

extern "C" int mednet_ce_bwd(const float* logits, const int64_t* labels, const float* weight, const float* saved,
                             const float* dloss, float* dlogits, int n, int c, size_t spatial, int64_t stride_n,
                             int64_t stride_c, int ignore_index, mednet_stream stream) {
  MEDNET_REQUIRE(c >= 1 && c <= 32, MEDNET_E_UNSUPPORTED, "ce_bwd: C=%d (supported: 1..32)", c);
  return class_loss_bwd("ce_bwd", MEDNET_CLASS_CE, logits, labels, MEDNET_I64, (int64_t)spatial, weight, saved, dloss, dlogits, n, c, spatial,
                        stride_n, stride_c, 0.f, 0, ignore_index, stream);
}

// ---- Dice + CE in one pass each way: labels as mednet_dice_*_lt takes them, softmax only, no ignore_index --------------------------
extern "C" size_t mednet_dice_ce_ws_bytes(int n, int c, size_t spatial) {
  return ((size_t)n * loss_blocks(spatial) * ((size_t)c * 2 + 2) + 64) * sizeof(float);
}

extern "C" int mednet_dice_ce_fwd_lt(const float* logits, const void* labels, int label_dtype, int64_t label_stride_n, const float* weight,
                                     float* loss, float* saved, float* dice_out, int n, int c, size_t spatial, int64_t stride_n,
                                     int64_t stride_c, float eps, void* ws, size_t ws_bytes, mednet_stream stream) {
  MEDNET_REQUIRE(logits && labels && loss && saved && ws, MEDNET_E_SHAPE, "dice_ce_fwd: bad arguments");
  MEDNET_REQUIRE(n > 0 && n <= 65535 && spatial > 0, MEDNET_E_SHAPE, "dice_ce_fwd: empty input");
  MEDNET_REQUIRE(c >= 1 && c <= 32, MEDNET_E_UNSUPPORTED, "dice_ce_fwd: C=%d (supported: 1..32)", c);
  MEDNET_REQUIRE(label_dtype == MEDNET_I64 || label_dtype == MEDNET_U8, MEDNET_E_DTYPE, "dice_ce_fwd: labels are int64 or uint8 (got %d)", label_dtype);
  MEDNET_REQUIRE(ws_bytes >= mednet_dice_ce_ws_bytes(n, c, spatial), MEDNET_E_WORKSPACE, "dice_ce_fwd: workspace too small");
  return class_loss_fwd("dice_ce_fwd", MEDNET_CLASS_DICE_CE, logits, labels, label_dtype, label_stride_n, weight, loss, saved, dice_out, n, c,
                        spatial, stride_n, stride_c, eps, 0, MEDNET_NO_IGNORE, ws, stream);
}

extern "C" int mednet_dice_ce_bwd_lt(const float* logits, const void* labels, int label_dtype, int64_t label_stride_n, const float* weight,
                                     const float* saved, const float* dloss, float* dlogits, int n, int c, size_t spatial,
                                     int64_t stride_n, int64_t stride_c, float eps, mednet_stream stream) {
  MEDNET_REQUIRE(logits && labels && saved && dloss && dlogits, MEDNET_E_SHAPE, "dice_ce_bwd: bad arguments");
  MEDNET_REQUIRE(n > 0 && n <= 65535 && spatial > 0, MEDNET_E_SHAPE, "dice_ce_bwd: empty input");
  MEDNET_REQUIRE(c >= 1 && c <= 32, MEDNET_E_UNSUPPORTED, "dice_ce_bwd: C=%d (supported: 1..32)", c);
  MEDNET_REQUIRE(label_dtype == MEDNET_I64 || label_dtype == MEDNET_U8, MEDNET_E_DTYPE, "dice_ce_bwd: labels are int64 or uint8 (got %d)", label_dtype);
  return class_loss_bwd("dice_ce_bwd", MEDNET_CLASS_DICE_CE, logits, labels, label_dtype, label_stride_n, weight, saved, dloss, dlogits, n, c,
                        spatial, stride_n, stride_c, eps, 0, MEDNET_NO_IGNORE, stream);
}

// target_stride_n: element stride between the samples of `target` (channel ch of sample n at + n * target_stride_n + ch * spatial):
// the heat-map channels of a label volume are consumed where they lie, no .contiguous() copy (landmarks.py:68)
extern "C" int mednet_heatmap_loss_fwd_strided(const float* out, const void* target, int64_t target_stride_n, const float* cweight,
                                               float* loss, int n, int c, size_t spatial, int64_t stride_n, int64_t stride_c, int kind,
                                               int tgt_u8, void* ws, size_t ws_bytes, mednet_stream stream) {
  MEDNET_REQUIRE(n > 0 && c > 0 && spatial > 0 && c <= 65535 && n <= 65535, MEDNET_E_SHAPE, "heatmap_loss_fwd: bad shape");
  MEDNET_REQUIRE(ws_bytes >= mednet_loss_ws_bytes(n, c, spatial), MEDNET_E_WORKSPACE, "heatmap_loss_fwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const unsigned nb = loss_blocks(spatial);
  float* partial = (float*)ws;
  if (tgt_u8) hipLaunchKernelGGL(hm_fwd_kernel<uint8_t>, dim3(nb, c, n), dim3(256), 0, s, out, (const uint8_t*)target, target_stride_n, partial, c, spatial, stride_n, stride_c, kind);
  else hipLaunchKernelGGL(hm_fwd_kernel<float>, dim3(nb, c, n), dim3(256), 0, s, out, (const float*)target, target_stride_n, partial, c, spatial, stride_n, stride_c, kind);
  int rc = check_launch("heatmap_loss_fwd");
  if (rc) return rc;
  hipLaunchKernelGGL(hm_finalize_kernel, dim3(1), dim3(1024), 0, s, partial, cweight, loss, n, c, (int)nb, (double)n * (double)spatial);
  return check_launch("heatmap_loss_finalize");
}
extern "C" int mednet_heatmap_loss_fwd(const float* out, const void* target, const float* cweight, float* loss, int n,
                                       int c, size_t spatial, int64_t stride_n, int64_t stride_c, int kind, int tgt_u8,
                                       void* ws, size_t ws_bytes, mednet_stream stream) {
  return mednet_heatmap_loss_fwd_strided(out, target, (int64_t)c * (int64_t)spatial, cweight, loss, n, c, spatial, stride_n, stride_c, kind,
                                         tgt_u8, ws, ws_bytes, stream);
}

extern "C" int mednet_heatmap_loss_bwd_strided(const float* out, const void* target, int64_t target_stride_n, const float* cweight,
                                               const float* dloss, float* dout, int n, int c, size_t spatial, int64_t stride_n,
                                               int64_t stride_c, int kind, int tgt_u8, mednet_stream stream) {
  hipStream_t s = (hipStream_t)stream;
  const unsigned nb = loss_blocks(spatial);
  const float inv = (float)(1.0 / ((double)n * (double)spatial));
  if (tgt_u8) hipLaunchKernelGGL(hm_bwd_kernel<uint8_t>, dim3(nb, c, n), dim3(256), 0, s, out, (const uint8_t*)target, target_stride_n, cweight, dloss, dout, c, spatial, stride_n, stride_c, kind, inv);
  else hipLaunchKernelGGL(hm_bwd_kernel<float>, dim3(nb, c, n), dim3(256), 0, s, out, (const float*)target, target_stride_n, cweight, dloss, dout, c, spatial, stride_n, stride_c, kind, inv);
  return check_launch("heatmap_loss_bwd");
}
extern "C" int mednet_heatmap_loss_bwd(const float* out, const void* target, const float* cweight, const float* dloss,
                                       float* dout, int n, int c, size_t spatial, int64_t stride_n, int64_t stride_c,
                                       int kind, int tgt_u8, mednet_stream stream) {
  return mednet_heatmap_loss_bwd_strided(out, target, (int64_t)c * (int64_t)spatial, cweight, dloss, dout, n, c, spatial, stride_n, stride_c,
                                         kind, tgt_u8, stream);
}
