// The landmark head on the matrix cores (16-bit storage): the 1x1x1 `final_conv` (model.py:207) of LandmarkNet -- 32 features ->
// nh heat maps + ncls classes (landmarks.py:71-75: 16 + 2) -- fused with BOTH of its losses, the per-channel weighted heat-map
// regression (landmarks.py:125-134) and the Dice loss of the class channels (loss.py:114-130).
//
// Unfused, the 18 planar fp32 logit planes (604 MB at config 4) are written by the head, read by the two loss forwards, read
// again by the two loss backwards, which write their gradient (604 MB), which the head's data gradient, weight gradient and
// bias sums each read again: 2.4 ms of a 21.1 ms step, and with 18 x 32 multiply-adds per voxel and direction the VALU forms
// of the head are compute-bound (head_dgrad_gn_kernel 653 us, wgrad_1x1_kernel 914 us for 1.1 - 1.7 GB each).  Here
//   forward   head_lm_kernel<false>: logits^T = W z^T on v_mfma_f32_32x32x16 (W split hi + lo: fp32-level products), loss terms taken
//             from the accumulator registers; nothing but per-workgroup partial sums is written (the logits only on request).
//   backward  head_lm_kernel<true>: the same MFMAs rebuild the logits bit for bit, the logit gradient is formed in registers
//             (closed forms of loss.hip's hm_bwd_kernel / dice_bwd_kernel) and feeds, split hi + lo,
//               dz^T = W^T dl^T      (stored; the first pass of the producing block's GroupNorm-3 backward is taken from the stored
//                                     rows as head_dgrad_gn_kernel does),
//               dW  += dl^T z        (both operands through the transposing LDS read, contraction over 32 voxels per step),
//               db  += dl            (lane sums).
//             It reads z, the GroupNorm input, the uint8 targets and labels once and writes dz once: 1.75 GB at config 4.
// A wave owns runs of 128 consecutive voxels; lane (g, h) = (lane % 32, lane / 32) holds voxels 4g .. 4g+3 of the run (sub-tile
// j = voxels {4g + j}) and, of each voxel row, the two 16-byte pieces at bytes 16h and 32 + 16h -- channels 8h .. 8h+7 and
// 16+8h .. 16+8h+7 -- for z, the GroupNorm input and dz alike: the row order of the weight operands is permuted (free: they
// are built once per wave from the fp32 weights) so that every MFMA result lands in the lane that owns those bytes.
//
// The file holds two kernels of this shape -- head_lm_kernel (nh heat maps + up to 4 classes in the lanes of half 0) and, further down,
// head_seg_kernel (5 .. 16 classes spread over both lane halves, softmax through v_permlane32_swap) -- and ONE copy of everything they
// do alike: the hlm_* / Hlm* building blocks below HlmArgs (weight operands, row loads, logit MFMAs, dz store + GroupNorm pass, the dW
// tiles, the end-of-kernel sums), head_lm_wfinal_kernel, and on the host one HlmArgs filler behind launch_head_lm_{fwd,bwd} and
// launch_head_seg_{fwd,bwd}, which take the class loss as `int ce`.
#include "conv.h"
#include "elt16.inc"

namespace mednet {

constexpr int HLM_RUN = 128;       // voxels per wave and trip
constexpr int HLM_MAXH = 16;       // heat maps (one MFMA k-block)
constexpr int HLM_MAXC = 4;        // classes (second k-block, lanes 0..31)
constexpr int HLM_WIDTH = 32 * 33; // per-workgroup partial of (dW [32 k'][32 ci], db [32 k']); k' = heat map c, or 16 + class
constexpr int HLM_SCR = 33;        // floats per thread of the end-of-kernel LDS scratch
// the class loss of an instantiation (= MEDNET_CLASS_*; the launches take it as `int ce`): DiceLoss, nn.CrossEntropyLoss, or their sum
constexpr int HLM_DICE = 0, HLM_CE = 1, HLM_DICE_CE = 2;

struct HlmArgs {
  const elt* z;          // [n][spatial][32]: head input (the last block's output)
  const float* W;        // [nh + ncls][32] fp32
  const float* bias;     // [nh + ncls], nullable
  const uint8_t* tgt;    // heat-map targets, planar: sample stride tgt_sn, plane stride spatial
  const uint8_t* lab;    // class labels: sample stride lab_sn
  int64_t tgt_sn, lab_sn;
  size_t spatial;        // % 4 == 0
  int nh, ncls;
  int runs, chunk_runs, chunks;  // runs per sample, runs per workgroup, workgroups per sample
  int kind, sigmoid, ignore;
  // forward
  float* hm_partial;     // [(n * nh + c)][chunks]           (hm_finalize_kernel's layout)
  float* dice_partial;   // [n][chunk][ncls][2]              (dice_finalize_kernel's layout)
  float* logits;         // nullable: [n][nh + ncls][spatial] fp32
  // backward
  const float* saved;    // [ncls][2] = {I, D} of the Dice forward (CE: sum w_y; Dice + CE: [ncls][2], then sum w_y)
  const float* cls_weight;  // [ncls] nullable
  const float* reg_weight;  // [nh] nullable
  const float* dcls;     // upstream gradient of the class loss (scalar)
  const float* dreg;     // ... of the regression loss
  float eps, inv_count;
  elt* dz;               // [n][spatial][32]
  const elt* gn_y;       // nullable: input of the GroupNorm whose activated (+ residual) output z is
  int gn_act;
  float* gn_partial;     // [n][chunks][32][2] = {sum du, sum du * gn_y}, du = dz * act'(z)
  float* wpart;          // [n * chunks][HLM_WIDTH]
  float* ce_partial;     // CE forward: [n][chunk][2] = {sum w_y nll, sum w_y}  (ce_finalize_kernel's layout)
};

// ---- building blocks of head_lm_kernel and head_seg_kernel -------------------------------------------------------------------
// Everything the two kernels do alike, written once; what differs between them is where the classes live (below).
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

__device__ __forceinline__ void hlm_split(const float (&v)[8], eltx8& hi, eltx8& lo) {  // v = hi + lo in the storage type
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    hi[e] = (elt)v[e];
    lo[e] = (elt)(v[e] - (float)hi[e]);
  }
}

// Row i = 8q + 4hh + t of a 32-row weight operand, as lane i (and i + 32) builds it
struct HlmRow {
  int q, hh, t;
  __device__ __forceinline__ explicit HlmRow(int lane) : q((lane & 31) >> 3), hh((lane & 7) >> 2), t(lane & 3) {}
  __device__ __forceinline__ int out() const { return 8 * hh + 4 * q + t; }                          // logits: q 0/1 -> output 8hh + 4q + t
  __device__ __forceinline__ int channel() const { return (q >> 1) * 16 + 8 * hh + (q & 1) * 4 + t; }  // dz: the channel this row stands for
};

// logits^T [output row][voxel]: wops[0,1] = hi, [2,3] = lo parts of row `lrow` of W (-1: a zero row), k-steps of 16 channels
__device__ __forceinline__ void hlm_logit_operands(u32x4 (*wops)[64], const float* W, int lrow, int lane) {
  const int h = lane >> 5;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    float w[8];
    eltx8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; ++e) w[e] = lrow >= 0 ? W[lrow * 32 + 16 * s + 8 * h + e] : 0.f;
    hlm_split(w, hi, lo);
    wops[s][lane] = __builtin_bit_cast(u32x4, hi);
    wops[2 + s][lane] = __builtin_bit_cast(u32x4, lo);
  }
}
// dz^T [channel row][voxel], one k-block: k-slot 8h + e = row `row0 + e` of W for e < cnt (the others zero), this lane's channel
__device__ __forceinline__ void hlm_dz_operand(u32x4& hi_out, u32x4& lo_out, const float* W, int row0, int cnt, int ch) {
  float w[8];
  eltx8 hi, lo;
#pragma unroll
  for (int e = 0; e < 8; ++e) w[e] = e < cnt ? W[(row0 + e) * 32 + ch] : 0.f;
  hlm_split(w, hi, lo);
  hi_out = __builtin_bit_cast(u32x4, hi);
  lo_out = __builtin_bit_cast(u32x4, lo);
}
__device__ __forceinline__ eltx8 hlm_wop(const u32x4* wbase, int i) { return __builtin_bit_cast(eltx8, wbase[i * 64]); }

// loss.hip dice_bwd_kernel's per-class terms: gI (the factor of the one-hot target) and gD
__device__ __forceinline__ float hlm_dice_gI(float w, float I, float D, float eps, int ncls, float gc) {
  return -2.f * w / ((float)ncls * fmaxf(D, eps)) * gc + ((I != I || D != D) ? __builtin_nanf("") : 0.f);
}
__device__ __forceinline__ float hlm_dice_gD(float w, float I, float D, float eps, int ncls, float gc) {
  const float Dc = fmaxf(D, eps);
  return (D >= eps ? 2.f * w * I / ((float)ncls * Dc * Dc) : 0.f) * gc;
}

// The lane's 4 voxel rows (2 pieces of 16 bytes each) of z for a run, and of the GroupNorm input two sub-tiles at a time: sub-tile j
// in yp[j & 1], sub-tile j + 1 fetched at the top of trip j
struct HlmRows {
  u32x4 zp[4][2], yp[2][2];
  __device__ __forceinline__ void load_z(const elt* zs, size_t vb, int h, bool live) {
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int s = 0; s < 2; ++s) zp[j][s] = live ? *reinterpret_cast<const u32x4*>(zs + (vb + j) * 32 + 16 * s + 8 * h) : zero4;
  }
  __device__ __forceinline__ void fetch_y(const elt* ys, size_t vb, int h, bool live, int j) {
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int s = 0; s < 2; ++s)
      yp[j & 1][s] = (live && ys) ? *reinterpret_cast<const u32x4*>(ys + (vb + j) * 32 + 16 * s + 8 * h) : zero4;
  }
};

// logits of the 32 voxels of a sub-tile: 4 MFMAs (2 k-steps x hi / lo)
__device__ __forceinline__ f32x16 hlm_logits(const u32x4* wbase, const u32x4 (&zp)[2]) {
  f32x16 lg;
#pragma unroll
  for (int i = 0; i < 16; ++i) lg[i] = 0.f;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const eltx8 zb = __builtin_bit_cast(eltx8, zp[s]);
    lg = MEDNET_MFMA_32x32x16(hlm_wop(wbase, s), zb, lg, 0, 0, 0);
    lg = MEDNET_MFMA_32x32x16(hlm_wop(wbase, 2 + s), zb, lg, 0, 0, 0);
  }
  return lg;
}

// dz of a voxel row: converted, stored (`dzrow`: the lane's first piece), and the first pass of the GroupNorm backward in front taken
// from the STORED values (head_dgrad_gn_kernel): du = dz * act'(z), ss += du, sq += du * gn_y.  `gn` is workgroup-uniform.
__device__ __forceinline__ void hlm_store_dz(const f32x16& dzv, elt* dzrow, bool live, bool gn, const u32x4 (&zp)[2], const u32x4 (&yp)[2],
                                             int gn_act, float (&ss)[16], float (&sq)[16]) {
  eltx8 o0, o1;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    o0[e] = (elt)dzv[e];
    o1[e] = (elt)dzv[8 + e];
  }
  if (live) {
    *reinterpret_cast<u32x4*>(dzrow) = __builtin_bit_cast(u32x4, o0);
    *reinterpret_cast<u32x4*>(dzrow + 16) = __builtin_bit_cast(u32x4, o1);
  }
  if (gn) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const eltx8 zv = __builtin_bit_cast(eltx8, zp[s]), yv = __builtin_bit_cast(eltx8, yp[s]);
      const eltx8 ov = s ? o1 : o0;
      float du[8], zz[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        du[e] = (float)ov[e];
        zz[e] = (float)zv[e];
      }
      act_grad_n<8>(du, zz, gn_act);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        ss[8 * s + e] += du[e];
        sq[8 * s + e] = fmaf(du[e], (float)yv[e], sq[8 * s + e]);
      }
    }
  }
}

// Wave-private LDS tiles of the backward, 32 voxel rows x 64 B each: z, dl (hi) and dl (lo).  dW += dl^T z over a sub-tile goes through
// them: every lane writes its voxel row, the operands are read back transposed (contraction over the 32 voxels).
struct HlmTiles {
  char *zt, *dlh, *dll;
  int troff;  // tr_operand: voxel rows 8h + tq (+ 4), 4 columns
  __device__ __forceinline__ HlmTiles(char* smem, int wv, int lane) : zt(smem + wv * 6144), dlh(zt + 2048), dll(zt + 4096) {
    const int tq = (lane & 15) >> 2, tp = lane & 3, tg = lane >> 4, h = lane >> 5;
    troff = (8 * h + tq) * 64 + (16 * (tg & 1) + 4 * tp) * 2;
  }
  // the dl columns that no step writes are zeroed once (rows of dW that nobody reads, but no NaNs)
  __device__ __forceinline__ void zero_dl(int lane) const {
    const u32x4 zero = {0u, 0u, 0u, 0u};
    *reinterpret_cast<u32x4*>(dlh + lane * 32) = zero;
    *reinterpret_cast<u32x4*>(dlh + lane * 32 + 16) = zero;
    *reinterpret_cast<u32x4*>(dll + lane * 32) = zero;
    *reinterpret_cast<u32x4*>(dll + lane * 32 + 16) = zero;
    wave_lds_fence();
  }
  // d_hi / d_lo: the lane's 8 dl columns 8h .. 8h+7; x_hi / x_lo (nullable, lanes of h = 0): 4 more columns at 16 .. 19
  __device__ __forceinline__ void dw_step(int g, int h, const u32x4 (&zp)[2], const eltx8& d_hi, const eltx8& d_lo, const eltx8* x_hi,
                                          const eltx8* x_lo, f32x16& accw) const {
    wave_lds_fence();  // (the reads of the previous sub-tile are above these writes)
    *reinterpret_cast<u32x4*>(zt + g * 64 + 16 * h) = zp[0];
    *reinterpret_cast<u32x4*>(zt + g * 64 + 32 + 16 * h) = zp[1];
    *reinterpret_cast<u32x4*>(dlh + g * 64 + 16 * h) = __builtin_bit_cast(u32x4, d_hi);
    *reinterpret_cast<u32x4*>(dll + g * 64 + 16 * h) = __builtin_bit_cast(u32x4, d_lo);
    if (x_hi && h == 0) {
      typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
      const u32x4 ch4 = __builtin_bit_cast(u32x4, *x_hi), cl4 = __builtin_bit_cast(u32x4, *x_lo);
      const u32x2 ch2 = {ch4[0], ch4[1]}, cl2 = {cl4[0], cl4[1]};
      *reinterpret_cast<u32x2*>(dlh + g * 64 + 32) = ch2;
      *reinterpret_cast<u32x2*>(dll + g * 64 + 32) = cl2;
    }
    wave_lds_fence();  // the rows below were written by OTHER lanes of this wave
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const eltx8 fz = tr_operand(zt + ks * 1024 + troff, 256);
      const eltx8 fh = tr_operand(dlh + ks * 1024 + troff, 256);
      const eltx8 fl = tr_operand(dll + ks * 1024 + troff, 256);
      accw = MEDNET_MFMA_32x32x16(fh, fz, accw, 0, 0, 0);
      accw = MEDNET_MFMA_32x32x16(fl, fz, accw, 0, 0, 0);
    }
  }
};

// ---- end of kernel: every thread has put its values at scr[tid * HLM_SCR + .]; sums in a fixed order -----------------------------
// value `idx` summed over the 4 waves x 32 lanes of lane half hh
__device__ __forceinline__ float hlm_lane_sum(const float* scr, int hh, int idx) {
  float s = 0.f;
  for (int w = 0; w < 4; ++w)
    for (int gg = 0; gg < 32; ++gg) s += scr[(w * 64 + hh * 32 + gg) * HLM_SCR + idx];
  return s;
}
// GroupNorm sums: 16 channels x {ss, sq} per lane -> out[32][2] (this workgroup's row of gn_partial)
__device__ __forceinline__ void hlm_gn_writeout(float* scr, int tid, const float (&ss)[16], const float (&sq)[16], float* out) {
  float* mine = scr + tid * HLM_SCR;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    mine[i] = ss[i];
    mine[16 + i] = sq[i];
  }
  __syncthreads();
  if (tid < 64) {
    const int which = tid & 1, idx = (tid >> 1) & 15, hh = tid >> 5;
    const float s = hlm_lane_sum(scr, hh, which * 16 + idx);
    const int ch = (idx >> 3) * 16 + 8 * hh + (idx & 7);
    out[ch * 2 + which] = s;
  }
  __syncthreads();
}
// dW and db of the workgroup -> wp[HLM_WIDTH].  Staged by the caller: the first NV accumulator values of every lane (dW rows k' =
// 8 (i / 4) + 4h + i % 4; NV = 8: rows 0 .. 15 only), behind them 8 db values per lane half (k' = 8h + e) and, for NDB > 16, NDB - 16
// more in the lanes of half 0 (k' = 16 + e)
template <int NV, int NDB>
__device__ __forceinline__ void hlm_dw_db_writeout(const float* scr, int tid, float* wp) {
  __syncthreads();
  for (int o = tid; o < 64 * NV; o += 256) {
    const int L = o & 63, i = o >> 6;
    const float s = (scr[(0 * 64 + L) * HLM_SCR + i] + scr[(1 * 64 + L) * HLM_SCR + i]) +
                    (scr[(2 * 64 + L) * HLM_SCR + i] + scr[(3 * 64 + L) * HLM_SCR + i]);
    const int kp = 8 * (i >> 2) + 4 * (L >> 5) + (i & 3);  // row k' of dW, column (input channel) L % 32
    wp[kp * 32 + (L & 31)] = s;
  }
  if (tid < NDB) {
    const int hh = tid < 16 ? tid >> 3 : 0, idx = tid < 16 ? NV + (tid & 7) : NV + 8 + (tid - 16);
    wp[1024 + tid] = hlm_lane_sum(scr, hh, idx);
  }
}

// (ds_head.hip includes this file for everything above and xor32_max below, with MEDNET_HEAD_BLOCKS_ONLY set: the kernels and the
//  host side of this file are compiled in head_mfma.o alone)
#ifndef MEDNET_HEAD_BLOCKS_ONLY
// CE: the class term is nn.CrossEntropyLoss(weight, ignore_index) (landmarks.py:49) instead of Dice: the forward accumulates
// ce_fwd_kernel's {sum w_y nll, sum w_y} and, for dice_metric (loss.py:51-55), the unweighted, unmasked softmax sums {I, D} into
// dice_partial; the backward's class gradient is ce_bwd_kernel's closed form (dcls / sum w) w_y (p_k - [k == y]).  Softmax only.
// Dice + CE (HLM_DICE_CE, softmax, no ignore_index): the class term is the sum of the two.  Its forward IS the CE forward -- without a
// mask the Dice sums are dice_metric's sums, the class weight enters in the finalize -- so only a backward is instantiated: the
// sum of the two closed forms, with w_k dcls / sum w in the last four constants of the lane half.
template <bool BWD, int KIND = HLM_DICE>
__global__ __launch_bounds__(256, 2) void head_lm_kernel(HlmArgs a) {
  constexpr bool CE = KIND == HLM_CE;
  static_assert(BWD || KIND != HLM_DICE_CE, "the Dice + CE forward is the CE forward");
  __shared__ __attribute__((aligned(16))) char smem[256 * HLM_SCR * 4];
  __shared__ float cst[2][32];
  __shared__ u32x4 wops[8][64];  // the 8 weight operands (below), one 16-byte fragment per lane: the same in every wave
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane & 31, h = lane >> 5;
  const int n = blockIdx.y, chunk = blockIdx.x;
  const int m = a.nh + a.ncls;

  // ---- weight operands, built once: hi + lo parts of the fp32 weights ---------------------------------------------
  // logits^T [k' row i][voxel]: A = W rows in the order that gives lane (g, h) its heat maps 8h .. 8h+7 in acc[0..7] and (h = 0)
  // the classes in acc[8..11]: row i = 8q + 4hh + t -> q 0/1: heat map 8hh + 4q + t; q 2, hh 0: class t
  const HlmRow r(lane);
  const int lrow = r.q < 2 ? (r.out() < a.nh ? r.out() : -1) : ((r.q == 2 && r.hh == 0 && r.t < a.ncls) ? a.nh + r.t : -1);
  if (wv == 0) hlm_logit_operands(wops, a.W, lrow, lane);
  // dz^T [channel row i][voxel]: row i = 8q + 4hh + t stands for channel (q / 2) * 16 + 8hh + (q % 2) * 4 + t, so that lane
  // (g, h) receives channels 8h .. 8h+7 in acc[0..7] and 16+8h .. in acc[8..15]; k-slots 8h + e: block 0 = heat map 8h + e,
  // block 1 = class e (lanes of h = 0)
  if (BWD && wv == 1) {
    hlm_dz_operand(wops[4][lane], wops[6][lane], a.W, 8 * h, a.nh - 8 * h, r.channel());
    hlm_dz_operand(wops[5][lane], wops[7][lane], a.W, a.nh, h == 0 ? a.ncls : 0, r.channel());
  }
  // ---- constants of a lane half, in LDS (they would hold 36 registers for the whole kernel): per h the biases of its 8 heat maps
  // [0..7] and of the classes [8..11], the heat maps' gradient scales [12..19] and the Dice gradient terms gI [20..23], gD [24..27]
  // (CE: the class weights [12..15] in the forward; w_k dcls / sum w [20..23] in the backward)
  if (wv == 2) {
    const int hh = lane >> 5, i = lane & 31;
    float v = 0.f;
    if (i < 8) v = (a.bias && 8 * hh + i < a.nh) ? a.bias[8 * hh + i] : 0.f;
    else if (i < 12) v = (a.bias && i - 8 < a.ncls) ? a.bias[a.nh + i - 8] : 0.f;
    else if (CE && !BWD && i < 16) v = i - 12 < a.ncls ? (a.cls_weight ? a.cls_weight[i - 12] : 1.f) : 0.f;
    else if (BWD && i < 20) {
      const int c = 8 * hh + i - 12;
      v = c < a.nh ? *a.dreg * (a.reg_weight ? a.reg_weight[c] : 1.f) * a.inv_count : 0.f;
    } else if (BWD && i < 28) {  // loss.hip dice_bwd_kernel
      const int k = (i - 20) & 3;
      if (CE && k < a.ncls) {
        v = i < 24 ? (a.cls_weight ? a.cls_weight[k] : 1.f) * (*a.dcls / a.saved[0]) : 0.f;  // (ce_bwd_kernel's `w`)
      } else if (k < a.ncls) {
        const float w = a.cls_weight ? a.cls_weight[k] : 1.f, I = a.saved[2 * k], D = a.saved[2 * k + 1];
        v = i < 24 ? hlm_dice_gI(w, I, D, a.eps, a.ncls, *a.dcls) : hlm_dice_gD(w, I, D, a.eps, a.ncls, *a.dcls);
      }
    } else if (BWD && KIND == HLM_DICE_CE && i - 28 < a.ncls) {  // [28..31]: ce_bwd_kernel's `w` per class
      v = (a.cls_weight ? a.cls_weight[i - 28] : 1.f) * (*a.dcls / a.saved[2 * a.ncls]);
    }
    cst[hh][i] = v;
  }
  __syncthreads();
  // 0,1: logits hi; 2,3: lo; 4,5: dz hi; 6,7: lo.  `wbase` is made opaque once per sub-tile: left alone, the compiler hoists the
  // eight loop-invariant fragments back into 32 registers for the whole kernel
  const u32x4* wbase = &wops[0][lane];
  const float* cbase = &cst[h][0];
  // ---- accumulators ---------------------------------------------------------------------------------------------------
  float hm_acc[8], dI[HLM_MAXC], dD[HLM_MAXC];  // forward
  float ss[16], sq[16], dbh[8], dbc[HLM_MAXC];  // backward
  f32x16 accw;
  bool bad = false;
#pragma unroll
  for (int e = 0; e < 8; ++e) hm_acc[e] = dbh[e] = 0.f;
#pragma unroll
  for (int k = 0; k < HLM_MAXC; ++k) dI[k] = dD[k] = dbc[k] = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) ss[i] = sq[i] = accw[i] = 0.f;

  const HlmTiles tiles(smem, wv, lane);
  // CE forward: {sum w_y nll, sum w_y} of this thread in its own slot of the end-of-kernel scratch (idle until then): as two more
  // loop-carried registers they took the form past its Dice twin's 148 VGPRs
  float* const ce_acc = reinterpret_cast<float*>(smem) + tid * HLM_SCR + 16;
  if constexpr (CE && !BWD) ce_acc[0] = ce_acc[1] = 0.f;
  if constexpr (BWD) tiles.zero_dl(lane);  // (columns 20 .. 31 of the dl tiles are never written)

  const elt* zs = a.z + (size_t)n * a.spatial * 32;
  const elt* ys = (BWD && a.gn_y) ? a.gn_y + (size_t)n * a.spatial * 32 : nullptr;
  elt* dzs = BWD ? a.dz + (size_t)n * a.spatial * 32 : nullptr;
  const uint8_t* tg8 = a.tgt + (size_t)n * a.tgt_sn;
  const uint8_t* lb8 = a.lab + (size_t)n * a.lab_sn;
  const int run_end = min(a.runs, (chunk + 1) * a.chunk_runs);

  // (Measured, profiles/r05_ab.md: requesting zp[j] of the NEXT run as soon as sub-tile j has used it -- a register-neutral software
  //  pipeline -- made both kernels slower, 0.47 -> 0.52 ms and 0.17 -> 0.22 ms at config 4: the loads stay at the top of a run.)
  for (int run = chunk * a.chunk_runs + wv; run < run_end; run += 4) {
    const size_t vb = (size_t)run * HLM_RUN + 4 * g;  // this lane's first voxel
    const bool live = vb < a.spatial;                 // (spatial % 4 == 0: all four voxels or none)
    // ---- loads: the lane's 4 voxel rows (2 pieces each) of z and of the GroupNorm input, 4 target bytes per heat map, 4 labels
    HlmRows rows;
    rows.load_z(zs, vb, h, live);
    if constexpr (BWD) rows.fetch_y(ys, vb, h, live, 0);
    unsigned tb[8];
#pragma unroll
    for (int e = 0; e < 8; ++e)
      tb[e] = (live && 8 * h + e < a.nh) ? *reinterpret_cast<const unsigned*>(tg8 + (size_t)(8 * h + e) * a.spatial + vb) : 0u;
    const unsigned lb = (live && h == 0) ? *reinterpret_cast<const unsigned*>(lb8 + vb) : 0u;

#pragma unroll
    for (int j = 0; j < 4; ++j) {
      asm volatile("" : "+v"(wbase), "+v"(cbase));
      if constexpr (BWD) {
        if (j < 3) rows.fetch_y(ys, vb, h, live, j + 1);
      }
      const f32x16 lg = hlm_logits(wbase, rows.zp[j]);  // the 32 voxels {4g + j}
      float lh[8], lc[HLM_MAXC], p[HLM_MAXC];
#pragma unroll
      for (int e = 0; e < 8; ++e) lh[e] = lg[e] + cbase[e];
#pragma unroll
      for (int k = 0; k < HLM_MAXC; ++k) lc[k] = lg[8 + k] + cbase[8 + k];
      if (!BWD && a.logits && live) {
        float* lo = a.logits + (size_t)n * m * a.spatial + vb + j;
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (8 * h + e < a.nh) lo[(size_t)(8 * h + e) * a.spatial] = lh[e];
        if (h == 0) {
#pragma unroll
          for (int k = 0; k < HLM_MAXC; ++k)
            if (k < a.ncls) lo[(size_t)(a.nh + k) * a.spatial] = lc[k];
        }
      }
      const bool cls_lane = live && h == 0;
      const int yl = (int)((lb >> (8 * j)) & 0xFFu);
      float lse = 0.f;  // (CE: max + log of the softmax's denominator)
      {
        // softmax / sigmoid of the class logits (loss.hip probs_of on registers)
        if (a.sigmoid) {
#pragma unroll
          for (int k = 0; k < HLM_MAXC; ++k) p[k] = k < a.ncls ? 1.f / (1.f + expf(-lc[k])) : 0.f;
        } else {
          float mx = -INFINITY;
#pragma unroll
          for (int k = 0; k < HLM_MAXC; ++k)
            if (k < a.ncls) mx = fmaxf(mx, lc[k]);
          float den = 0.f;
#pragma unroll
          for (int k = 0; k < HLM_MAXC; ++k) {
            p[k] = k < a.ncls ? expf(lc[k] - mx) : 0.f;
            den += p[k];
          }
          const float inv = 1.f / den;
#pragma unroll
          for (int k = 0; k < HLM_MAXC; ++k) p[k] *= inv;
          if (CE) lse = mx + logf(den);
        }
      }
      if constexpr (!BWD) {
        // ---- loss terms: hm_fwd_kernel / dice_fwd_kernel on registers
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float d = lh[e] - (float)((tb[e] >> (8 * j)) & 0xFFu);
          const float t = a.kind == MEDNET_REG_L2 ? d * d : fabsf(d);
          hm_acc[e] += (live && 8 * h + e < a.nh) ? t : 0.f;
        }
        if (CE && cls_lane) {
          // ce_fwd_kernel: w_y ((max + log sum exp) - z_y); an out-of-range label that is not ignore_index poisons the loss
          if (yl != a.ignore && (unsigned)yl >= (unsigned)a.ncls) ce_acc[0] = __builtin_nanf("");
          if (yl != a.ignore && yl < a.ncls) {
            float zy = 0.f, w = 0.f;
#pragma unroll
            for (int k = 0; k < HLM_MAXC; ++k)
              if (k == yl) {
                zy = lc[k];
                w = cbase[12 + k];
              }
            ce_acc[0] = fmaf(w, lse - zy, ce_acc[0]);
            ce_acc[1] += w;
          }
          // dice_metric's sums (dice_fwd_kernel without weight or mask)
          bad |= (unsigned)yl >= (unsigned)a.ncls;
#pragma unroll
          for (int k = 0; k < HLM_MAXC; ++k)
            if (k < a.ncls) {
              const float t = (k == yl) ? 1.f : 0.f;
              dI[k] = fmaf(p[k], t, dI[k]);
              dD[k] += p[k] + t;
            }
        } else if (cls_lane) {
          bad |= (unsigned)yl >= (unsigned)a.ncls;
#pragma unroll
          for (int k = 0; k < HLM_MAXC; ++k)
            if (k < a.ncls) {
              const float t = (k == yl) ? 1.f : 0.f;
              const float mk = (a.ignore != MEDNET_NO_IGNORE && t == (float)a.ignore) ? 0.f : 1.f;
              dI[k] = fmaf(p[k] * mk, t * mk, dI[k]);
              dD[k] += (p[k] + t) * mk;
            }
        }
      } else {
        // ---- logit gradient in registers: hm_bwd_kernel / dice_bwd_kernel
        float dh[8], dc[HLM_MAXC];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float d = lh[e] - (float)((tb[e] >> (8 * j)) & 0xFFu);
          const float sc = live ? cbase[12 + e] : 0.f;  // (0 for heat maps >= nh)
          dh[e] = a.kind == MEDNET_REG_L2 ? 2.f * d * sc : (d > 0.f ? sc : (d < 0.f ? -sc : 0.f));
          dbh[e] += dh[e];
        }
        if constexpr (CE) {
          float wy = 0.f;
#pragma unroll
          for (int k = 0; k < HLM_MAXC; ++k)
            if (k == yl) wy = cbase[20 + k];  // (0 for k >= ncls)
          wy = (yl != a.ignore && yl < a.ncls) ? wy : 0.f;
#pragma unroll
          for (int k = 0; k < HLM_MAXC; ++k) {
            dc[k] = (cls_lane && k < a.ncls) ? wy * (p[k] - (k == yl ? 1.f : 0.f)) : 0.f;
            dbc[k] += dc[k];
          }
        } else if constexpr (KIND == HLM_DICE_CE) {
          float gg[HLM_MAXC], dot = 0.f, wy = 0.f;
#pragma unroll
          for (int k = 0; k < HLM_MAXC; ++k) {
            const float t = (k == yl) ? 1.f : 0.f;
            gg[k] = k < a.ncls ? cbase[20 + k] * t + cbase[24 + k] : 0.f;
            dot = fmaf(p[k], gg[k], dot);
            if (k == yl) wy = cbase[28 + k];  // (0 for k >= ncls)
          }
#pragma unroll
          for (int k = 0; k < HLM_MAXC; ++k) {
            const float dl_dice = p[k] * (gg[k] - dot);
            const float dl_ce = wy * (p[k] - (k == yl ? 1.f : 0.f));
            dc[k] = (cls_lane && k < a.ncls) ? dl_dice + dl_ce : 0.f;
            dbc[k] += dc[k];
          }
        } else {
          float gg[HLM_MAXC], dot = 0.f;
#pragma unroll
          for (int k = 0; k < HLM_MAXC; ++k) {
            const float t = (k == yl) ? 1.f : 0.f;
            const float mk = (a.ignore != MEDNET_NO_IGNORE && t == (float)a.ignore) ? 0.f : 1.f;
            gg[k] = k < a.ncls ? mk * (cbase[20 + k] * t * mk + cbase[24 + k]) : 0.f;
            dot = fmaf(p[k], gg[k], dot);
          }
#pragma unroll
          for (int k = 0; k < HLM_MAXC; ++k) {
            const float v = a.sigmoid ? gg[k] * p[k] * (1.f - p[k]) : p[k] * (gg[k] - dot);
            dc[k] = (cls_lane && k < a.ncls) ? v : 0.f;
            dbc[k] += dc[k];
          }
        }
        float dc8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) dc8[e] = e < HLM_MAXC ? dc[e & (HLM_MAXC - 1)] : 0.f;
        eltx8 dh_hi, dh_lo, dc_hi, dc_lo;
        hlm_split(dh, dh_hi, dh_lo);
        hlm_split(dc8, dc_hi, dc_lo);
        // ---- dz^T = W^T dl^T: 6 MFMAs (two k-blocks x {hi hi, lo hi, hi lo})
        f32x16 dzv;
#pragma unroll
        for (int i = 0; i < 16; ++i) dzv[i] = 0.f;
        dzv = MEDNET_MFMA_32x32x16(hlm_wop(wbase, 4), dh_hi, dzv, 0, 0, 0);
        dzv = MEDNET_MFMA_32x32x16(hlm_wop(wbase, 6), dh_hi, dzv, 0, 0, 0);
        dzv = MEDNET_MFMA_32x32x16(hlm_wop(wbase, 4), dh_lo, dzv, 0, 0, 0);
        dzv = MEDNET_MFMA_32x32x16(hlm_wop(wbase, 5), dc_hi, dzv, 0, 0, 0);
        dzv = MEDNET_MFMA_32x32x16(hlm_wop(wbase, 7), dc_hi, dzv, 0, 0, 0);
        dzv = MEDNET_MFMA_32x32x16(hlm_wop(wbase, 5), dc_lo, dzv, 0, 0, 0);
        hlm_store_dz(dzv, dzs + (vb + j) * 32 + 8 * h, live, ys != nullptr, rows.zp[j], rows.yp[j & 1], a.gn_act, ss, sq);
        tiles.dw_step(g, h, rows.zp[j], dh_hi, dh_lo, &dc_hi, &dc_lo, accw);  // dW += dl^T z over these 32 voxels
      }
    }
  }

  // ---- end of kernel: lane and wave sums through LDS in a fixed order -----------------------------------------------
  float* scr = reinterpret_cast<float*>(smem);
  float* mine = scr + tid * HLM_SCR;
  __syncthreads();
  if constexpr (!BWD) {
    if (bad) dI[0] = dD[0] = __builtin_nanf("");
#pragma unroll
    for (int e = 0; e < 8; ++e) mine[e] = hm_acc[e];
#pragma unroll
    for (int k = 0; k < HLM_MAXC; ++k) {
      mine[8 + k] = dI[k];
      mine[12 + k] = dD[k];
    }
    __syncthreads();  // (CE: values 16 / 17 are the thread's ce_acc)
    if (CE && tid >= 16 + 2 * HLM_MAXC && tid < 18 + 2 * HLM_MAXC) {  // CE sums: lanes of half 0, values 16 / 17
      const int which = tid - (16 + 2 * HLM_MAXC);
      a.ce_partial[((size_t)n * a.chunks + chunk) * 2 + which] = hlm_lane_sum(scr, 0, 16 + which);
    }
    if (tid < 16 + 2 * HLM_MAXC) {
      // heat map c = 8hh + e: lanes of half hh, value e; class sums: lanes of half 0
      const int hh = tid < 16 ? tid >> 3 : 0, idx = tid < 16 ? tid & 7 : tid - 8;
      const float s = hlm_lane_sum(scr, hh, idx);
      if (tid < 16) {
        if (tid < a.nh) a.hm_partial[((size_t)n * a.nh + tid) * a.chunks + chunk] = s;
      } else {
        const int k = (tid - 16) & (HLM_MAXC - 1), which = (tid - 16) / HLM_MAXC;
        if (k < a.ncls) a.dice_partial[(((size_t)n * a.chunks + chunk) * a.ncls + k) * 2 + which] = s;
      }
    }
  } else {
    if (a.gn_partial) hlm_gn_writeout(scr, tid, ss, sq, a.gn_partial + ((size_t)n * a.chunks + chunk) * 64);
    // dW: 16 accumulator values per lane; db behind them: the heat maps', then the classes' (k' = heat map c, or 16 + class)
#pragma unroll
    for (int i = 0; i < 16; ++i) mine[i] = accw[i];
#pragma unroll
    for (int e = 0; e < 8; ++e) mine[16 + e] = dbh[e];
#pragma unroll
    for (int k = 0; k < HLM_MAXC; ++k) mine[24 + k] = dbc[k];
    hlm_dw_db_writeout<16, 16 + HLM_MAXC>(scr, tid, a.wpart + ((size_t)n * a.chunks + chunk) * HLM_WIDTH);
  }
}

// dw[co][ci] = sum over workgroups of wpart[.][k'(co)][ci], db[co] likewise; fixed order (deterministic).  A workgroup = 16 outputs x
// 16 row slices (a thread: every 16th row, 8 loads in flight), then the slices in order.
__global__ __launch_bounds__(256) void head_lm_wfinal_kernel(const float* __restrict__ wpart, int rows, int nh, int ncls,
                                                            float* __restrict__ dw, float* __restrict__ db) {
  __shared__ double sh[16][17];
  const int e = threadIdx.x & 15, q = threadIdx.x >> 4;
  const int m = nh + ncls, total = m * 33;
  const int o = blockIdx.x * 16 + e;
  double acc = 0.0;
  if (o < total) {
    const int co = o < m * 32 ? o / 32 : o - m * 32, kp = co < nh ? co : 16 + (co - nh);
    const int src = o < m * 32 ? kp * 32 + o % 32 : 1024 + kp;
    const float* p = wpart + src;
    int r = q;
    for (; r + 7 * 16 < rows; r += 8 * 16) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(r + 16 * u) * HLM_WIDTH];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += (double)v[u];
    }
    for (; r < rows; r += 16) acc += (double)p[(size_t)r * HLM_WIDTH];
  }
  sh[q][e] = acc;
  __syncthreads();
  if (q == 0 && o < total) {
    double t = 0.0;
#pragma unroll
    for (int u = 0; u < 16; ++u) t += sh[u][e];
    if (o < m * 32) dw[o] = (float)t;
    else if (db) db[o - m * 32] = (float)t;
  }
}
#endif  // MEDNET_HEAD_BLOCKS_ONLY

// ---- the segmentation head: 32 features -> ncls classes, 5 <= ncls <= 16, fused with DiceLoss (loss.py:114-130) or
// nn.CrossEntropyLoss (segmentation.py:49) ---------------------------------------------------------------------------------
// head_lm_kernel's heat-map rows carrying the classes: lane (g, h) holds, of its voxels 4g .. 4g+3, the logits of classes 8h .. 8h+7
// in acc[0..7] (weight rows of classes >= ncls are zero), so a voxel's classes live in the two lanes l and l ^ 32.  The softmax
// exchanges the half maximum and the half sum of those two lanes with v_permlane32_swap (common.h: plain VALU, no LDS queue); the
// Dice backward exchanges sum_k p_k g_k, the CE backward the label's weight, the same way.  Every exchange runs with all 64 lanes
// active, on predicated values (a dead lane's logits are the biases: finite).  HlmArgs with nh = 0: `ncls` classes, no targets.
//   forward   {I, D} per class (dice_finalize_kernel's rows) or {sum w_y nll, sum w_y} (ce_finalize_kernel's rows)
//   backward  logits rebuilt, dl from dice_bwd_kernel's / ce_bwd_kernel's closed form, dz^T = W^T dl^T stored once, dW through the
//             wave-private tiles (dl columns 0 .. 15; 16 .. 31 stay zero), db by lane sums, GroupNorm-3's first pass from the stored rows.
constexpr int HSG_MAXC = 16;

__device__ __forceinline__ float xor32_max(float v) {  // max(v(l), v(l ^ 32)) in every lane: xor32_sum's idiom
  float a = v, b = v;
  MEDNET_SWAP_PAIR("v_permlane32_swap_b32", a, b);
  return fmaxf(a, b);
}
#ifndef MEDNET_HEAD_BLOCKS_ONLY

// Dice + CE (HLM_DICE_CE, softmax, no ignore_index): the forward keeps the Dice accumulators in registers and the CE sums in the idle
// LDS slot; the backward adds the two closed forms, with w_k dloss / sum w in eight more constants of the lane half.
template <bool BWD, int KIND>
__global__ __launch_bounds__(256, 2) void head_seg_kernel(HlmArgs a) {
  constexpr bool CE = KIND == HLM_CE;
  constexpr int NCST = (BWD && KIND == HLM_DICE_CE) ? 32 : 24;
  __shared__ __attribute__((aligned(16))) char smem[256 * HLM_SCR * 4];
  __shared__ float cst[2][NCST];
  __shared__ u32x4 wops[6][64];  // 0,1: logits hi (k-steps); 2,3: lo; 4: dz hi; 5: dz lo
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane & 31, h = lane >> 5;
  const int n = blockIdx.y, chunk = blockIdx.x;
  const int nv = min(8, max(0, a.ncls - 8 * h));  // classes of this lane half

  // ---- weight operands (head_lm_kernel's, the classes in the heat maps' place) ----------------------------------------------
  const HlmRow r(lane);
  if (wv == 0) hlm_logit_operands(wops, a.W, (r.q < 2 && r.out() < a.ncls) ? r.out() : -1, lane);
  if (BWD && wv == 1) hlm_dz_operand(wops[4][lane], wops[5][lane], a.W, 8 * h, a.ncls - 8 * h, r.channel());
  // ---- constants of a lane half: the biases of its 8 classes [0..7]; CE forward: the class weights [8..15]; CE backward:
  // w_k dloss / sum w [8..15]; Dice backward: gI [8..15], gD [16..23] (dice_bwd_kernel); Dice + CE: the forward as CE, the backward as
  // Dice and w_k dloss / sum w [24..31]
  if (wv == 2 && (lane & 31) < NCST) {
    const int hh = lane >> 5, i = lane & 31, k = 8 * hh + (i & 7);
    float v = 0.f;
    if (k < a.ncls) {
      const float w = a.cls_weight ? a.cls_weight[k] : 1.f;
      if (i < 8) v = a.bias ? a.bias[k] : 0.f;
      else if (KIND == HLM_DICE_CE && !BWD) v = i < 16 ? w : 0.f;
      else if (KIND == HLM_DICE_CE && i >= 24) v = w * (*a.dcls / a.saved[2 * a.ncls]);
      else if (CE) v = i < 16 ? (BWD ? w * (*a.dcls / a.saved[0]) : w) : 0.f;
      else if (BWD) {
        const float I = a.saved[2 * k], D = a.saved[2 * k + 1];
        v = i < 16 ? hlm_dice_gI(w, I, D, a.eps, a.ncls, *a.dcls) : hlm_dice_gD(w, I, D, a.eps, a.ncls, *a.dcls);
      }
    }
    cst[hh][i] = v;
  }
  __syncthreads();
  const u32x4* wbase = &wops[0][lane];
  const float* cbase = &cst[h][0];
  // ---- accumulators ---------------------------------------------------------------------------------------------------
  float dI[8], dD[8];                 // forward (Dice)
  float ss[16], sq[16], dbc[8];       // backward
  f32x16 accw;
  bool bad = false;
#pragma unroll
  for (int e = 0; e < 8; ++e) dI[e] = dD[e] = dbc[e] = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) ss[i] = sq[i] = accw[i] = 0.f;

  const HlmTiles tiles(smem, wv, lane);
  float* const ce_acc = reinterpret_cast<float*>(smem) + tid * HLM_SCR + 16;  // (the forward has no tiles: head_lm_kernel)
  if constexpr (KIND != HLM_DICE && !BWD) ce_acc[0] = ce_acc[1] = 0.f;
  if constexpr (BWD) tiles.zero_dl(lane);  // (columns 16 .. 31 of the dl tiles are never written)

  const elt* zs = a.z + (size_t)n * a.spatial * 32;
  const elt* ys = (BWD && a.gn_y) ? a.gn_y + (size_t)n * a.spatial * 32 : nullptr;
  elt* dzs = BWD ? a.dz + (size_t)n * a.spatial * 32 : nullptr;
  const uint8_t* lb8 = a.lab + (size_t)n * a.lab_sn;
  const int run_end = min(a.runs, (chunk + 1) * a.chunk_runs);

  for (int run = chunk * a.chunk_runs + wv; run < run_end; run += 4) {
    const size_t vb = (size_t)run * HLM_RUN + 4 * g;
    const bool live = vb < a.spatial;  // (spatial % 4 == 0: all four voxels or none)
    HlmRows rows;
    rows.load_z(zs, vb, h, live);
    if constexpr (BWD) rows.fetch_y(ys, vb, h, live, 0);
    const unsigned lb = live ? *reinterpret_cast<const unsigned*>(lb8 + vb) : 0u;  // (both halves: each owns 8 of the classes)

#pragma unroll
    for (int j = 0; j < 4; ++j) {
      asm volatile("" : "+v"(wbase), "+v"(cbase));
      if constexpr (BWD) {
        if (j < 3) rows.fetch_y(ys, vb, h, live, j + 1);
      }
      const f32x16 lg = hlm_logits(wbase, rows.zp[j]);
      float lc[8], p[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) lc[e] = lg[e] + cbase[e];
      if (!BWD && a.logits && live) {
        float* lo = a.logits + ((size_t)n * a.ncls + 8 * h) * a.spatial + vb + j;
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (e < nv) lo[(size_t)e * a.spatial] = lc[e];
      }
      const int yl = (int)((lb >> (8 * j)) & 0xFFu);
      const int yk = yl - 8 * h;  // the label's slot in this half, if in 0 .. nv-1
      float lse = 0.f;
      if (a.sigmoid) {
#pragma unroll
        for (int e = 0; e < 8; ++e) p[e] = e < nv ? 1.f / (1.f + expf(-lc[e])) : 0.f;
      } else {
        float mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (e < nv) mx = fmaxf(mx, lc[e]);
        mx = xor32_max(mx);
        float den = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          p[e] = e < nv ? expf(lc[e] - mx) : 0.f;
          den += p[e];
        }
        den = xor32_sum(den);
        const float inv = 1.f / den;
#pragma unroll
        for (int e = 0; e < 8; ++e) p[e] *= inv;
        if (KIND != HLM_DICE) lse = mx + logf(den);
      }
      if constexpr (!BWD) {
        if constexpr (KIND != HLM_DICE) {
          // ce_fwd_kernel; the half that owns the label's class takes the voxel's term
          if (live && h == 0 && yl != a.ignore && yl >= a.ncls) ce_acc[0] = __builtin_nanf("");
          if (live && yl != a.ignore && yk >= 0 && yk < nv) {
            float zy = 0.f, w = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (e == yk) {
                zy = lc[e];
                w = cbase[8 + e];
              }
            ce_acc[0] = fmaf(w, lse - zy, ce_acc[0]);
            ce_acc[1] += w;
          }
        }
        if constexpr (!CE) {
          bad |= live && yl >= a.ncls;
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (e < nv) {
              const float t = (e == yk) ? 1.f : 0.f;
              const float mk = (!live || (a.ignore != MEDNET_NO_IGNORE && t == (float)a.ignore)) ? 0.f : 1.f;
              dI[e] = fmaf(p[e] * mk, t * mk, dI[e]);
              dD[e] += (p[e] + t) * mk;
            }
        }
      } else {
        float dc[8];
        if constexpr (CE) {
          float wy = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (e == yk) wy = cbase[8 + e];  // (0 for classes >= ncls)
          wy = xor32_sum(wy);                // (the other half's lane has 0)
          wy = (live && yl != a.ignore && yl < a.ncls) ? wy : 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            dc[e] = e < nv ? wy * (p[e] - (e == yk ? 1.f : 0.f)) : 0.f;
            dbc[e] += dc[e];
          }
        } else if constexpr (KIND == HLM_DICE_CE) {
          float gg[8], dot = 0.f, wy = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float t = (e == yk) ? 1.f : 0.f;
            gg[e] = e < nv ? cbase[8 + e] * t + cbase[16 + e] : 0.f;
            dot = fmaf(p[e], gg[e], dot);
            if (e == yk) wy = cbase[24 + e];  // (0 for classes >= ncls)
          }
          dot = xor32_sum(dot);
          wy = xor32_sum(wy);  // (the other half's lane has 0)
          wy = (live && yl < a.ncls) ? wy : 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float dl_dice = p[e] * (gg[e] - dot);
            const float dl_ce = wy * (p[e] - (e == yk ? 1.f : 0.f));
            dc[e] = (live && e < nv) ? dl_dice + dl_ce : 0.f;
            dbc[e] += dc[e];
          }
        } else {
          float gg[8], dot = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float t = (e == yk) ? 1.f : 0.f;
            const float mk = (a.ignore != MEDNET_NO_IGNORE && t == (float)a.ignore) ? 0.f : 1.f;
            gg[e] = e < nv ? mk * (cbase[8 + e] * t * mk + cbase[16 + e]) : 0.f;
            dot = fmaf(p[e], gg[e], dot);
          }
          if (!a.sigmoid) dot = xor32_sum(dot);  // (uniform)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float v = a.sigmoid ? gg[e] * p[e] * (1.f - p[e]) : p[e] * (gg[e] - dot);
            dc[e] = (live && e < nv) ? v : 0.f;
            dbc[e] += dc[e];
          }
        }
        eltx8 dc_hi, dc_lo;
        hlm_split(dc, dc_hi, dc_lo);
        // ---- dz^T = W^T dl^T: hi hi, lo hi, hi lo
        f32x16 dzv;
#pragma unroll
        for (int i = 0; i < 16; ++i) dzv[i] = 0.f;
        dzv = MEDNET_MFMA_32x32x16(hlm_wop(wbase, 4), dc_hi, dzv, 0, 0, 0);
        dzv = MEDNET_MFMA_32x32x16(hlm_wop(wbase, 5), dc_hi, dzv, 0, 0, 0);
        dzv = MEDNET_MFMA_32x32x16(hlm_wop(wbase, 4), dc_lo, dzv, 0, 0, 0);
        hlm_store_dz(dzv, dzs + (vb + j) * 32 + 8 * h, live, ys != nullptr, rows.zp[j], rows.yp[j & 1], a.gn_act, ss, sq);
        tiles.dw_step(g, h, rows.zp[j], dc_hi, dc_lo, nullptr, nullptr, accw);  // dW += dl^T z over these 32 voxels
      }
    }
  }

  // ---- end of kernel: lane and wave sums through LDS in a fixed order -----------------------------------------------
  float* scr = reinterpret_cast<float*>(smem);
  float* mine = scr + tid * HLM_SCR;
  __syncthreads();
  if constexpr (!BWD) {
    if constexpr (KIND != HLM_DICE) {  // values 16 / 17 of every thread are its ce_acc
      if (tid < 2) {
        float s = 0.f;
        for (int t = 0; t < 256; ++t) s += scr[t * HLM_SCR + 16 + tid];
        a.ce_partial[((size_t)n * a.chunks + chunk) * 2 + tid] = s;
      }
    }
    if constexpr (!CE) {
      if (bad) dI[0] = dD[0] = __builtin_nanf("");
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        mine[e] = dI[e];
        mine[8 + e] = dD[e];
      }
      __syncthreads();
      if (tid < 2 * HSG_MAXC) {  // class k = 8hh + e: lanes of half hh, value e (I) / 8 + e (D)
        const int k = tid >> 1, which = tid & 1;
        const float s = hlm_lane_sum(scr, k >> 3, 8 * which + (k & 7));
        if (k < a.ncls) a.dice_partial[(((size_t)n * a.chunks + chunk) * a.ncls + k) * 2 + which] = s;
      }
    }
  } else {
    if (a.gn_partial) hlm_gn_writeout(scr, tid, ss, sq, a.gn_partial + ((size_t)n * a.chunks + chunk) * 64);
    // head_lm_kernel's rows: dW row k' = class k' (accumulator values 0 .. 7 of a lane; 8 .. 15 are the zero rows 16 .. 31, which
    // head_lm_wfinal_kernel never reads with ncls = 0), db at 1024 + k'
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      mine[i] = accw[i];
      mine[8 + i] = dbc[i];
    }
    hlm_dw_db_writeout<8, HSG_MAXC>(scr, tid, a.wpart + ((size_t)n * a.chunks + chunk) * HLM_WIDTH);
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------
bool head_lm_supported(int cin, int nh, int ncls, int dtype, size_t spatial) {
  return cin == 32 && nh >= 1 && nh <= HLM_MAXH && ncls >= 1 && ncls <= HLM_MAXC && dtype == ELT_DTYPE && spatial % 4 == 0 &&
         tuning_option("head_lm_mfma", 1);
}
static void head_lm_plan(size_t spatial, int& runs, int& chunk_runs, int& chunks) {
  runs = (int)((spatial + HLM_RUN - 1) / HLM_RUN);
  chunk_runs = 64;  // 16 trips per wave
  chunks = (runs + chunk_runs - 1) / chunk_runs;
}
int head_lm_chunks(size_t spatial) {
  int runs, cr, chunks;
  head_lm_plan(spatial, runs, cr, chunks);
  return chunks;
}
size_t head_lm_ws_bytes(int n, size_t spatial, int nh, int ncls) {
  const size_t chunks = head_lm_chunks(spatial);
  // forward: heat-map rows, Dice rows, CE rows [n][chunk][2] and dice_metric's scratch [ncls][2] (mednet_head_landmark_cls_fwd)
  const size_t fwd = (size_t)n * chunks * (nh + 2 * ncls + 2) + 2 * (size_t)ncls;
  const size_t bwd = (size_t)n * chunks * HLM_WIDTH;
  return ((fwd > bwd ? fwd : bwd) + 64) * sizeof(float);
}

// Everything both directions of both heads share; the segmentation head is nh = 0 without targets.  `tgt` and `lab` are read four
// voxels at a time.
static int hlm_args(HlmArgs& a, const char* what, const void* z, const float* W, const float* bias, const void* tgt, int64_t tgt_sn,
                    const void* lab, int64_t lab_sn, const float* cls_weight, size_t spatial, int nh, int ncls, int kind, int sigmoid,
                    int ignore) {
  a.z = (const elt*)z; a.W = W; a.bias = bias; a.tgt = (const uint8_t*)tgt; a.lab = (const uint8_t*)lab;
  a.tgt_sn = tgt_sn; a.lab_sn = lab_sn; a.spatial = spatial; a.nh = nh; a.ncls = ncls;
  head_lm_plan(spatial, a.runs, a.chunk_runs, a.chunks);
  a.kind = kind; a.sigmoid = sigmoid; a.ignore = ignore; a.cls_weight = cls_weight;
  MEDNET_REQUIRE(tgt_sn % 4 == 0 && lab_sn % 4 == 0 && ((uintptr_t)tgt & 3) == 0 && ((uintptr_t)lab & 3) == 0, MEDNET_E_SHAPE,
                 "%s: %s must be 4-byte aligned per sample", what, tgt ? "targets and labels" : "labels");
  return 0;
}
// ... and what the backward adds; its workspace holds the dW / db partial rows
static int hlm_bwd_args(HlmArgs& a, const char* what, const float* saved, const float* dcls, float eps, void* dz, const void* gn_y,
                        int gn_act, float* gn_partial, void* ws, size_t ws_bytes, size_t ws_need) {
  a.saved = saved; a.dcls = dcls; a.eps = eps;
  a.dz = (elt*)dz; a.gn_y = (const elt*)gn_y; a.gn_act = gn_act; a.gn_partial = gn_partial;
  MEDNET_REQUIRE((gn_y == nullptr) == (gn_partial == nullptr), MEDNET_E_SHAPE, "%s: gn_y and gn_partial go together", what);
  MEDNET_REQUIRE(ws_bytes >= ws_need, MEDNET_E_WORKSPACE, "%s: workspace too small", what);
  a.wpart = (float*)ws;
  return 0;
}

// ce = 2 (HLM_DICE_CE): the forward is the CE form's (the caller finalises both rows); the backward reads saved = [ncls][2], then sum w_y.
// ce = 1: nn.CrossEntropyLoss(cls_weight, ignore) as the class term (softmax; `sigmoid` and `eps` are not read): ce_partial [n][chunk][2]
// for ce_finalize, and dice_partial takes dice_metric's unweighted, unmasked sums; the backward reads saved[0] = sum w_y of that forward.
int launch_head_lm_fwd(const void* z, const float* W, const float* bias, const void* tgt, int64_t tgt_sn, const void* lab,
                       int64_t lab_sn, const float* cls_weight, float* logits, float* hm_partial, float* dice_partial, float* ce_partial,
                       int n, size_t spatial, int nh, int ncls, int kind, int ce, int sigmoid, int ignore, hipStream_t s) {
  HlmArgs a = {};
  const int rc = hlm_args(a, "head_lm", z, W, bias, tgt, tgt_sn, lab, lab_sn, ce ? cls_weight : nullptr, spatial, nh, ncls, kind,
                          ce ? 0 : sigmoid, ignore);
  if (rc) return rc;
  a.hm_partial = hm_partial; a.dice_partial = dice_partial; a.logits = logits; a.ce_partial = ce ? ce_partial : nullptr;
  if (ce) hipLaunchKernelGGL((head_lm_kernel<false, HLM_CE>), dim3(a.chunks, n), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((head_lm_kernel<false, HLM_DICE>), dim3(a.chunks, n), dim3(256), 0, s, a);
  return check_launch(ce ? "head_lm_ce_fwd" : "head_lm_fwd");
}
int launch_head_lm_bwd(const void* z, const float* W, const float* bias, const void* tgt, int64_t tgt_sn, const void* lab,
                       int64_t lab_sn, const float* saved, const float* cls_weight, const float* reg_weight, const float* dcls,
                       const float* dreg, float eps, void* dz, const void* gn_y, int gn_act, float* gn_partial, float* dw, float* db,
                       int n, size_t spatial, int nh, int ncls, int kind, int ce, int sigmoid, int ignore, void* ws, size_t ws_bytes,
                       hipStream_t s) {
  HlmArgs a = {};
  int rc = hlm_args(a, "head_lm", z, W, bias, tgt, tgt_sn, lab, lab_sn, cls_weight, spatial, nh, ncls, kind, ce ? 0 : sigmoid, ignore);
  if (rc) return rc;
  rc = hlm_bwd_args(a, "head_lm_bwd", saved, dcls, ce == HLM_CE ? 0.f : eps, dz, gn_y, gn_act, gn_partial, ws, ws_bytes,
                    head_lm_ws_bytes(n, spatial, nh, ncls));
  if (rc) return rc;
  a.reg_weight = reg_weight; a.dreg = dreg; a.inv_count = (float)(1.0 / ((double)n * (double)spatial));
  if (ce == HLM_DICE_CE) hipLaunchKernelGGL((head_lm_kernel<true, HLM_DICE_CE>), dim3(a.chunks, n), dim3(256), 0, s, a);
  else if (ce) hipLaunchKernelGGL((head_lm_kernel<true, HLM_CE>), dim3(a.chunks, n), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((head_lm_kernel<true, HLM_DICE>), dim3(a.chunks, n), dim3(256), 0, s, a);
  rc = check_launch(ce == HLM_DICE_CE ? "head_lm_dice_ce_bwd" : ce ? "head_lm_ce_bwd" : "head_lm_bwd");
  if (rc) return rc;
  const int total = (nh + ncls) * 33;
  hipLaunchKernelGGL(head_lm_wfinal_kernel, dim3((total + 15) / 16), dim3(256), 0, s, a.wpart, n * a.chunks, nh, ncls, dw, db);
  return check_launch("head_lm_wfinal");
}

// ---- the segmentation head (head_seg_kernel): head_lm's plan, partial rows and final sums -------------------------------------
bool head_seg_supported(int cin, int ncls, int dtype, size_t spatial) {
  return cin == 32 && ncls >= 5 && ncls <= HSG_MAXC && dtype == ELT_DTYPE && spatial % 4 == 0 && tuning_option("head_seg_mfma", 1);
}
size_t head_seg_ws_bytes(int n, size_t spatial, int ncls) {
  const size_t chunks = head_lm_chunks(spatial);
  const size_t fwd = (size_t)n * chunks * (2 * ncls + 2);  // Dice rows [n][chunk][ncls][2] or CE rows [n][chunk][2]
  const size_t bwd = (size_t)n * chunks * HLM_WIDTH;
  return ((fwd > bwd ? fwd : bwd) + 64) * sizeof(float);
}
int launch_head_seg_fwd(const void* z, const float* W, const float* bias, const void* lab, int64_t lab_sn, const float* cls_weight,
                        float* logits, float* partial, int n, size_t spatial, int ncls, int ce, int sigmoid, int ignore, hipStream_t s) {
  HlmArgs a = {};
  const int rc = hlm_args(a, "head_seg_fwd", z, W, bias, nullptr, 0, lab, lab_sn, cls_weight, spatial, 0, ncls, 0, sigmoid, ignore);
  if (rc) return rc;
  a.logits = logits;
  (ce == HLM_CE ? a.ce_partial : a.dice_partial) = partial;
  if (ce == HLM_DICE_CE) {  // the Dice rows, behind all of them the CE rows
    a.ce_partial = partial + (size_t)n * a.chunks * ncls * 2;
    hipLaunchKernelGGL((head_seg_kernel<false, HLM_DICE_CE>), dim3(a.chunks, n), dim3(256), 0, s, a);
    return check_launch("head_seg_dice_ce_fwd");
  }
  if (ce) hipLaunchKernelGGL((head_seg_kernel<false, HLM_CE>), dim3(a.chunks, n), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((head_seg_kernel<false, HLM_DICE>), dim3(a.chunks, n), dim3(256), 0, s, a);
  return check_launch(ce ? "head_seg_ce_fwd" : "head_seg_fwd");
}
int launch_head_seg_bwd(const void* z, const float* W, const float* bias, const void* lab, int64_t lab_sn, const float* saved,
                        const float* cls_weight, const float* dloss, float eps, void* dz, const void* gn_y, int gn_act,
                        float* gn_partial, float* dw, float* db, int n, size_t spatial, int ncls, int ce, int sigmoid, int ignore,
                        void* ws, size_t ws_bytes, hipStream_t s) {
  HlmArgs a = {};
  int rc = hlm_args(a, "head_seg_bwd", z, W, bias, nullptr, 0, lab, lab_sn, cls_weight, spatial, 0, ncls, 0, sigmoid, ignore);
  if (rc) return rc;
  rc = hlm_bwd_args(a, "head_seg_bwd", saved, dloss, eps, dz, gn_y, gn_act, gn_partial, ws, ws_bytes, head_seg_ws_bytes(n, spatial, ncls));
  if (rc) return rc;
  if (ce == HLM_DICE_CE) hipLaunchKernelGGL((head_seg_kernel<true, HLM_DICE_CE>), dim3(a.chunks, n), dim3(256), 0, s, a);
  else if (ce) hipLaunchKernelGGL((head_seg_kernel<true, HLM_CE>), dim3(a.chunks, n), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((head_seg_kernel<true, HLM_DICE>), dim3(a.chunks, n), dim3(256), 0, s, a);
  rc = check_launch(ce == HLM_DICE_CE ? "head_seg_dice_ce_bwd" : ce ? "head_seg_ce_bwd" : "head_seg_bwd");
  if (rc) return rc;
  hipLaunchKernelGGL(head_lm_wfinal_kernel, dim3((ncls * 33 + 15) / 16), dim3(256), 0, s, a.wpart, n * a.chunks, ncls, 0, dw, db);
  return check_launch("head_seg_wfinal");
}
#endif  // MEDNET_HEAD_BLOCKS_ONLY

}  // namespace mednet
