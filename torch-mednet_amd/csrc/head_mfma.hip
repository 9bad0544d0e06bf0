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
//             (closed forms of loss.hip's hm_bwd_kernel / class_loss_bwd_kernel<DICE>) and feeds, split hi + lo,
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
// head_seg_kernel (5 .. 16 classes spread over both lane halves, softmax through v_permlane32_swap).  Everything they do alike, and
// everything head_seg_kernel does alike with ds_head.hip's kernel, is in head_blocks.inc: the hlm_* / Hlm* skeleton (weight operands,
// row loads, logit MFMAs, dz store + GroupNorm pass, the dW tiles, the end-of-kernel sums) and the hsg_* class-loss arithmetic of
// the wide-class layout.  Here: the two kernels, head_lm_wfinal_kernel, and on the host one HlmArgs filler behind
// launch_head_lm_{fwd,bwd} and launch_head_seg_{fwd,bwd}, which take the class loss as `int ce` (for_class_kind, conv.h).
#include "conv.h"
#include "elt16.inc"
#include "head_blocks.inc"

namespace mednet {

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

// CE: the class term is nn.CrossEntropyLoss(weight, ignore_index) (landmarks.py:49) instead of Dice: the forward accumulates
// class_loss_fwd_kernel<CE>'s {sum w_y nll, sum w_y} and, for dice_metric (loss.py:51-55), the unweighted, unmasked softmax sums {I, D} into
// dice_partial; the backward's class gradient is class_loss_bwd_kernel<CE>'s closed form (dcls / sum w) w_y (p_k - [k == y]).  Softmax only.
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
  if (wv == 0) hlm_logit_operands(wops, a.W, lrow, lane, 32, 0);
  // dz^T [channel row i][voxel]: row i = 8q + 4hh + t stands for channel (q / 2) * 16 + 8hh + (q % 2) * 4 + t, so that lane
  // (g, h) receives channels 8h .. 8h+7 in acc[0..7] and 16+8h .. in acc[8..15]; k-slots 8h + e: block 0 = heat map 8h + e,
  // block 1 = class e (lanes of h = 0)
  if (BWD && wv == 1) {
    hlm_dz_operand(wops[4][lane], wops[6][lane], a.W, 8 * h, a.nh - 8 * h, r.channel(), 32, 0);
    hlm_dz_operand(wops[5][lane], wops[7][lane], a.W, a.nh, h == 0 ? a.ncls : 0, r.channel(), 32, 0);
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
    } else if (BWD && i < 28) {  // loss.hip class_loss_bwd_kernel<DICE>
      const int k = (i - 20) & 3;
      if (CE && k < a.ncls) {
        v = i < 24 ? (a.cls_weight ? a.cls_weight[k] : 1.f) * (*a.dcls / a.saved[0]) : 0.f;  // (class_loss_bwd_kernel<CE>'s `w`)
      } else if (k < a.ncls) {
        const float w = a.cls_weight ? a.cls_weight[k] : 1.f, I = a.saved[2 * k], D = a.saved[2 * k + 1];
        v = i < 24 ? hlm_dice_gI(w, I, D, a.eps, a.ncls, *a.dcls) : hlm_dice_gD(w, I, D, a.eps, a.ncls, *a.dcls);
      }
    } else if (BWD && KIND == HLM_DICE_CE && i - 28 < a.ncls) {  // [28..31]: class_loss_bwd_kernel<CE>'s `w` per class
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
        // softmax / sigmoid of the class logits (loss.hip cl_probs on registers)
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
        // ---- loss terms: hm_fwd_kernel / class_loss_fwd_kernel<DICE> on registers
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float d = lh[e] - (float)((tb[e] >> (8 * j)) & 0xFFu);
          const float t = a.kind == MEDNET_REG_L2 ? d * d : fabsf(d);
          hm_acc[e] += (live && 8 * h + e < a.nh) ? t : 0.f;
        }
        if (CE && cls_lane) {
          // class_loss_fwd_kernel<CE>: w_y ((max + log sum exp) - z_y); an out-of-range label that is not ignore_index poisons the loss
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
          // dice_metric's sums (class_loss_fwd_kernel<DICE> without weight or mask)
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
        // ---- logit gradient in registers: hm_bwd_kernel / class_loss_bwd_kernel<DICE>
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

// ---- the segmentation head: 32 features -> ncls classes, 5 <= ncls <= 16, fused with DiceLoss (loss.py:114-130) or
// nn.CrossEntropyLoss (segmentation.py:49) ---------------------------------------------------------------------------------
// head_lm_kernel's heat-map rows carrying the classes in the wide-class layout of head_blocks.inc (classes 8h .. 8h+7 in lane half h;
// the hsg_* blocks are the per-voxel loss arithmetic).  HlmArgs with nh = 0: `ncls` classes, no targets.
//   forward   {I, D} per class (dice_finalize_kernel's rows) or {sum w_y nll, sum w_y} (ce_finalize_kernel's rows)
//   backward  logits rebuilt, dl from class_loss_bwd_kernel<DICE>'s / class_loss_bwd_kernel<CE>'s closed form, dz^T = W^T dl^T stored once, dW through the
//             wave-private tiles (dl columns 0 .. 15; 16 .. 31 stay zero), db by lane sums, GroupNorm-3's first pass from the stored rows.
// Dice + CE (HLM_DICE_CE, softmax, no ignore_index): the forward keeps the Dice accumulators in registers and the CE sums in the idle
// LDS slot; the backward adds the two closed forms, with w_k dloss / sum w in eight more constants of the lane half.
template <bool BWD, int KIND>
__global__ __launch_bounds__(256, 2) void head_seg_kernel(HlmArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[256 * HLM_SCR * 4];
  __shared__ float cst[2][HSG_NCST<BWD, KIND>];
  __shared__ u32x4 wops[6][64];  // 0,1: logits hi (k-steps); 2,3: lo; 4: dz hi; 5: dz lo
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane & 31, h = lane >> 5;
  const int n = blockIdx.y, chunk = blockIdx.x;
  const int nv = min(8, max(0, a.ncls - 8 * h));  // classes of this lane half
  const HsgLoss c = {a.bias, a.cls_weight, a.saved, a.dcls, a.eps, a.ncls, a.sigmoid, a.ignore};

  // ---- weight operands (head_lm_kernel's, the classes in the heat maps' place) and the constants of a lane half ---------------
  const HlmRow r(lane);
  if (wv == 0) hlm_logit_operands(wops, a.W, (r.q < 2 && r.out() < a.ncls) ? r.out() : -1, lane, 32, 0);
  if (BWD && wv == 1) hlm_dz_operand(wops[4][lane], wops[5][lane], a.W, 8 * h, a.ncls - 8 * h, r.channel(), 32, 0);
  if (wv == 2) hsg_constants<BWD, KIND>(cst, lane, c);
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
      float lse;
      hsg_probs<KIND>(lc, nv, a.sigmoid, p, lse);
      if constexpr (!BWD) {
        hsg_fwd_terms<KIND>(c, p, lc, lse, yl, yk, nv, live, h, cbase, ce_acc, dI, dD, bad);
      } else {
        eltx8 dc_hi, dc_lo;
        hsg_logit_grad<KIND>(c, p, yl, yk, nv, live, cbase, dbc, dc_hi, dc_lo);
        const f32x16 dzv = hlm_dz(hlm_wop(wbase, 4), hlm_wop(wbase, 5), dc_hi, dc_lo);
        hlm_store_dz(dzv, dzs + (vb + j) * 32 + 8 * h, live, ys != nullptr, rows.zp[j], rows.yp[j & 1], a.gn_act, ss, sq);
        tiles.dw_step(g, h, rows.zp[j], dc_hi, dc_lo, nullptr, nullptr, accw);  // dW += dl^T z over these 32 voxels
      }
    }
  }

  // ---- end of kernel: lane and wave sums through LDS in a fixed order -----------------------------------------------
  float* scr = reinterpret_cast<float*>(smem);
  __syncthreads();
  if constexpr (!BWD) {
    hsg_fwd_writeout<KIND>(scr, tid, dI, dD, bad, a.ce_partial, a.dice_partial, (size_t)n * a.chunks + chunk, a.ncls);
  } else {
    float* mine = scr + tid * HLM_SCR;
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
  for_class_kind(ce, [&](auto kind) {
    hipLaunchKernelGGL((head_lm_kernel<true, decltype(kind)::value>), dim3(a.chunks, n), dim3(256), 0, s, a);
  });
  rc = check_launch(MEDNET_CLASS_KIND_NAME(ce, "head_lm", "_bwd"));
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
  if (ce == HLM_DICE_CE) a.ce_partial = partial + (size_t)n * a.chunks * ncls * 2;  // the Dice rows, behind all of them the CE rows
  for_class_kind(ce, [&](auto kind) {
    hipLaunchKernelGGL((head_seg_kernel<false, decltype(kind)::value>), dim3(a.chunks, n), dim3(256), 0, s, a);
  });
  return check_launch(MEDNET_CLASS_KIND_NAME(ce, "head_seg", "_fwd"));
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
  for_class_kind(ce, [&](auto kind) {
    hipLaunchKernelGGL((head_seg_kernel<true, decltype(kind)::value>), dim3(a.chunks, n), dim3(256), 0, s, a);
  });
  rc = check_launch(MEDNET_CLASS_KIND_NAME(ce, "head_seg", "_bwd"));
  if (rc) return rc;
  hipLaunchKernelGGL(head_lm_wfinal_kernel, dim3((ncls * 33 + 15) / 16), dim3(256), 0, s, a.wpart, n * a.chunks, ncls, 0, dw, db);
  return check_launch("head_seg_wfinal");
}

}  // namespace mednet
