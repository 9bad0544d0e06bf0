// Building blocks of the matrix-core class heads -- head_lm_kernel and head_seg_kernel (head_mfma.hip), ds_head_kernel (ds_head.hip):
// device code only, ONE copy of everything those kernels do alike.  Included once per translation unit after conv.h and elt16.inc,
// outside any namespace (so once per element type).
//   hlm_* / Hlm*   the skeleton of a 32-feature tile: the hi + lo split, the permuted weight operands (row stride and column offset
//                  as arguments: a tile of a wider W is the same operand), row loads, logit MFMAs, dz store + GroupNorm pass, the
//                  wave-private dW tiles, the end-of-kernel sums;
//   hsg_* / HsgLoss  the per-voxel class-loss arithmetic of the wide-class layout (1 .. 16 classes, classes 8h .. 8h+7 in lane half
//                  h): the constants table of a lane half, sigmoid / two-lane softmax, the forward terms of CE and Dice, the logit
//                  gradient's closed forms, the forward's end-of-kernel rows.
// What stays in the kernels is what differs between them: where the rows come from, the tile loop, and the register-pressure
// measures (the asm barriers on the LDS base pointers, `ce_acc` in the idle LDS slot).
namespace mednet {

constexpr int HLM_RUN = 128;       // voxels per wave and trip
constexpr int HLM_MAXH = 16;       // heat maps (one MFMA k-block)
constexpr int HLM_MAXC = 4;        // classes (second k-block, lanes 0..31)
constexpr int HLM_WIDTH = 32 * 33; // per-workgroup partial of (dW [32 k'][32 ci], db [32 k']); k' = heat map c, or 16 + class
constexpr int HLM_SCR = 33;        // floats per thread of the end-of-kernel LDS scratch
// the class loss of an instantiation (= MEDNET_CLASS_*; the launches take it as `int ce`): DiceLoss, nn.CrossEntropyLoss, or their sum
constexpr int HLM_DICE = 0, HLM_CE = 1, HLM_DICE_CE = 2;
constexpr int HSG_MAXC = 16;       // classes of the wide-class layout: 8 per lane half

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

// The operands take 32 columns of W[.][ld] from column col0 on (a 32-feature head: ld = 32, col0 = 0; tile t of a wider one: 32 t).
// logits^T [output row][voxel]: wops[0,1] = hi, [2,3] = lo parts of row `lrow` of W (-1: a zero row), k-steps of 16 channels
__device__ __forceinline__ void hlm_logit_operands(u32x4 (*wops)[64], const float* W, int lrow, int lane, int ld, int col0) {
  const int h = lane >> 5;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    float w[8];
    eltx8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; ++e) w[e] = lrow >= 0 ? W[(size_t)lrow * ld + col0 + 16 * s + 8 * h + e] : 0.f;
    hlm_split(w, hi, lo);
    wops[s][lane] = __builtin_bit_cast(u32x4, hi);
    wops[2 + s][lane] = __builtin_bit_cast(u32x4, lo);
  }
}
// dz^T [channel row][voxel], one k-block: k-slot 8h + e = row `row0 + e` of W for e < cnt (the others zero), this lane's channel
__device__ __forceinline__ void hlm_dz_operand(u32x4& hi_out, u32x4& lo_out, const float* W, int row0, int cnt, int ch, int ld,
                                               int col0) {
  float w[8];
  eltx8 hi, lo;
#pragma unroll
  for (int e = 0; e < 8; ++e) w[e] = e < cnt ? W[(size_t)(row0 + e) * ld + col0 + ch] : 0.f;
  hlm_split(w, hi, lo);
  hi_out = __builtin_bit_cast(u32x4, hi);
  lo_out = __builtin_bit_cast(u32x4, lo);
}
__device__ __forceinline__ eltx8 hlm_wop(const u32x4* wbase, int i) { return __builtin_bit_cast(eltx8, wbase[i * 64]); }

// loss.hip class_loss_bwd_kernel<DICE>'s per-class terms: gI (the factor of the one-hot target) and gD
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

// dz^T = W^T dl^T of one k-block, W and dl split hi + lo: the three MFMAs hi hi, lo hi, hi lo
__device__ __forceinline__ f32x16 hlm_dz(const eltx8& wop_hi, const eltx8& wop_lo, const eltx8& dc_hi, const eltx8& dc_lo) {
  f32x16 dzv;
#pragma unroll
  for (int i = 0; i < 16; ++i) dzv[i] = 0.f;
  dzv = MEDNET_MFMA_32x32x16(wop_hi, dc_hi, dzv, 0, 0, 0);
  dzv = MEDNET_MFMA_32x32x16(wop_lo, dc_hi, dzv, 0, 0, 0);
  dzv = MEDNET_MFMA_32x32x16(wop_hi, dc_lo, dzv, 0, 0, 0);
  return dzv;
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

// ---- the wide-class layout: 1 .. 16 classes, fused with DiceLoss (loss.py:114-130), nn.CrossEntropyLoss (segmentation.py:49) or
// their sum ---------------------------------------------------------------------------------------------------------------------
// Lane (g, h) holds, of its voxels 4g .. 4g+3, the logits of classes 8h .. 8h+7 in acc[0..7] (weight rows of classes >= ncls are
// zero), so a voxel's classes live in the two lanes l and l ^ 32; `nv` = min(8, max(0, ncls - 8h)) of them are real.  The softmax
// exchanges the half maximum and the half sum of those two lanes with v_permlane32_swap (common.h: plain VALU, no LDS queue); the
// Dice backward exchanges sum_k p_k g_k, the CE backward the label's weight, the same way.  Every exchange runs with all 64 lanes
// active, on predicated values (a dead lane's logits are the biases: finite).
__device__ __forceinline__ float xor32_max(float v) {  // max(v(l), v(l ^ 32)) in every lane: xor32_sum's idiom
  float a = v, b = v;
  MEDNET_SWAP_PAIR("v_permlane32_swap_b32", a, b);
  return fmaxf(a, b);
}

// the class-loss operands of a launch (filled from HlmArgs / DsArgs)
struct HsgLoss {
  const float* bias;        // [ncls], nullable
  const float* cls_weight;  // [ncls], nullable
  const float* saved;       // backward: [ncls][2] = {I, D} of the Dice forward (CE: sum w_y; Dice + CE: [ncls][2], then sum w_y)
  const float* dloss;       // backward: upstream gradient of the loss (scalar)
  float eps;
  int ncls, sigmoid, ignore;
};

// Constants of a lane half, cst[hh][i]: the biases of its 8 classes [0..7]; CE forward: the class weights [8..15]; CE backward:
// w_k dloss / sum w [8..15]; Dice backward: gI [8..15], gD [16..23] (class_loss_bwd_kernel<DICE>); Dice + CE: the forward as CE, the backward as
// Dice and w_k dloss / sum w [24..31].  Called by one whole wave.
template <bool BWD, int KIND>
constexpr int HSG_NCST = (BWD && KIND == HLM_DICE_CE) ? 32 : 24;
template <bool BWD, int KIND, int NCST>
__device__ __forceinline__ void hsg_constants(float (&cst)[2][NCST], int lane, const HsgLoss& c) {
  constexpr bool CE = KIND == HLM_CE;
  static_assert(NCST == HSG_NCST<BWD, KIND>, "the table of this instantiation");
  if ((lane & 31) < NCST) {
    const int hh = lane >> 5, i = lane & 31, k = 8 * hh + (i & 7);
    float v = 0.f;
    if (k < c.ncls) {
      const float w = c.cls_weight ? c.cls_weight[k] : 1.f;
      if (i < 8) v = c.bias ? c.bias[k] : 0.f;
      else if (KIND == HLM_DICE_CE && !BWD) v = i < 16 ? w : 0.f;
      else if (KIND == HLM_DICE_CE && i >= 24) v = w * (*c.dloss / c.saved[2 * c.ncls]);
      else if (CE) v = i < 16 ? (BWD ? w * (*c.dloss / c.saved[0]) : w) : 0.f;
      else if (BWD) {
        const float I = c.saved[2 * k], D = c.saved[2 * k + 1];
        v = i < 16 ? hlm_dice_gI(w, I, D, c.eps, c.ncls, *c.dloss) : hlm_dice_gD(w, I, D, c.eps, c.ncls, *c.dloss);
      }
    }
    cst[hh][i] = v;
  }
}

// sigmoid / softmax of a voxel's class logits (loss.hip cl_probs on registers), the softmax over both lane halves; `lse` (CE terms):
// max + log of the softmax's denominator
template <int KIND>
__device__ __forceinline__ void hsg_probs(const float (&lc)[8], int nv, int sigmoid, float (&p)[8], float& lse) {
  lse = 0.f;
  if (sigmoid) {
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
}

// Forward terms of a voxel with label yl (slot yk = yl - 8h of this half, if in 0 .. nv-1): class_loss_fwd_kernel<CE>'s {sum w_y nll, sum w_y} into
// ce_acc[0..1] (an out-of-range label that is not ignore_index poisons the loss), class_loss_fwd_kernel<DICE>'s {I, D} into dI / dD (`bad`: an
// out-of-range label, NaN at the end of the kernel)
template <int KIND>
__device__ __forceinline__ void hsg_fwd_terms(const HsgLoss& c, const float (&p)[8], const float (&lc)[8], float lse, int yl, int yk,
                                              int nv, bool live, int h, const float* cbase, float* ce_acc, float (&dI)[8],
                                              float (&dD)[8], bool& bad) {
  if constexpr (KIND != HLM_DICE) {
    // class_loss_fwd_kernel<CE>; the half that owns the label's class takes the voxel's term
    if (live && h == 0 && yl != c.ignore && yl >= c.ncls) ce_acc[0] = __builtin_nanf("");
    if (live && yl != c.ignore && yk >= 0 && yk < nv) {
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
  if constexpr (KIND != HLM_CE) {
    bad |= live && yl >= c.ncls;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (e < nv) {
        const float t = (e == yk) ? 1.f : 0.f;
        const float mk = (!live || (c.ignore != MEDNET_NO_IGNORE && t == (float)c.ignore)) ? 0.f : 1.f;
        dI[e] = fmaf(p[e] * mk, t * mk, dI[e]);
        dD[e] += (p[e] + t) * mk;
      }
  }
}

// Logit gradient of a voxel, dc = class_loss_bwd_kernel<CE>'s / class_loss_bwd_kernel<DICE>'s closed form or their sum: added into dbc (db by lane sums) and
// split hi + lo for the MFMAs
template <int KIND>
__device__ __forceinline__ void hsg_logit_grad(const HsgLoss& c, const float (&p)[8], int yl, int yk, int nv, bool live,
                                               const float* cbase, float (&dbc)[8], eltx8& dc_hi, eltx8& dc_lo) {
  float dc[8];
  if constexpr (KIND == HLM_CE) {
    float wy = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (e == yk) wy = cbase[8 + e];  // (0 for classes >= ncls)
    wy = xor32_sum(wy);                // (the other half's lane has 0)
    wy = (live && yl != c.ignore && yl < c.ncls) ? wy : 0.f;
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
    wy = (live && yl < c.ncls) ? wy : 0.f;
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
      const float mk = (c.ignore != MEDNET_NO_IGNORE && t == (float)c.ignore) ? 0.f : 1.f;
      gg[e] = e < nv ? mk * (cbase[8 + e] * t * mk + cbase[16 + e]) : 0.f;
      dot = fmaf(p[e], gg[e], dot);
    }
    if (!c.sigmoid) dot = xor32_sum(dot);  // (uniform)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float v = c.sigmoid ? gg[e] * p[e] * (1.f - p[e]) : p[e] * (gg[e] - dot);
      dc[e] = (live && e < nv) ? v : 0.f;
      dbc[e] += dc[e];
    }
  }
  hlm_split(dc, dc_hi, dc_lo);
}

// End of the forward, after the workgroup's barrier: row `wg` of ce_partial [.][2] from every thread's ce_acc (values 16 / 17 of its
// scratch slot), row `wg` of dice_partial [.][ncls][2] from the lane sums of dI / dD
template <int KIND>
__device__ __forceinline__ void hsg_fwd_writeout(float* scr, int tid, float (&dI)[8], float (&dD)[8], bool bad, float* ce_partial,
                                                 float* dice_partial, size_t wg, int ncls) {
  float* mine = scr + tid * HLM_SCR;
  if constexpr (KIND != HLM_DICE) {  // values 16 / 17 of every thread are its ce_acc
    if (tid < 2) {
      float s = 0.f;
      for (int t = 0; t < 256; ++t) s += scr[t * HLM_SCR + 16 + tid];
      ce_partial[wg * 2 + tid] = s;
    }
  }
  if constexpr (KIND != HLM_CE) {
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
      if (k < ncls) dice_partial[(wg * ncls + k) * 2 + which] = s;
    }
  }
}

}  // namespace mednet
