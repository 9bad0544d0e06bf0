// The per-voxel arithmetic of the class losses -- DiceLoss, nn.CrossEntropyLoss and their sum (KIND = MEDNET_CLASS_*) -- in the layout
// "one voxel per lane, one register per class": device code only, ONE copy for class_loss_*_kernel (loss.hip, MAXC = 2 .. 32) and for
// head_dice_*_kernel (head_loss.hip, MAXC = HL_MAXC).  Included after common.h.  The blocks work on register arrays; where the logits
// come from stays with the kernel.  The build contracts within a statement only (-ffp-contract=on): every statement boundary, operand
// order and fmaf below is part of the result, bit for bit, and the tests that compare the fused heads with the stand-alone losses hold
// because both run these lines.
#pragma once

namespace mednet {

// A label as an int.  An int64 label that does not fit an int (2^32 + 1) must not narrow to a class: it becomes a negative value
// that is not ignore_index, so the range tests below see it as out of range.  Every label that fits is returned as it is, so it
// can be compared with ignore_index; "in range" is (unsigned)y < (unsigned)c everywhere.
template <typename TL>
__device__ __forceinline__ int label_at(const TL* __restrict__ lab, size_t i, int ignore) {
  const int64_t y = (int64_t)lab[i];
  if (y == (int64_t)(int)y) return (int)y;
  return ignore == -1 ? -2 : -1;
}

// The class count is wave-uniform, so `if (k < c)` is a scalar branch that skips a class.  Before a block is inlined into its kernel the
// optimiser folds such a small conditional into selects (every class computed, old and new value live), which cost the stand-alone
// kernels of 8 and 16 classes up to 11 VGPRs and with them a wave per SIMD.  An empty volatile asm in the body keeps the branch; it
// emits nothing.  Up to four classes (the fused heads among them) the selects cost no wave and the blocks are left to the optimiser.
template <int MAXC>
__device__ __forceinline__ void cl_keep_branch() {
  if constexpr (MAXC > 4) asm volatile("");
}

// ---- softmax in pieces (the Dice + CE forward needs mx and den themselves), and whole.  logit(k) hands out the voxel's class-k logit:
// a register, or a load of the stand-alone kernels ------------------------------------------------------------------------------------
template <int MAXC, class Z>
__device__ __forceinline__ float cl_load_max(float* p, Z&& logit, int c, int y, float& zy) {  // p[k] = logit(k); their maximum; zy = p[y]
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < MAXC; ++k)
    if (k < c) {
      cl_keep_branch<MAXC>();
      p[k] = logit(k);
      mx = fmaxf(mx, p[k]);
      if (k == y) zy = p[k];
    }
  return mx;
}
template <int MAXC>
__device__ __forceinline__ float cl_exp_sum(float* p, int c, float mx) {  // p[k] = exp(p[k] - mx); their sum in class order
  float den = 0.f;
#pragma unroll
  for (int k = 0; k < MAXC; ++k)
    if (k < c) {
      cl_keep_branch<MAXC>();
      p[k] = expf(p[k] - mx);
      den += p[k];
    }
  return den;
}
// softmax / sigmoid of the class logits of one voxel
template <int MAXC, class Z>
__device__ __forceinline__ void cl_probs(float* p, Z&& logit, int c, int sigmoid) {
  if (sigmoid) {
#pragma unroll
    for (int k = 0; k < MAXC; ++k)
      if (k < c) p[k] = 1.f / (1.f + expf(-logit(k)));
  } else {
    [[maybe_unused]] float zy;
    const float mx = cl_load_max<MAXC>(p, logit, c, -1, zy);
    const float den = cl_exp_sum<MAXC>(p, c, mx);
    const float inv = 1.f / den;
#pragma unroll
    for (int k = 0; k < MAXC; ++k)
      if (k < c) p[k] *= inv;
  }
}

// ---- forward: the sums of one thread ------------------------------------------------------------------------------------------------
// Dice: I[k] = sum p t mask, D[k] = sum (p + t) mask;  CE: num = sum w_y nll, den = sum w_y;  Dice + CE: all four
template <int MAXC>
struct ClassSums {
  float I[MAXC], D[MAXC];
  float num = 0.f, den = 0.f;
  bool bad = false;  // a label outside [0, C) was seen (Dice forms)
  __device__ __forceinline__ ClassSums() {
#pragma unroll
    for (int k = 0; k < MAXC; ++k) I[k] = D[k] = 0.f;
  }
};

// Dice accumulation with the ignore mask, and without it (a factor of 1.f there: the same sums bit for bit)
template <int MAXC>
__device__ __forceinline__ void cl_dice_terms_masked(ClassSums<MAXC>& a, const float* p, int y, int c, int ignore) {
#pragma unroll
  for (int k = 0; k < MAXC; ++k)
    if (k < c) {
      cl_keep_branch<MAXC>();
      const float t = (k == y) ? 1.f : 0.f;
      // loss.py:31-36: the mask is computed on the ONE-HOT target (values 0/1), not on the label image
      const float m = (ignore != MEDNET_NO_IGNORE && t == (float)ignore) ? 0.f : 1.f;
      a.I[k] = fmaf(p[k] * m, t * m, a.I[k]);
      a.D[k] += (p[k] + t) * m;
    }
}
// (p holds the softmax numerators on entry: scaled by inv = 1 / den where they are used)
template <int MAXC>
__device__ __forceinline__ void cl_dice_terms(ClassSums<MAXC>& a, float* p, float inv, int y, int c) {
#pragma unroll
  for (int k = 0; k < MAXC; ++k)
    if (k < c) {
      cl_keep_branch<MAXC>();
      p[k] *= inv;
      const float t = (k == y) ? 1.f : 0.f;
      a.I[k] = fmaf(p[k], t, a.I[k]);
      a.D[k] += p[k] + t;
    }
}
// the CE term of a voxel whose label y is in range: mx, s = the maximum and the sum of exp(z - mx) of its logits, zy = z[y]
template <int MAXC>
__device__ __forceinline__ void cl_ce_term(ClassSums<MAXC>& a, const float* __restrict__ weight, int y, float mx, float s, float zy) {
  const float w = weight ? weight[y] : 1.f;
  a.num = fmaf(w, (mx + logf(s)) - zy, a.num);
  a.den += w;
}

// One voxel of the forward pass.  logit(k) hands out the voxel's class-k logit: a register of the fused head, a load of the
// stand-alone kernel (cl_load_max).  The CE form asks for every logit twice and keeps no p[]: the stand-alone kernel re-reads the planes for the
// exponentials (32 registers and a wave per SIMD less than holding them at MAXC = 32), and an ignored voxel skips the softmax.
template <int KIND, int MAXC, class Z>
__device__ __forceinline__ void class_fwd_voxel(ClassSums<MAXC>& a, Z&& logit, int y, int c, int sigmoid, int ignore,
                                                const float* __restrict__ weight) {
  const bool ok = (unsigned)y < (unsigned)c;
  if constexpr (KIND == MEDNET_CLASS_CE) {
    // nll_loss raises for a class index outside [0, C) that is not ignore_index; here the loss becomes NaN (see below)
    if (y != ignore && !ok) a.num = __builtin_nanf("");
    if (y != ignore && ok) {
      float mx = -INFINITY, zy = 0.f;
#pragma unroll
      for (int k = 0; k < MAXC; ++k)
        if (k < c) {
          cl_keep_branch<MAXC>();
          const float z = logit(k);
          mx = fmaxf(mx, z);
          if (k == y) zy = z;
        }
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < MAXC; ++k)
        if (k < c) s += expf(logit(k) - mx);
      cl_ce_term<MAXC>(a, weight, y, mx, s, zy);
    }
  } else {
    float p[MAXC];
    // A label outside [0, C) makes the reference raise (scatter_ index error, loss.py:81-86).  Raising from a kernel
    // would cost a host sync per step; instead the loss (and with it every gradient) becomes NaN: loud, not silent.
    a.bad |= !ok;
    if constexpr (KIND == MEDNET_CLASS_DICE_CE) {
      // The softmax of a voxel is computed once: its numerators are the CE form's expf(z - mx) terms and its `den` is that form's `s`
      // (same terms, same order), and the Dice sums are the masked ones with a factor of 1.f: both terms are the single losses' bit for bit.
      float zy = 0.f;
      const float mx = cl_load_max<MAXC>(p, logit, c, y, zy);
      const float den = cl_exp_sum<MAXC>(p, c, mx);
      const float inv = 1.f / den;
      cl_dice_terms<MAXC>(a, p, inv, y, c);
      if (ok) cl_ce_term<MAXC>(a, weight, y, mx, den, zy);
    } else {
      cl_probs<MAXC>(p, logit, c, sigmoid);
      cl_dice_terms_masked<MAXC>(a, p, y, c, ignore);
    }
  }
}

// The workgroup's partial rows, row = blockIdx.y * gridDim.x + blockIdx.x: Dice rows partial[row][c][2] = {I, D}, CE rows [row][2] =
// {num, den}; Dice + CE: the CE rows behind ALL the Dice rows of the grid.  An out-of-range label poisons every term of its kind.
template <int KIND, int MAXC>
__device__ __forceinline__ void class_fwd_writeout(ClassSums<MAXC>& a, float* __restrict__ partial, int c, float* scratch) {
  const size_t row = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  if constexpr (KIND != MEDNET_CLASS_CE) {
    if (a.bad) a.I[0] = a.D[0] = a.num = __builtin_nanf("");
    float* out = partial + row * c * 2;
#pragma unroll
    for (int k = 0; k < MAXC; ++k)
      if (k < c) {
        const float s0 = block_sum<4>(a.I[k], scratch);
        const float s1 = block_sum<4>(a.D[k], scratch);
        if (threadIdx.x == 0) {
          out[2 * k] = s0;
          out[2 * k + 1] = s1;
        }
      }
  }
  if constexpr (KIND != MEDNET_CLASS_DICE) {
    const float num = block_sum<4>(a.num, scratch);
    const float den = block_sum<4>(a.den, scratch);
    if (threadIdx.x == 0) {
      float* o = partial + (KIND == MEDNET_CLASS_DICE_CE ? (size_t)gridDim.y * gridDim.x * c * 2 : 0) + row * 2;
      o[0] = num;
      o[1] = den;
    }
  }
}

// ---- backward: the per-class coefficients of the closed forms ----------------------------------------------------------------------
//   Dice   dL/dp[k] = mask (gI[k] t mask + gD[k]),  gI = -2 w / (C D') dloss,  gD = 2 w I [D >= eps] / (C D'^2) dloss,  D' = max(D, eps)
//   CE     dL/dz[k] = wce[y] (p[k] - t),            wce[k] = w_k dloss / sum w_y
// saved = [c][2] {I, D} (Dice forms), then sum w_y (CE forms)
template <int KIND>
__device__ __forceinline__ void class_coef_of(int k, int c, const float* __restrict__ weight, const float* __restrict__ saved,
                                              float eps, float go, float& gI, float& gD, float& wce) {
  const float w = weight ? weight[k] : 1.f;
  if constexpr (KIND != MEDNET_CLASS_CE) {
    const float I = saved[2 * k], D = saved[2 * k + 1];
    const float Dc = fmaxf(D, eps);  // (fmaxf drops a NaN: the poison of an out-of-range label is re-applied below)
    gI = -2.f * w / ((float)c * Dc) * go + ((I != I || D != D) ? __builtin_nanf("") : 0.f);
    gD = (D >= eps ? 2.f * w * I / ((float)c * Dc * Dc) : 0.f) * go;
  }
  if constexpr (KIND != MEDNET_CLASS_DICE) wce = w * (go / saved[KIND == MEDNET_CLASS_CE ? 0 : 2 * c]);
}
// Where a kernel keeps them: in registers (every thread computes all of them) ...
template <int MAXC>
struct ClassCoefRegs {
  float a[MAXC], b[MAXC], w[MAXC];
  template <int KIND>
  __device__ __forceinline__ void fill(int c, const float* __restrict__ weight, const float* __restrict__ saved, float eps, float go) {
#pragma unroll
    for (int k = 0; k < MAXC; ++k) {
      a[k] = b[k] = w[k] = 0.f;
      if (k < c) class_coef_of<KIND>(k, c, weight, saved, eps, go, a[k], b[k], w[k]);
    }
  }
  __device__ __forceinline__ float gI(int k) const { return a[k]; }
  __device__ __forceinline__ float gD(int k) const { return b[k]; }
  __device__ __forceinline__ float wce(int k) const { return w[k]; }
};
// ... or in an LDS row [gI | gD | wce] of 3 * MAXC floats, read where they are used (thread k < MAXC fills class k; the caller
// makes the barrier).  `off` is 0: a kernel that makes it opaque to the compiler keeps the reads from being hoisted into registers.
template <int MAXC>
struct ClassCoefLds {
  float* row;
  int off = 0;
  template <int KIND>
  __device__ __forceinline__ void fill(int k, int c, const float* __restrict__ weight, const float* __restrict__ saved, float eps, float go) {
    float a = 0.f, b = 0.f, w = 0.f;
    if (k < c) class_coef_of<KIND>(k, c, weight, saved, eps, go, a, b, w);
    row[k] = a;
    row[MAXC + k] = b;
    row[2 * MAXC + k] = w;
  }
  __device__ __forceinline__ float gI(int k) const { return row[off + k]; }
  __device__ __forceinline__ float gD(int k) const { return row[off + MAXC + k]; }
  __device__ __forceinline__ float wce(int k) const { return row[off + 2 * MAXC + k]; }
};

// The logit gradient of one voxel, in place: p holds the logits of the classes < c on entry and their gradient on exit (0 for the
// classes from c on).  softmax: dL/dz[k] = p[k] (g[k] - sum_j p[j] g[j]);  sigmoid: dL/dz[k] = g[k] p[k] (1 - p[k])
template <int KIND, int MAXC, class Coef>
__device__ __forceinline__ void class_logit_grad(float* p, int y, int c, int sigmoid, int ignore, const Coef& coef) {
  cl_probs<MAXC>(p, [&](int k) { return p[k]; }, c, KIND == MEDNET_CLASS_DICE ? sigmoid : 0);
  if constexpr (KIND == MEDNET_CLASS_CE) {
    float w = 0.f;
#pragma unroll
    for (int k = 0; k < MAXC; ++k)
      if (k < c && k == y) w = coef.wce(k);
    w = (y != ignore && (unsigned)y < (unsigned)c) ? w : 0.f;  // (nothing for an ignored or out-of-range label)
#pragma unroll
    for (int k = 0; k < MAXC; ++k) p[k] = k < c ? w * (p[k] - (k == y ? 1.f : 0.f)) : 0.f;
  } else if constexpr (KIND == MEDNET_CLASS_DICE_CE) {
    // One value per logit: the Dice form plus the CE form.  The two terms are formed in statements of their own and added by a plain
    // add: inside one expression -ffp-contract=on would fuse w * (p - t) into the add, and the sum would no longer be the fp32 add of
    // the two losses' gradients that autograd makes of them.
    float g[MAXC];
    float dot = 0.f, w = 0.f;
#pragma unroll
    for (int k = 0; k < MAXC; ++k)
      if (k < c) {
        const float t = (k == y) ? 1.f : 0.f;
        g[k] = coef.gI(k) * t + coef.gD(k);  // (gI * t is exact: fused or not, this is the Dice form's g with mask 1)
        dot = fmaf(p[k], g[k], dot);
        if (k == y) w = coef.wce(k);
      }
#pragma unroll
    for (int k = 0; k < MAXC; ++k) {
      if (k < c) {
        const float dl_dice = p[k] * (g[k] - dot);
        const float dl_ce = w * (p[k] - (k == y ? 1.f : 0.f));
        p[k] = dl_dice + dl_ce;
      } else {
        p[k] = 0.f;
      }
    }
  } else {
    float g[MAXC];
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < MAXC; ++k)
      if (k < c) {
        const float t = (k == y) ? 1.f : 0.f;
        const float m = (ignore != MEDNET_NO_IGNORE && t == (float)ignore) ? 0.f : 1.f;
        g[k] = m * (coef.gI(k) * t * m + coef.gD(k));
        dot = fmaf(p[k], g[k], dot);
      }
#pragma unroll
    for (int k = 0; k < MAXC; ++k) p[k] = k < c ? (sigmoid ? g[k] * p[k] * (1.f - p[k]) : p[k] * (g[k] - dot)) : 0.f;
  }
}

// ---- the 32-feature head: the four lanes that own a voxel's row are one DPP quad, and a quad works on two voxels a and b per trip ----
// Lane q of the quad has loaded the class-q logit of both voxels (oa, ob; 0 for q >= c).  The closed form runs ONCE per voxel: the
// even lanes of the quad evaluate voxel a, the odd lanes voxel b, and the quad hands the results round -- the function and its inputs
// are class_logit_grad's, so da / db are the values every lane used to compute for itself, bit for bit.  Every lane of the quad must be
// active.  (head_dice_bwd_kernel and the GroupNorm-3 apply pass that rebuilds the head's feature gradient, gn_bwd_apply_head_kernel)
template <int KIND, class Coef>
__device__ __forceinline__ void class_logit_grad_quad(float (&da)[4], float (&db)[4], float oa, float ob, int ya, int yb, int c,
                                                      int sigmoid, int ignore, const Coef& coef) {
  const bool second = threadIdx.x & 1;
  // every exchange is made by ALL lanes, in statements of its own, and the choice between the two voxels comes after it: an exchange
  // in one arm of a conditional expression runs with the other arm's lanes switched off and reads nothing from them
  const float a0 = dpp_f32<0x00>(oa), a1 = dpp_f32<0x55>(oa), a2 = dpp_f32<0xAA>(oa), a3 = dpp_f32<0xFF>(oa);
  const float b0 = dpp_f32<0x00>(ob), b1 = dpp_f32<0x55>(ob), b2 = dpp_f32<0xAA>(ob), b3 = dpp_f32<0xFF>(ob);
  float g[4] = {second ? b0 : a0, second ? b1 : a1, second ? b2 : a2, second ? b3 : a3};  // the logits of this lane's voxel
  class_logit_grad<KIND, 4>(g, second ? yb : ya, c, sigmoid, ignore, coef);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    da[k] = dpp_f32<0x00>(g[k]);  // lane 0 of the quad: voxel a
    db[k] = dpp_f32<0x55>(g[k]);  // lane 1: voxel b
  }
}

// The head's feature gradient of one voxel, the 8 channels of one lane: t[j] = sum_i dl[i] * W[i][j] over the classes i < c in class
// order from a zero start, then rounded through the storage type TO -- the value head_dice_bwd_kernel stores, whose GroupNorm sums it
// takes, and which the apply pass of the lazy form rebuilds instead of reading it (one copy: the two must agree bit for bit).
template <typename TO, int MAXC>
__device__ __forceinline__ void head_dz_row(float (&t)[8], const float (&dl)[MAXC], const float (&w)[MAXC][8], int c) {
#pragma unroll
  for (int j = 0; j < 8; ++j) t[j] = 0.f;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    if (i < c) {
#pragma unroll
      for (int j = 0; j < 8; ++j) t[j] = fmaf(dl[i], w[i][j], t[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) t[j] = (float)(TO)t[j];
}

}  // namespace mednet
