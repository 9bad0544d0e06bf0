// Deep supervision: the auxiliary 1x1x1 head of a coarser decoder level (cin = 64 .. 256 features -> ncls <= 16 classes) fused with
// its class loss against the FULL-resolution uint8 label volume read at a stride -- voxel (z, y, x) of level s reads
// label[z << s][y << s][x << s], which is F.interpolate(mode="nearest") for the scale 2^-s -- and, in the backward, with the junction
// "block output -> {next decoder, auxiliary head}": the gradient that arrives from the next decoder (d_pass) is added in fp32 to
// W^T dl before the one rounding to the storage type.  No down-sampled label tensor, no logit tensor, no logit-gradient tensor and
// no autograd add of two feature gradients exist.
//
// The kernel is head_seg_kernel (head_mfma.hip) with the 32-feature row made a loop over 32-channel tiles.  Both are built from
// head_blocks.inc: the hi + lo split, the permuted weight operands (here at row stride cin, column offset 32 t), the wave-private dW
// tiles HlmTiles, the end-of-kernel sums, and the hsg_* class-loss arithmetic of the wide-class layout, of which there is one copy.
//   forward   logits^T = W z^T on v_mfma_f32_32x32x16, accumulated over the tiles (4 MFMAs per tile and 32 voxels: 2 k-steps x hi / lo
//             of the fp32 weights); lane (g, h) then holds classes 8h .. 8h+7 of its voxels 4g .. 4g+3 exactly as in head_seg_kernel
//             (hsg_probs, hsg_fwd_terms).  Only loss partial rows are written (dice_finalize_kernel's / ce_finalize_kernel's layouts).
//   backward  the same MFMAs rebuild the logits bit for bit; dl from the closed forms; per tile dz^T = W_t^T dl^T (3 MFMAs), + d_pass,
//             rounded once, stored; dW_t += dl^T z_t through the transposing LDS tiles; db by lane sums.  The tile's z rows are read a
//             second time for dW (the run's 128 rows were read a moment ago by the same wave: they come from the cache).
//             Per-workgroup partial rows [tiles][HLM_WIDTH], summed in a fixed order by ds_head_wfinal_kernel: no float atomics.
// The register budget does not grow with cin except for the dW accumulators (16 per tile): the backward is instantiated for up to 4
// and up to 8 tiles.  The producing block's GroupNorm-3 sums are NOT taken here (mednet_ds_head_gn_rows answers 0): the block runs
// its stand-alone first pass.
#include "conv.h"
#include "elt16.inc"
#include "head_blocks.inc"

namespace mednet {

constexpr int DSH_MAXT = 8;  // 32-channel tiles: cin <= 256

struct DsArgs {
  const elt* z;          // [n][spatial][cin]: the level's block output
  const float* W;        // [ncls][cin] fp32
  const float* bias;     // [ncls], nullable
  const uint8_t* lab;    // the full-resolution label volume, sample stride lab_sn
  int64_t lab_sn;
  int64_t full_w, full_hw;  // W and H * W of the full volume
  unsigned lev_w, lev_hw;   // w and h * w of the level
  int shift;
  size_t spatial;        // d * h * w of the level, % 4 == 0, < 2^31
  int cin, tiles, ncls;
  int runs, chunk_runs, chunks;
  int sigmoid, ignore;
  float* dice_partial;   // [n][chunk][ncls][2]
  float* ce_partial;     // [n][chunk][2]
  const float* saved;
  const float* cls_weight;
  const float* dloss;
  float eps;
  const elt* d_pass;     // nullable: [n][spatial][cin], the gradient from the other consumer of z
  elt* dz;
  float* wpart;          // [n * chunks][tiles][HLM_WIDTH]
};

// the labels of voxels v0 .. v0 + 3 of the level, one byte load each, packed as head_seg_kernel's 4-voxel word
__device__ __forceinline__ unsigned ds_pick4(const DsArgs& a, const uint8_t* lb8, unsigned v0, bool live) {
  unsigned lb = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (live) {
      const unsigned v = v0 + j;
      const unsigned zz = v / a.lev_hw, r = v - zz * a.lev_hw;
      const unsigned y = r / a.lev_w, x = r - y * a.lev_w;
      const int64_t at = ((int64_t)zz << a.shift) * a.full_hw + ((int64_t)y << a.shift) * a.full_w + ((int64_t)x << a.shift);
      lb |= (unsigned)lb8[at] << (8 * j);
    }
  }
  return lb;
}

template <bool BWD, int KIND, int TMAX>
__global__ __launch_bounds__(256, (BWD && TMAX > 4) ? 1 : 2) void ds_head_kernel(DsArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[256 * HLM_SCR * 4];
  __shared__ float cst[2][HSG_NCST<BWD, KIND>];
  __shared__ u32x4 wlog[TMAX][4][64];             // per tile: logits hi (k-steps 0, 1), lo (k-steps 0, 1)
  __shared__ u32x4 wdz[BWD ? TMAX : 1][2][64];    // per tile: dz hi, lo
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane & 31, h = lane >> 5;
  const int n = blockIdx.y, chunk = blockIdx.x;
  const int nv = min(8, max(0, a.ncls - 8 * h));  // classes of this lane half
  const HsgLoss c = {a.bias, a.cls_weight, a.saved, a.dloss, a.eps, a.ncls, a.sigmoid, a.ignore};

  // ---- weight operands of every tile (head_seg_kernel's, columns 32 t .. of W at row stride cin), the waves taking tiles in turn,
  // and the constants of a lane half
  const HlmRow r(lane);
  const int lrow = (r.q < 2 && r.out() < a.ncls) ? r.out() : -1;
  for (int t = wv; t < a.tiles; t += 4) {
    hlm_logit_operands(wlog[t], a.W, lrow, lane, a.cin, 32 * t);
    if constexpr (BWD) hlm_dz_operand(wdz[t][0][lane], wdz[t][1][lane], a.W, 8 * h, a.ncls - 8 * h, r.channel(), a.cin, 32 * t);
  }
  if (wv == 2) hsg_constants<BWD, KIND>(cst, lane, c);
  __syncthreads();
  // (made opaque inside the loops: left alone, the compiler hoists the loop-invariant fragments into registers for the whole kernel)
  const u32x4* wlbase = &wlog[0][0][lane];
  const u32x4* wdbase = &wdz[0][0][lane];
  const float* cbase = &cst[h][0];
  // ---- accumulators ---------------------------------------------------------------------------------------------------
  float dI[8], dD[8], dbc[8];
  f32x16 accw[BWD ? TMAX : 1];
  bool bad = false;
#pragma unroll
  for (int e = 0; e < 8; ++e) dI[e] = dD[e] = dbc[e] = 0.f;
#pragma unroll
  for (int t = 0; t < (BWD ? TMAX : 1); ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) accw[t][i] = 0.f;

  const HlmTiles tiles(smem, wv, lane);
  float* const ce_acc = reinterpret_cast<float*>(smem) + tid * HLM_SCR + 16;  // (the forward has no tiles)
  if constexpr (KIND != HLM_DICE && !BWD) ce_acc[0] = ce_acc[1] = 0.f;
  if constexpr (BWD) tiles.zero_dl(lane);  // (columns 16 .. 31 of the dl tiles are never written)

  const size_t sample = (size_t)n * a.spatial * a.cin;
  const elt* zs = a.z + sample;
  const elt* ps = (BWD && a.d_pass) ? a.d_pass + sample : nullptr;
  elt* dzs = BWD ? a.dz + sample : nullptr;
  const uint8_t* lb8 = a.lab + (int64_t)n * a.lab_sn;
  const int run_end = min(a.runs, (chunk + 1) * a.chunk_runs);
  const u32x4 zero4 = {0u, 0u, 0u, 0u};

  for (int run = chunk * a.chunk_runs + wv; run < run_end; run += 4) {
    const size_t vb = (size_t)run * HLM_RUN + 4 * g;
    const bool live = vb < a.spatial;  // (spatial % 4 == 0: all four voxels or none)
    const elt* zrow = zs + vb * a.cin + 8 * h;
    const unsigned lb = ds_pick4(a, lb8, (unsigned)vb, live);

    // ---- logits of the run's four sub-tiles, accumulated over the channel tiles
    f32x16 lg[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) lg[j][i] = 0.f;
#pragma unroll 1
    for (int t = 0; t < a.tiles; ++t) {
      asm volatile("" : "+v"(wlbase));
      u32x4 zp[4][2];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int s = 0; s < 2; ++s)
          zp[j][s] = live ? *reinterpret_cast<const u32x4*>(zrow + (size_t)j * a.cin + 32 * t + 16 * s) : zero4;
      const u32x4* wt = wlbase + t * 4 * 64;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const eltx8 zb = __builtin_bit_cast(eltx8, zp[j][s]);
          lg[j] = MEDNET_MFMA_32x32x16(hlm_wop(wt, s), zb, lg[j], 0, 0, 0);
          lg[j] = MEDNET_MFMA_32x32x16(hlm_wop(wt, 2 + s), zb, lg[j], 0, 0, 0);
        }
    }

    eltx8 dch[BWD ? 4 : 1], dcl[BWD ? 4 : 1];  // backward: the logit gradient of the sub-tiles, hi + lo
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      asm volatile("" : "+v"(cbase));
      float lc[8], p[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) lc[e] = lg[j][e] + cbase[e];
      const int yl = (int)((lb >> (8 * j)) & 0xFFu);
      const int yk = yl - 8 * h;  // the label's slot in this half, if in 0 .. nv-1
      float lse;
      hsg_probs<KIND>(lc, nv, a.sigmoid, p, lse);
      if constexpr (!BWD) hsg_fwd_terms<KIND>(c, p, lc, lse, yl, yk, nv, live, h, cbase, ce_acc, dI, dD, bad);
      else hsg_logit_grad<KIND>(c, p, yl, yk, nv, live, cbase, dbc, dch[j], dcl[j]);
    }

    if constexpr (BWD) {
      // ---- per channel tile: dz^T = W_t^T dl^T + d_pass, rounded once and stored; dW_t += dl^T z_t
      elt* dzrow = dzs + vb * a.cin + 8 * h;
      const elt* prow = ps ? ps + vb * a.cin + 8 * h : nullptr;
#pragma unroll
      for (int t = 0; t < TMAX; ++t) {
        if (t < a.tiles) {
          asm volatile("" : "+v"(wdbase));
          const u32x4* wt = wdbase + t * 2 * 64;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            u32x4 zp[2], pp[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
              const size_t at = (size_t)j * a.cin + 32 * t + 16 * s;
              zp[s] = live ? *reinterpret_cast<const u32x4*>(zrow + at) : zero4;
              pp[s] = (live && prow) ? *reinterpret_cast<const u32x4*>(prow + at) : zero4;
            }
            const f32x16 dzv = hlm_dz(hlm_wop(wt, 0), hlm_wop(wt, 1), dch[j], dcl[j]);
            const eltx8 p0 = __builtin_bit_cast(eltx8, pp[0]), p1 = __builtin_bit_cast(eltx8, pp[1]);
            eltx8 o0, o1;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              o0[e] = (elt)(dzv[e] + (float)p0[e]);
              o1[e] = (elt)(dzv[8 + e] + (float)p1[e]);
            }
            if (live) {
              elt* out = dzrow + (size_t)j * a.cin + 32 * t;
              *reinterpret_cast<u32x4*>(out) = __builtin_bit_cast(u32x4, o0);
              *reinterpret_cast<u32x4*>(out + 16) = __builtin_bit_cast(u32x4, o1);
            }
            tiles.dw_step(g, h, zp, dch[j], dcl[j], nullptr, nullptr, accw[t]);
          }
        }
      }
    }
  }

  // ---- end of kernel: lane and wave sums through LDS in a fixed order (head_seg_kernel's) ---------------------------------
  float* scr = reinterpret_cast<float*>(smem);
  __syncthreads();
  if constexpr (!BWD) {
    hsg_fwd_writeout<KIND>(scr, tid, dI, dD, bad, a.ce_partial, a.dice_partial, (size_t)n * a.chunks + chunk, a.ncls);
  } else {
    // per tile a row of head_lm_kernel's shape: dW row k' = class k' (accumulator values 0 .. 7 of a lane), db at 1024 + k'
    float* mine = scr + tid * HLM_SCR;
    float* wp = a.wpart + ((size_t)n * a.chunks + chunk) * a.tiles * HLM_WIDTH;
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
      if (t < a.tiles) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          mine[i] = accw[t][i];
          mine[8 + i] = dbc[i];
        }
        hlm_dw_db_writeout<8, HSG_MAXC>(scr, tid, wp + (size_t)t * HLM_WIDTH);
        __syncthreads();
      }
    }
  }
}


// dw[co][32 t + c] = sum over the workgroups' rows of wpart[.][t][co * 32 + c], db[co] of wpart[.][0][1024 + co]: one thread per
// output, the rows in order, in fp64 (deterministic)
__global__ __launch_bounds__(256) void ds_head_wfinal_kernel(const float* __restrict__ wpart, int rows, int tiles, int ncls,
                                                            float* __restrict__ dw, float* __restrict__ db) {
  const int cin = 32 * tiles, nw = ncls * cin;
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= nw + ncls || (o >= nw && !db)) return;
  const int co = o < nw ? o / cin : o - nw, ci = o < nw ? o % cin : 0;
  const size_t src = o < nw ? (size_t)(ci >> 5) * HLM_WIDTH + co * 32 + (ci & 31) : (size_t)1024 + co;
  const size_t stride = (size_t)tiles * HLM_WIDTH;
  double acc = 0.0;
  for (int r = 0; r < rows; ++r) acc += (double)wpart[(size_t)r * stride + src];
  if (o < nw) dw[o] = (float)acc;
  else db[co] = (float)acc;
}

// ---- host side -------------------------------------------------------------------------------------------------------
bool ds_head_supported(int cin, int ncls, int dtype, size_t spatial) {
  return cin >= 64 && cin <= 32 * DSH_MAXT && cin % 32 == 0 && ncls >= 1 && ncls <= HSG_MAXC && dtype == ELT_DTYPE && spatial % 4 == 0 &&
         spatial < ((size_t)1 << 31) && tuning_option("ds_head_fuse", 1);
}
// A coarse level is small: 16 runs (4 trips per wave) per workgroup keep a 64^3 x 4 level at two workgroups per CU, where
// head_lm_plan's 64 would leave half the CUs idle
static void ds_head_plan(size_t spatial, int& runs, int& chunk_runs, int& chunks) {
  runs = (int)((spatial + HLM_RUN - 1) / HLM_RUN);
  chunk_runs = 16;
  chunks = (runs + chunk_runs - 1) / chunk_runs;
}
int ds_head_chunks(size_t spatial) {
  int runs, cr, chunks;
  ds_head_plan(spatial, runs, cr, chunks);
  return chunks;
}
size_t ds_head_ws_bytes(int n, size_t spatial, int cin, int ncls) {
  const size_t chunks = ds_head_chunks(spatial);
  const size_t fwd = (size_t)n * chunks * (2 * ncls + 2);  // Dice rows [n][chunk][ncls][2] and / or CE rows [n][chunk][2]
  const size_t bwd = (size_t)n * chunks * (cin / 32) * HLM_WIDTH;
  return ((fwd > bwd ? fwd : bwd) + 64) * sizeof(float);
}

static void ds_args(DsArgs& a, const void* z, const float* W, const float* bias, const void* lab, int64_t lab_sn,
                    const float* cls_weight, int d, int h, int w, int H, int Wf, int shift, int cin, int ncls, int sigmoid, int ignore) {
  a.z = (const elt*)z; a.W = W; a.bias = bias; a.lab = (const uint8_t*)lab; a.lab_sn = lab_sn; a.cls_weight = cls_weight;
  a.full_w = Wf; a.full_hw = (int64_t)H * Wf; a.lev_w = (unsigned)w; a.lev_hw = (unsigned)h * (unsigned)w; a.shift = shift;
  a.spatial = (size_t)d * h * w; a.cin = cin; a.tiles = cin / 32; a.ncls = ncls;
  ds_head_plan(a.spatial, a.runs, a.chunk_runs, a.chunks);
  a.sigmoid = sigmoid; a.ignore = ignore;
}

// `partial`: [n][chunk][ncls][2] (Dice), [n][chunk][2] (CE), the first followed by the second for Dice + CE (launch_head_seg_fwd's)
int launch_ds_head_fwd(const void* z, const float* W, const float* bias, const void* lab, int64_t lab_sn, const float* cls_weight,
                       float* partial, int n, int d, int h, int w, int H, int Wf, int shift, int cin, int ncls, int ce, int sigmoid,
                       int ignore, hipStream_t s) {
  DsArgs a = {};
  ds_args(a, z, W, bias, lab, lab_sn, cls_weight, d, h, w, H, Wf, shift, cin, ncls, sigmoid, ignore);
  (ce == HLM_CE ? a.ce_partial : a.dice_partial) = partial;
  if (ce == HLM_DICE_CE) a.ce_partial = partial + (size_t)n * a.chunks * ncls * 2;
  for_class_kind(ce, [&](auto kind) {
    hipLaunchKernelGGL((ds_head_kernel<false, decltype(kind)::value, DSH_MAXT>), dim3(a.chunks, n), dim3(256), 0, s, a);
  });
  return check_launch(MEDNET_CLASS_KIND_NAME(ce, "ds_head", "_fwd"));
}

int launch_ds_head_bwd(const void* z, const float* W, const float* bias, const void* lab, int64_t lab_sn, const float* saved,
                       const float* cls_weight, const float* dloss, float eps, const void* d_pass, void* dz, float* dw, float* db, int n,
                       int d, int h, int w, int H, int Wf, int shift, int cin, int ncls, int ce, int sigmoid, int ignore, void* ws,
                       size_t ws_bytes, hipStream_t s) {
  DsArgs a = {};
  ds_args(a, z, W, bias, lab, lab_sn, cls_weight, d, h, w, H, Wf, shift, cin, ncls, sigmoid, ignore);
  MEDNET_REQUIRE(ws_bytes >= ds_head_ws_bytes(n, a.spatial, cin, ncls), MEDNET_E_WORKSPACE, "ds_head_bwd: workspace too small");
  a.saved = saved; a.dloss = dloss; a.eps = eps; a.d_pass = (const elt*)d_pass; a.dz = (elt*)dz; a.wpart = (float*)ws;
  for_class_kind(ce, [&](auto kind) {
    constexpr int KIND = decltype(kind)::value;
    if (a.tiles <= 4) hipLaunchKernelGGL((ds_head_kernel<true, KIND, 4>), dim3(a.chunks, n), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((ds_head_kernel<true, KIND, DSH_MAXT>), dim3(a.chunks, n), dim3(256), 0, s, a);
  });
  int rc = check_launch(MEDNET_CLASS_KIND_NAME(ce, "ds_head", "_bwd"));
  if (rc) return rc;
  const int total = ncls * cin + ncls;
  hipLaunchKernelGGL(ds_head_wfinal_kernel, dim3((total + 255) / 256), dim3(256), 0, s, a.wpart, n * a.chunks, a.tiles, ncls, dw, db);
  return check_launch("ds_head_wfinal");
}

}  // namespace mednet
