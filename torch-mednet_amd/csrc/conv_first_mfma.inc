// The first layer (Cin = 1, 2, 3, 4) of the 16-bit modes on the matrix cores: forward with its fused GroupNorm pair sums, and the
// weight gradient in its plain and GroupNorm form.  Included by conv_mfma.hip inside namespace mednet (so once per element type).
// DESIGN.md sections 4 and 16.
//
// Forward:  y[v][co] = sum_ci sum_tap W[co][ci][tap] * x_ci[v + tap - 1].  With so few input channels the contraction index is
// the TAP (27, padded to 32 = two MFMA k-steps) per channel: 2 * Cin k-steps of MFMA_32x32x16.  The B operand (k = tap, n = voxel)
// is gathered from a halo brick of x in LDS -- 8 scalar LDS reads per fragment -- in its elt high and low parts (x = hi + lo to
// ~2^-17), so the network input keeps fp32-level precision at 4 MFMAs per 32 voxels and channel; under SPLIT the weights' low part
// is multiplied too.  The weights (Cin x 32 x 32 elt) live in registers for the kernel's lifetime.  The kernel is bound by writing
// its output (32 channels per input voxel); the VALU formulation it replaced was 4x slower.
// The input is read where it lies: element (v, ci) of a sample sits at v * sv + ci * sc -- planar N x C x D x H x W (sv = 1,
// sc = D H W) or channels-last (sv = Cin, sc = 1) -- through a per-sample buffer resource; positions outside the volume get an
// out-of-range offset and come back as zeros.  One channel may also arrive in the storage type (x16).
// PERSISTENT (round 6).  With one short-lived workgroup per brick, 63 % of the instruction stream was per-brick fixed cost -- the
// weight fragments and tap offsets (21 %) and the reduction of the 32 statistics sums over the wave (42 %) -- in a kernel that
// is instruction-bound (252 us for 537 MB of output).  Now at most 4 workgroups per CU walk the (brick, channel block) items:
// weights and offsets are made once, the next brick's halo values are in flight (registers) while the current brick is on the
// matrix cores, and a wave keeps its sums over all its bricks of a sample: one partial row per wave, workgroup and sample.
// The output is bit-identical to the one-brick-per-workgroup form (same MFMA sequence per voxel); option conv_c1_persist=0
// launches a workgroup per item.  No atomics.
struct FirstArgs {
  const void* x;      // N samples of Cin x D x H x W (planar) or D x H x W x Cin (channels-last): fp32, or elt when x16
  const float* w;     // packed forward image Pf[tap][ci][co] (fp32)
  elt* y;             // NDHWC
  float* gn_partial;  // nullable: [n][4 * gridDim.x / ncb][cout][2] per-wave {sum y, sum y^2} of the stored values
  int n, d, h, w_, cout;
  int tiles_z, tiles_y, tiles_x, ntiles, ncb;
  unsigned rcp_tiles_x, rcp_tiles_y, rcp_tiles_z, rcp_ncb;
  unsigned sv4, sc4;  // byte strides of a voxel and of a channel inside one sample
  unsigned bytes_x;   // one sample of x, all channels
  int x16;            // Cin = 1 only: x holds elt values (the 1-channel output of a GroupNorm in the 'gcr' orders), else fp32
};

// one element of x at byte `off` of a sample; the 16-bit form exists in the one-channel kernels only
template <int CIN, typename Rsrc>
__device__ __forceinline__ float first_load_x(Rsrc rsrc, unsigned off, int x16) {
  if constexpr (CIN == 1) {
    if (x16) {  // (workgroup-uniform) a 16-bit buffer load of the element, widened
      const unsigned short raw = __builtin_amdgcn_raw_buffer_load_b16(rsrc, off, 0, 0);
      return (float)__builtin_bit_cast(elt, raw);
    }
  }
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, off, 0, 0));
}

// waves per SIMD (= workgroups of 256 per CU) the registers leave room for.  One channel: four (128 registers per lane; SPLIT is
// compiled apart so that the default form keeps no registers for the weights' low parts).  More: the weights take 8 per channel,
// twice that under SPLIT, and the halo values in flight 5 per channel -- 147 to 161 registers without SPLIT (three workgroups, 168
// each; Cin = 2 spilled at the 128 of four), 183 and 191 for SPLIT with Cin = 3, 4 (two).  DESIGN.md section 16 has the counts the
// compiler reports.
constexpr int first_fwd_waves(int cin, bool split) { return cin == 1 ? 4 : split && cin >= 3 ? 2 : 3; }

template <int CIN, bool SPLIT>
__global__ __launch_bounds__(256, first_fwd_waves(CIN, SPLIT)) void conv_first_mfma_kernel(FirstArgs a) {
  constexpr int TZ = 4, TY = 8, TX = 16, HZ = TZ + 2, HY = TY + 2, HX = TX + 2, NV = HZ * HY * HX, NTW = 4;
  static_assert(NTW == TY / 2 && TZ == 4, "a wave owns one z-plane of the brick");
  constexpr int IN_ROUNDS = (NV + 255) / 256;
  constexpr unsigned OOB = 0xFFFFFF00u;
  // one halo brick per channel, ALREADY split into its elt high and low parts: every halo value feeds up to 27 taps, and split
  // where it is gathered (round 1-5) the two conversions and the subtraction ran once per tap, tile and k-step
  __shared__ elt xs_hi[CIN * NV], xs_lo[CIN * NV];
  __shared__ __attribute__((aligned(16))) elt epi[4 * 1024];  // per wave: one tile of 32 voxels x 32 channels on its way out
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
  // items (brick, channel block) = item / ncb, item % ncb; gridDim.x is a multiple of ncb: a workgroup keeps its channel block
  const int cb = (int)(blockIdx.x % a.ncb);
  const int nitems = a.ntiles * a.ncb;
  // weights: A operand of k-step (ci, ks): lane (co = r, h) holds taps 16 ks + 8h .. + 7 of channel ci; taps >= 27 are 0
  eltx8 wa[CIN][2], wl[SPLIT ? CIN : 1][2];
#pragma unroll
  for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int tap = ks * 16 + 8 * h + j;
        // (a 16-channel layer fills half a block)
        const float wf = tap < 27 && cb * 32 + r < a.cout ? a.w[((size_t)tap * CIN + ci) * a.cout + cb * 32 + r] : 0.f;
        wa[ci][ks][j] = (elt)wf;
        if constexpr (SPLIT) wl[ci][ks][j] = (elt)(wf - (float)wa[ci][ks][j]);
      }
  // LDS offsets of this lane's 8 taps per k-step (every channel's brick has the same shape)
  int toff[2][8];  // (both k-halves' offsets are compile-time constants: one select per entry instead of the divisions by 9 and 3)
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int t0 = ks * 16 + j, t1 = ks * 16 + 8 + j;
      const int o0 = t0 < 27 ? ((t0 / 9) * HY + (t0 / 3) % 3) * HX + t0 % 3 : 0, o1 = t1 < 27 ? ((t1 / 9) * HY + (t1 / 3) % 3) * HX + t1 % 3 : 0;
      toff[ks][j] = h ? o1 : o0;
    }
  // this thread's halo positions (the same for every brick): hz << 16 | hy << 8 | hx; slots past the halo fail every range check
  int hpos[IN_ROUNDS];
#pragma unroll
  for (int k = 0; k < IN_ROUNDS; ++k) {
    const int i = tid + 256 * k;
    hpos[k] = i < NV ? ((i / (HX * HY)) << 16) | (((i / HX) % HY) << 8) | (i % HX) : 0x7FFF0000;
  }
  auto origin = [&](int item, int& n, int& tz0, int& ty0, int& tx0) {
    int tt = fastdiv(item, a.ncb, a.rcp_ncb);
    int qd = fastdiv(tt, a.tiles_x, a.rcp_tiles_x);
    tx0 = (tt - qd * a.tiles_x) * TX;
    tt = qd;
    qd = fastdiv(tt, a.tiles_y, a.rcp_tiles_y);
    ty0 = (tt - qd * a.tiles_y) * TY;
    tt = qd;
    qd = fastdiv(tt, a.tiles_z, a.rcp_tiles_z);
    tz0 = (tt - qd * a.tiles_z) * TZ;
    n = qd;
  };
  // halo values of a brick: buffer loads through a per-sample resource (no bytes at all for a brick that does not exist)
  float xin[CIN][IN_ROUNDS];
  auto fetch = [&](int item, bool valid) {
    int n, tz0, ty0, tx0;
    origin(item, n, tz0, ty0, tx0);
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(reinterpret_cast<const char*>(a.x) + (size_t)n * a.bytes_x), 0,
                                                        a.bytes_x & (0u - (unsigned)valid), 0x00020000);
#pragma unroll
    for (int k = 0; k < IN_ROUNDS; ++k) {
      const int gz = tz0 - 1 + (hpos[k] >> 16), gy = ty0 - 1 + ((hpos[k] >> 8) & 255), gx = tx0 - 1 + (hpos[k] & 255);
      const bool in_vol = ((unsigned)gz < (unsigned)a.d) & ((unsigned)gy < (unsigned)a.h) & ((unsigned)gx < (unsigned)a.w_);
      const unsigned off = (unsigned)((gz * a.h + gy) * a.w_ + gx) * a.sv4;
#pragma unroll
      for (int ci = 0; ci < CIN; ++ci) xin[ci][k] = first_load_x<CIN>(rsrc, in_vol ? off + ci * a.sc4 : OOB, a.x16);
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int k = 0; k < IN_ROUNDS; ++k) {
      const int i = tid + 256 * k;
      if (i < NV) {
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) {
          const elt xh = (elt)xin[ci][k];
          xs_hi[ci * NV + i] = xh;
          xs_lo[ci * NV + i] = (elt)(xin[ci][k] - (float)xh);
        }
      }
    }
  };
  const size_t vol = (size_t)a.d * a.h * a.w_;
  // fused GroupNorm statistics, as in conv_mfma_kernel: per channel PAIR (v_dot2c_f32: two exact products + fp32 add per
  // instruction), taken from the stored 64-byte rows -- lane = (voxel, 16-byte piece lane & 3) -- over the wave's tiles of a sample;
  // entry 2j of the partial row gets the sums of channels 2j and 2j + 1, entry 2j + 1 is zero (GroupNorm only adds the channels of a
  // group; the host asks for fused partials only when the channels per group are even).  Until round 6: 32 per-channel sums per
  // lane from the accumulators, reduced over the wave once per BRICK -- 42 % of the kernel's instructions.
  typedef __attribute__((ext_vector_type(2))) elt eltx2;
  const eltx2 ones = {(elt)1.0f, (elt)1.0f};
  float gs[4], gq[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) gs[k] = gq[k] = 0.f;
  int acc_n = 0;
  auto flush = [&](int nn) {  // one row per wave: sum over the 16 lanes that share a piece (DPP / v_permlane steps: plain VALU)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      gs[k] = lane_class_sum<4>(gs[k]);
      gq[k] = lane_class_sum<4>(gq[k]);
    }
    const int pjl = lane & 3;
    if (lane < 4 && cb * 32 + pjl * 8 < a.cout) {
      const int rows = 4 * (int)(gridDim.x / a.ncb);
      float* dst = a.gn_partial + (((size_t)nn * rows + (blockIdx.x / a.ncb) * 4 + wv) * a.cout + cb * 32 + pjl * 8) * 2;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const f32x4 o = {gs[k], gq[k], 0.f, 0.f};
        *reinterpret_cast<f32x4*>(dst + k * 4) = o;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) gs[k] = gq[k] = 0.f;
  };

  int item = blockIdx.x;  // (the launcher never starts more workgroups than items)
  fetch(item, true);
  while (true) {
    int n, tz0, ty0, tx0;
    origin(item, n, tz0, ty0, tx0);
    const int nitem = item + (int)gridDim.x;
    const bool has_next = nitem < nitems;
    if (a.gn_partial) {
      while (acc_n < n) {  // (workgroup-uniform) a new sample: the finished one's row goes out, zero rows for skipped samples
        flush(acc_n);
        ++acc_n;
      }
    }
    __syncthreads();  // every wave is done gathering from the previous brick
    commit();
    __syncthreads();
    fetch(has_next ? nitem : item, has_next);  // in flight while this brick is on the matrix cores
    // (a rolled loop: unrolled inside the item loop, the compiler hoists the 4 x 16 gather addresses, which are the same for every
    //  brick, out of it and spills 181 registers at the 128 that four workgroups per CU leave)
#pragma unroll 1
    for (int t = 0; t < NTW; ++t) {
      const int g = wv * NTW + t;
      const int lz = wv, ly = t * 2 + (r >> 4), lx = r & 15;  // (N-tile g = wv * 4 + t: z-plane g / 4, rows 2 (g % 4), + 1)
      const int oz_t = tz0 + lz;
      const int base = (lz * HY + ly) * HX + lx;
      f32x16 acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
      for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          eltx8 hi, lo;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            hi[j] = xs_hi[ci * NV + base + toff[ks][j]];
            lo[j] = xs_lo[ci * NV + base + toff[ks][j]];
          }
          acc = MEDNET_MFMA_32x32x16(wa[ci][ks], hi, acc, 0, 0, 0);
          acc = MEDNET_MFMA_32x32x16(wa[ci][ks], lo, acc, 0, 0, 0);
          if constexpr (SPLIT) acc = MEDNET_MFMA_32x32x16(wl[ci][ks], hi, acc, 0, 0, 0);
        }
      // The accumulator layout gives a lane four 8-byte pieces (channels 8q + 4h ..) of ITS voxel's 64-byte row: stored as they
      // stand, one instruction touches 64 rows with 8 bytes each, and this kernel does little else than store.
      // The tile goes through 2 KB of LDS private to the wave (8-byte pieces XOR-swizzled by voxel: conflict-free both ways, no
      // barrier -- a wave's LDS operations execute in order, the fence keeps the compiler from reordering them) and leaves as whole
      // rows: 4 lanes per voxel, 16 voxels = one x-row of the brick = 1 KB contiguous per instruction when Cout = 32.
      elt* tile_lds = epi + wv * 1024;
      wave_lds_fence();  // (the previous tile's row reads stay above these writes)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        eltx4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (elt)acc[q * 4 + j];
        *reinterpret_cast<eltx4*>(tile_lds + r * 32 + (((2 * q + h) ^ ((r >> 2) & 7)) * 4)) = o;
      }
      wave_lds_fence();
      eltx8 rows2[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int v = i * 16 + (lane >> 2), sw = (v >> 2) & 7;
        eltx8 rv = *reinterpret_cast<const eltx8*>(tile_lds + v * 32 + (((lane & 3) ^ (sw >> 1)) * 8));
        if (sw & 1) rv = __builtin_shufflevector(rv, rv, 4, 5, 6, 7, 0, 1, 2, 3);
        rows2[i] = rv;
      }
      wave_lds_fence();
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int v = i * 16 + (lane >> 2);
        const int sy = ty0 + (g % (TY / 2)) * 2 + (v >> 4), sx = tx0 + (v & 15);
        const bool ok = oz_t < a.d && sy < a.h && sx < a.w_ && cb * 32 + (lane & 3) * 8 < a.cout;
        if (ok)
          __builtin_nontemporal_store(rows2[i], reinterpret_cast<eltx8*>(a.y + ((size_t)n * vol + ((size_t)oz_t * a.h + sy) * a.w_ + sx) * a.cout + cb * 32 + (lane & 3) * 8));
        const eltx8 vz = ok ? rows2[i] : eltx8{};  // statistics of what is stored
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const eltx2 pr = {vz[2 * k], vz[2 * k + 1]};
          gs[k] = MEDNET_FDOT2(pr, ones, gs[k], false);
          gq[k] = MEDNET_FDOT2(pr, pr, gq[k], false);
        }
      }
    }
    if (!has_next) break;
    item = nitem;
  }
  if (a.gn_partial) {
    while (acc_n < a.n) {  // the last sample of this workgroup, then zero rows for the samples after it
      flush(acc_n);
      ++acc_n;
    }
  }
}

// One channel arrives as fp32 (the network input) or in the storage type, in either layout (they coincide); 2 to 4 as fp32.
bool conv_first_mfma_supported(int cin, int cout, int ksize, int x_dtype, int y_dtype, int y_layout, bool bias) {
  return cin >= 1 && cin <= 4 && ksize == 3 && cout % 16 == 0 && (x_dtype == MEDNET_F32 || (cin == 1 && x_dtype == ELT_DTYPE)) &&
         y_dtype == ELT_DTYPE && y_layout == MEDNET_NDHWC && !bias;
}
// workgroups of a launch: 4, 3 or 2 per CU -- whichever leaves the last round of the walk fullest (the item count of config 5's
// first layer, 14 400, is 14.06 rounds of 1024 workgroups: 15 rounds with the last one 6 % full, measured 6 % slower than 18.75
// rounds of 768) -- rounded down to a multiple of the channel-block count so that a workgroup keeps its block; one per (brick,
// channel block) item when there are no more items than that, or with option conv_c1_persist=0
static int conv_c1_grid(int n, int d, int h, int w, int cout) {
  const int ncb = (cout + 31) / 32;
  const int nitems = n * ((d + 3) / 4) * ((h + 7) / 8) * ((w + 15) / 16) * ncb;
  const int cus = ::mednet_internal_cu_count() > 0 ? ::mednet_internal_cu_count() : 256;
  if (!tuning_option("conv_c1_persist", 1) || nitems <= 4 * cus) return nitems;
  int best = 0;
  double best_fill = 0.0;
  for (int per_cu = 4; per_cu >= 2; --per_cu) {
    const int g = per_cu * cus / ncb * ncb;
    if (g <= 0) continue;
    const double fill = (double)nitems / ((double)((nitems + g - 1) / g) * g);
    if (fill > best_fill + 0.01) {  // (more workgroups per CU hide more latency: fewer only for a clearly fuller last round)
      best = g;
      best_fill = fill;
    }
  }
  return best > 0 ? best : nitems;
}
// partial rows per sample: 4 (one per wave) per workgroup of a channel block
int conv_first_stats_chunks(int n, int d, int h, int w, int cout) { return 4 * (conv_c1_grid(n, d, h, w, cout) / ((cout + 31) / 32)); }
int launch_conv_first_mfma(const void* x, int x_layout, int x_dtype, const float* w_pf, void* y, int n, int d, int h, int w, int cin,
                           int cout, float* gn_partial, hipStream_t s, int split) {
  const char* who = cin == 1 ? "conv_c1_mfma" : "conv_cm_mfma";
  MEDNET_REQUIRE(cin >= 1 && cin <= 4 && (cin == 1 || x_dtype == MEDNET_F32), MEDNET_E_UNSUPPORTED,
                 "conv_first_mfma: cin=%d (1 to 4; 16-bit x with one channel only)", cin);
  FirstArgs a;
  a.gn_partial = gn_partial;
  a.x = x;
  a.x16 = x_dtype != MEDNET_F32;
  a.w = w_pf;
  a.y = (elt*)y;
  a.n = n; a.d = d; a.h = h; a.w_ = w; a.cout = cout;
  a.tiles_z = (d + 3) / 4;
  a.tiles_y = (h + 7) / 8;
  a.tiles_x = (w + 15) / 16;
  a.ntiles = n * a.tiles_z * a.tiles_y * a.tiles_x;
  a.ncb = (cout + 31) / 32;
  a.rcp_tiles_x = fastdiv_rcp(a.tiles_x); a.rcp_tiles_y = fastdiv_rcp(a.tiles_y); a.rcp_tiles_z = fastdiv_rcp(a.tiles_z); a.rcp_ncb = fastdiv_rcp(a.ncb);
  MEDNET_REQUIRE((double)a.ntiles * a.ncb * 1024.0 < 4294967296.0, MEDNET_E_UNSUPPORTED, "%s: grid too large", who);
  MEDNET_REQUIRE((double)d * h * w * cin * 4.0 < 4294960000.0, MEDNET_E_UNSUPPORTED, "%s: one input sample must stay below 4 GB", who);
  const size_t vol = (size_t)d * h * w;
  const unsigned esz = a.x16 ? 2u : 4u;
  a.bytes_x = (unsigned)(vol * cin * esz);
  a.sv4 = x_layout == MEDNET_NCDHW ? esz : esz * (unsigned)cin;
  a.sc4 = x_layout == MEDNET_NCDHW ? (unsigned)(vol * esz) : esz;
  const dim3 grid((unsigned)conv_c1_grid(n, d, h, w, cout));
#define FIRST_GO(CIN_)                                                                             \
  do {                                                                                             \
    if (split) hipLaunchKernelGGL((conv_first_mfma_kernel<CIN_, true>), grid, dim3(256), 0, s, a); \
    else hipLaunchKernelGGL((conv_first_mfma_kernel<CIN_, false>), grid, dim3(256), 0, s, a);      \
  } while (0)
  if (cin == 1) FIRST_GO(1);
  else if (cin == 2) FIRST_GO(2);
  else if (cin == 3) FIRST_GO(3);
  else FIRST_GO(4);
#undef FIRST_GO
  return check_launch(who);
}

// ---- weight gradient: dW[co][ci][tap] = sum_v x_ci[v + tap - 1] * dy[v][co] ------------------------------------------------------
//   D_ci[tap (27 of 32 rows)][co] += A_ci[tap][k = voxel] * B[k = voxel][co], one accumulator tile per input channel.
// B comes from the dy brick in LDS through the transposing read (as in wgrad_mfma2); A is gathered from an fp32 halo brick of x_ci
// (lane = tap row: 8 consecutive x-values of its shifted row) and split into elt hi + lo parts (two MFMAs), so the network input
// keeps fp32-level precision.  The dy brick is read from HBM once per launch and staged once per brick; all Cin halo bricks of x
// are contracted against the one B operand read from it.  The kernel is bound by reading dy (537 MB at config 2); the VALU kernel
// it replaced (27 FMAs per voxel and channel) took 0.65 ms.  One partial block [co][ci][27] per workgroup, then reduce_chunks_kernel.
struct WfirstArgs {
  const void* x;   // as FirstArgs::x
  const elt* dy;   // N x D x H x W x cout
  float* part;     // [workgroup][cout][cin][27]
  int n, d, h, w, cout;
  int tiles_z, tiles_y, tiles_x, ntiles;
  unsigned rcp_tiles_x, rcp_tiles_y, rcp_tiles_z;
  unsigned sv4, sc4, bytes_x, bytes_dy;  // byte strides inside a sample of x; bytes per sample
  int x16;                               // as FirstArgs::x16
  // GN form: `dy` holds dz (the gradient of the layer's activated, normalised output) and the kernel applies GroupNorm's
  // backward while it stages:  dy = k1 * dz * act'(ca * y + cb) + k2 * y + k3, rounded to elt -- the value
  // norm_act.hip's gn_bwd_apply_kernel would have stored, expression for expression -- so dy is never written or re-read
  const elt* y;        // N x D x H x W x cout: the convolution's output
  const float* coef;   // [n][cout][2] = {ca, cb}
  const float* bcoef;  // [n][cout][3] = {k1, k2, k3}
  int act;
};

// workgroups per CU.  One channel: two in every form.  More: Cin * NB accumulator tiles of 16 registers, up to 4 of them beside
// the staging registers at two workgroups per CU, more only at one (512 registers per lane; the LDS of Cin = 4, NB = 2 -- 81 KB --
// allows one anyway); the GN form stages dz and y, 64 NB registers in flight instead of 32 NB, so its Cin = 2, NB = 2 form needs
// the 512 too.  (At two, <1, 2, GN> spills 17 registers: DESIGN.md section 16.)
constexpr int wfirst_waves(int cin, int nb, bool gn) { return cin == 1 ? 2 : cin * nb > 4 || (gn && nb == 2) ? 1 : 2; }

template <int CIN, int NB, bool GN>  // NB: 32-channel blocks of dy
__global__ __launch_bounds__(256, wfirst_waves(CIN, NB, GN)) void wgrad_first_mfma_kernel(WfirstArgs a) {
  constexpr int TZ = 4, TY = 8, TX = 16, HZ = TZ + 2, HY = TY + 2, HX = TX + 2;
  constexpr int NJ = TZ * TY * TX, NH = HZ * HY * HX;
  constexpr int ROWB = 64 * NB;                         // bytes of one voxel row of dy in LDS
  constexpr int XH_BYTES = (NH * 4 + 255) / 256 * 256;  // fp32 halo brick of one channel of x
  constexpr int XH_F = XH_BYTES / 4;
  constexpr int DY_ROUNDS = NJ * 4 * NB / 256, X_ROUNDS = (NH + 255) / 256;
  typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* xh = reinterpret_cast<float*>(smem);  // [CIN][XH_F]
  char* dyl = smem + CIN * XH_BYTES;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hk = lane >> 5;
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int coloff = (16 * (g & 1) + 4 * p) * 2;
  const int tapc = r < 27 ? r : 26;  // rows 27..31 duplicate tap 26 and are dropped at write-out
  const int abase = ((tapc / 9) * HY + (tapc / 3) % 3) * HX + tapc % 3 + 8 * hk;

  constexpr unsigned OOB = 0xFFFFFF00u;
  u32x4 rdy[DY_ROUNDS];
  u32x4 ryy[GN ? DY_ROUNDS : 1];
  float rx[CIN][X_ROUNDS];
  // GN form: this thread's 8 channels are the same in every round (256 % (4 * NB) == 0)
  float gca[GN ? 8 : 1], gcb[GN ? 8 : 1], gk1[GN ? 8 : 1], gk2[GN ? 8 : 1], gk3[GN ? 8 : 1];
  unsigned in_mask = 0;  // bit `it`: round `it` of the fetched brick lies inside the volume
  int coef_n = -1;       // sample the coefficients in registers belong to
  auto fetch = [&](int tile) {
    int tt = tile;
    int qd = fastdiv(tt, a.tiles_x, a.rcp_tiles_x);
    const int tx0 = (tt - qd * a.tiles_x) * TX;
    tt = qd;
    qd = fastdiv(tt, a.tiles_y, a.rcp_tiles_y);
    const int ty0 = (tt - qd * a.tiles_y) * TY;
    tt = qd;
    qd = fastdiv(tt, a.tiles_z, a.rcp_tiles_z);
    const int tz0 = (tt - qd * a.tiles_z) * TZ;
    const size_t svox = (size_t)qd * a.d * a.h * a.w;
    const auto rD = __builtin_amdgcn_make_buffer_rsrc((void*)(a.dy + svox * a.cout), 0, a.bytes_dy, 0x00020000);
    const auto rY = __builtin_amdgcn_make_buffer_rsrc((void*)((GN ? a.y : a.dy) + svox * a.cout), 0, a.bytes_dy, 0x00020000);
    if constexpr (GN) {
      in_mask = 0;
      if (qd != coef_n) {  // (workgroup-uniform) first brick of a sample
        coef_n = qd;
        const int ch0 = (tid % (4 * NB)) * 8;
        if (ch0 < a.cout) {
          const float* pc = a.coef + ((size_t)qd * a.cout + ch0) * 2;
          const float* pb = a.bcoef + ((size_t)qd * a.cout + ch0) * 3;
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            gca[k] = pc[2 * k];
            gcb[k] = pc[2 * k + 1];
            gk1[k] = pb[3 * k];
            gk2[k] = pb[3 * k + 1];
            gk3[k] = pb[3 * k + 2];
          }
        }
      }
    }
    const auto rX = __builtin_amdgcn_make_buffer_rsrc((void*)(reinterpret_cast<const char*>(a.x) + (size_t)qd * a.bytes_x), 0, a.bytes_x, 0x00020000);
#pragma unroll
    for (int it = 0; it < DY_ROUNDS; ++it) {
      const int c = it * 256 + tid;
      const int part = c % (4 * NB), v = c / (4 * NB);
      const int gz = tz0 + v / (TX * TY), gy = ty0 + (v / TX) % TY, gx = tx0 + v % TX;
      const bool in_vol = (gz < a.d) & (gy < a.h) & (gx < a.w) & (part * 8 < a.cout);  // (a partial block: the rest of the row is zeros)
      const unsigned off = ((unsigned)((gz * a.h + gy) * a.w + gx) * (unsigned)a.cout + part * 8) * 2u;
      rdy[it] = __builtin_amdgcn_raw_buffer_load_b128(rD, in_vol ? off : OOB, 0, 0);
      if constexpr (GN) {
        ryy[it] = __builtin_amdgcn_raw_buffer_load_b128(rY, in_vol ? off : OOB, 0, 0);
        in_mask |= in_vol ? 1u << it : 0u;
      }
    }
#pragma unroll
    for (int it = 0; it < X_ROUNDS; ++it) {
      const int v = it * 256 + tid;
      const int gz = tz0 - 1 + v / (HX * HY), gy = ty0 - 1 + (v / HX) % HY, gx = tx0 - 1 + v % HX;
      const bool in_vol = (v < NH) & ((unsigned)gz < (unsigned)a.d) & ((unsigned)gy < (unsigned)a.h) & ((unsigned)gx < (unsigned)a.w);
      const unsigned off = (unsigned)((gz * a.h + gy) * a.w + gx) * a.sv4;
#pragma unroll
      for (int ci = 0; ci < CIN; ++ci) rx[ci][it] = first_load_x<CIN>(rX, in_vol ? off + ci * a.sc4 : OOB, a.x16);
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int it = 0; it < DY_ROUNDS; ++it) {
      if constexpr (GN) {
        const eltx8 gz8 = __builtin_bit_cast(eltx8, rdy[it]), yv8 = __builtin_bit_cast(eltx8, ryy[it]);
        float gg[8], u[8], yy[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          yy[k] = (float)yv8[k];
          gg[k] = (float)gz8[k];
          u[k] = fmaf(gca[k], yy[k], gcb[k]);
        }
        act_grad_pre_n<8>(gg, u, a.act);
        eltx8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = (elt)fmaf(gk1[k], gg[k], fmaf(gk2[k], yy[k], gk3[k]));
        const u32x4 zero = {0u, 0u, 0u, 0u};
        *reinterpret_cast<u32x4*>(dyl + (it * 256 + tid) * 16) = (in_mask >> it) & 1u ? __builtin_bit_cast(u32x4, o) : zero;
      } else {
        *reinterpret_cast<u32x4*>(dyl + (it * 256 + tid) * 16) = rdy[it];
      }
    }
#pragma unroll
    for (int it = 0; it < X_ROUNDS; ++it) {
      const int v = it * 256 + tid;
      if (v < NH) {
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) xh[ci * XH_F + v] = rx[ci][it];
      }
    }
  };

  f32x16 acc[CIN][NB];
#pragma unroll
  for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[ci][b][j] = 0.f;

  int tile = blockIdx.x;
  if (tile < a.ntiles) fetch(tile);
  for (; tile < a.ntiles; tile += gridDim.x) {
    __syncthreads();  // previous brick fully consumed
    commit();
    __syncthreads();
    if (tile + (int)gridDim.x < a.ntiles) fetch(tile + gridDim.x);  // flies while this brick is worked on
#pragma unroll
    for (int s8 = 0; s8 < 8; ++s8) {
      const int row = wv * 8 + s8;  // (lz, ly) = (row / TY, row % TY): 16 x-consecutive voxels = one MFMA k-step
      const char* brow = dyl + (row * TX + 8 * hk + q) * ROWB + coloff;
      eltx8 fb[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) fb[b] = tr_operand(brow + b * 64, 4 * ROWB);
#pragma unroll
      for (int ci = 0; ci < CIN; ++ci) {
        const float* px = xh + ci * XH_F + abase + ((row / TY) * HY + row % TY) * HX;
        eltx8 hi, lo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float xv = px[j];
          hi[j] = (elt)xv;
          lo[j] = (elt)(xv - (float)hi[j]);
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          acc[ci][b] = MEDNET_MFMA_32x32x16(hi, fb[b], acc[ci][b], 0, 0, 0);
          acc[ci][b] = MEDNET_MFMA_32x32x16(lo, fb[b], acc[ci][b], 0, 0, 0);
        }
      }
    }
  }
  // ---- per channel: sum the 4 waves in LDS (fixed order), write the workgroup's partial in dW layout [co][ci][27]
  float* red = reinterpret_cast<float*>(smem);  // [4 waves][NB][16][64 lanes]
#pragma unroll
  for (int ci = 0; ci < CIN; ++ci) {
    __syncthreads();
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int j = 0; j < 16; ++j) red[((wv * NB + b) * 16 + j) * 64 + lane] = acc[ci][b][j];
    __syncthreads();
    if (wv == 0) {
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const float s = (red[((0 * NB + b) * 16 + j) * 64 + lane] + red[((1 * NB + b) * 16 + j) * 64 + lane]) +
                          (red[((2 * NB + b) * 16 + j) * 64 + lane] + red[((3 * NB + b) * 16 + j) * 64 + lane]);
          const int tap = (j & 3) + 8 * (j >> 2) + 4 * hk, co = b * 32 + (lane & 31);
          if (tap < 27 && co < a.cout) a.part[(((size_t)blockIdx.x * a.cout + co) * CIN + ci) * 27 + tap] = s;
        }
    }
  }
}

// One channel: Cout in {16, 32, 64}, x fp32 or in the storage type.  2 to 4: Cout a multiple of 16 up to 64, fp32 x.
bool wgrad_first_mfma_supported(int cin, int cout, int x_dtype, int dy_dtype) {
  if (dy_dtype != ELT_DTYPE) return false;
  if (cin == 1) return (cout == 16 || cout == 32 || cout == 64) && (x_dtype == MEDNET_F32 || x_dtype == ELT_DTYPE);
  return cin >= 2 && cin <= 4 && cout % 16 == 0 && cout <= 64 && x_dtype == MEDNET_F32;
}
// out4 = {workgroups, NB (32-channel blocks per workgroup), workgroups per CU the kernel is built for, dynamic LDS bytes}
void wgrad_first_mfma_plan(int n, int d, int h, int w, int cin, int cout, bool gn, int* out4) {
  const int nt = n * ((d + 3) / 4) * ((h + 7) / 8) * ((w + 15) / 16);
  const int nb = (cout + 31) / 32;
  const int per_cu = wfirst_waves(cin, nb, gn);
  const int cap = 512 * per_cu;  // two rounds of resident workgroups on 256 CUs
  const size_t stage = (size_t)cin * 4352 + (size_t)512 * 64 * nb, red = (size_t)4 * nb * 16 * 64 * 4;
  out4[0] = nt < cap ? nt : cap;
  out4[1] = nb;
  out4[2] = per_cu;
  out4[3] = (int)(stage > red ? stage : red);
}
int wgrad_first_mfma_blocks(int n, int d, int h, int w, int cin, int cout, bool gn) {
  int p[4];
  wgrad_first_mfma_plan(n, d, h, w, cin, cout, gn, p);
  return p[0];
}
int launch_wgrad_first_mfma(const void* x, int x_layout, int x_dtype, const void* dy, float* part, int n, int d, int h, int w, int cin,
                            int cout, hipStream_t s, const void* gn_y, const float* gn_coef, const float* gn_bcoef, int gn_act) {
  const char* who = cin == 1 ? "wgrad_c1_mfma" : "wgrad_cm_mfma";
  WfirstArgs a;
  const bool gn = gn_y != nullptr;  // dy is dz: GroupNorm's backward applied while staging (WfirstArgs)
  MEDNET_REQUIRE(cin >= 1 && cin <= 4 && cout % 16 == 0 && cout <= 64 && (cin == 1 || x_dtype == MEDNET_F32), MEDNET_E_UNSUPPORTED,
                 "%s: cin=%d cout=%d", who, cin, cout);
  MEDNET_REQUIRE(!gn || (gn_coef && gn_bcoef), MEDNET_E_SHAPE, "%s: the GroupNorm form needs both coefficient tables", who);
  a.y = (const elt*)gn_y; a.coef = gn_coef; a.bcoef = gn_bcoef; a.act = gn_act;
  a.x = x;
  a.x16 = x_dtype != MEDNET_F32;
  a.dy = (const elt*)dy;
  a.part = part;
  a.n = n; a.d = d; a.h = h; a.w = w; a.cout = cout;
  a.tiles_z = (d + 3) / 4; a.tiles_y = (h + 7) / 8; a.tiles_x = (w + 15) / 16;
  a.ntiles = n * a.tiles_z * a.tiles_y * a.tiles_x;
  a.rcp_tiles_x = fastdiv_rcp(a.tiles_x); a.rcp_tiles_y = fastdiv_rcp(a.tiles_y); a.rcp_tiles_z = fastdiv_rcp(a.tiles_z);
  MEDNET_REQUIRE((double)d * h * w * cout * 2.0 < 4294960000.0 && (double)d * h * w * cin * 4.0 < 4294960000.0, MEDNET_E_UNSUPPORTED,
                 "%s: one sample must stay below 4 GB", who);
  const size_t vol = (size_t)d * h * w;
  const unsigned esz = a.x16 ? 2u : 4u;
  a.bytes_x = (unsigned)(vol * cin * esz);
  a.bytes_dy = (unsigned)(vol * cout * 2);
  a.sv4 = x_layout == MEDNET_NCDHW ? esz : esz * (unsigned)cin;
  a.sc4 = x_layout == MEDNET_NCDHW ? (unsigned)(vol * esz) : esz;
  int plan[4];
  wgrad_first_mfma_plan(n, d, h, w, cin, cout, gn, plan);
  const int blocks = plan[0], nb = plan[1];
  const size_t lds = (size_t)plan[3];
#define WFIRST_NB(CIN_)                                                                            \
  (nb == 1 ? (gn ? wgrad_first_mfma_kernel<CIN_, 1, true> : wgrad_first_mfma_kernel<CIN_, 1, false>) \
           : (gn ? wgrad_first_mfma_kernel<CIN_, 2, true> : wgrad_first_mfma_kernel<CIN_, 2, false>))
  const auto kernel = cin == 1 ? WFIRST_NB(1) : cin == 2 ? WFIRST_NB(2) : cin == 3 ? WFIRST_NB(3) : WFIRST_NB(4);
#undef WFIRST_NB
  if (lds > 48 * 1024) return launch_lds(who, kernel, dim3(blocks), dim3(256), lds, s, a);  // (below that the default limit serves)
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), lds, s, a);
  return check_launch(who);
}
