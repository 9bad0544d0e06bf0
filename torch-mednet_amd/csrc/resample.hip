// Resampling of device-resident volumes between voxel grids: one separable, table-driven axis pass, and the fused way back --
// class scores at the network's grid in, the arg-max class at the native grid out, without a class volume at the output size.
//
// THE ARITHMETIC, pinned (fp32 throughout; tests/resample_util.py restates it operation by operation).  The host states an axis as
// a table (mednet_hip/resample.py: axis_table): output index i reads the source indices start[i] .. start[i] + count[i] - 1 with
// the weights weight[i * taps + k].  A chain over the row's values v[k] is
//     acc = w[0] * v[0];   acc = fmaf(w[k], v[k], acc)  for k = 1 .. count - 1,
// in exactly this order.  A voxel outside the row's count is never read into the chain (a NaN next to the support does not leak),
// f16 and u8 values are widened first.  Stores: f32 as is, f16 one round-to-nearest-even, u8 fminf(fmaxf(acc, 0), 255) and one
// rintf (nearest-even).  The fused kernel's score of (output voxel, class) is the tensor product of the three tables in the
// association of three passes x, then y, then z with fp32 between them: the x chain for every (z-tap, y-tap), the y chain over
// those, the z chain over those -- bit for bit what three axis passes (axis 2, 1, 0) into fp32 volumes give.
//
// SAFETY.  count is clamped to 1 .. taps and every index to the extent inside the kernels, so any table is safe for memory, as any
// coordinate is for the warp.
//
// MAPPING.  Both kernels are bandwidth / cache kernels: no matrix cores, no atomics, no LDS; every output voxel has one owning
// thread, so results are a pure function of the input.
//   axis pass:  the volume is outer x n_in x inner (axis 0: c | d | h w, axis 1: c d | h | w, axis 2: c d h | w | 1); a thread owns
//               one output element, or, for axes 0 / 1 with w % 4 == 0 and aligned bases, four consecutive x (one 16-byte load per
//               tap for f32) -- then a wave reads 1 KiB runs of x per tap.
//   fused:      a thread owns 4 consecutive x outputs of one (z, y) and writes them as one 32-bit store where the address allows
//               (scalar otherwise: the tail of a row, an odd ow).  Threads are numbered x-group fastest, then y, then z, and
//               workgroups in that order: a slab of outputs needs the two-to-few source planes per class of its z rows, which stay
//               in the XCD's 4 MiB L2 while the slab is walked.  The thread's x rows of the table are loaded once (start, count;
//               with at most 2 taps on every axis -- every up-sampling, the common way back -- the weights too, and the 8 taps
//               are unrolled) and y / z walk with them.  Where the taps of the four outputs lie within 4 consecutive source
//               voxels (always under up-sampling) a (z-tap, y-tap) row is ONE 4-wide load per class and the taps are picked
//               from registers: measured 0.60 against 1.18 ms with eight scalar loads per row (14 classes, 160 x 160 x 96 ->
//               320 x 320 x 192; tuning option "resample_span", an A/B knob only: results never depend on it).
#include "common.h"
#include "volume.h"

namespace mednet {

constexpr int RESAMPLE_MAX_TAPS = 64;
constexpr int RESAMPLE_MAX_CLASSES = 256;
constexpr size_t RESAMPLE_MAX_BLOCKS = (size_t)1 << 22;  // the axis pass walks a capped grid in grid strides

struct AxisTable {
  const int* start;
  const int* count;
  const float* weight;
  int taps;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// row i of a table: first source index inside [0, n) and the number of taps inside [1, taps]
__device__ __forceinline__ void table_row(const AxisTable& t, int i, int n, int& s, int& cnt) {
  s = clampi(t.start[i], 0, n - 1);
  cnt = clampi(t.count[i], 1, t.taps);
}

// ---------------------------------------------------------------------------------------------- stores
__device__ __forceinline__ void rs_store(float* p, float v) { *p = v; }
__device__ __forceinline__ void rs_store(f16* p, float v) { *p = (f16)v; }
__device__ __forceinline__ void rs_store(uint8_t* p, float v) { *p = (uint8_t)(int)rintf(fminf(fmaxf(v, 0.f), 255.f)); }

template <typename T>
struct Vec4 { T v[4]; } __attribute__((aligned(4 * sizeof(T))));

// ---------------------------------------------------------------------------------------------- the axis pass
// src outer x n_in x inner -> dst outer x n_out x inner; V = 1 or 4 consecutive elements of inner per thread
template <typename TS, typename TD, int V>
__global__ __launch_bounds__(256) void resample_axis_kernel(const TS* __restrict__ src, TD* __restrict__ dst, const size_t outer,
                                                            const int n_in, const int n_out, const size_t inner, const AxisTable t) {
  const size_t inner_v = inner / V;
  const size_t total = outer * (size_t)n_out * inner_v;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t row = e / inner_v;
    const size_t in = (e - row * inner_v) * V;
    const int o = (int)(row % (size_t)n_out);
    const size_t ou = row / (size_t)n_out;
    int s, cnt;
    table_row(t, o, n_in, s, cnt);
    const float* __restrict__ wt = t.weight + (size_t)o * t.taps;
    const TS* p = src + ou * (size_t)n_in * inner + in;
    float acc[V];
    {
      const Vec4<TS>* q = reinterpret_cast<const Vec4<TS>*>(p + (size_t)s * inner);
      const float w0 = wt[0];
      if (V == 4) {
        const Vec4<TS> a = *q;
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = __fmul_rn(w0, (float)a.v[j]);
      } else {
        acc[0] = __fmul_rn(w0, (float)p[(size_t)s * inner]);
      }
    }
    for (int k = 1; k < cnt; ++k) {
      const int i = min(s + k, n_in - 1);
      const float wk = wt[k];
      if (V == 4) {
        const Vec4<TS> a = *reinterpret_cast<const Vec4<TS>*>(p + (size_t)i * inner);
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = fmaf(wk, (float)a.v[j], acc[j]);
      } else {
        acc[0] = fmaf(wk, (float)p[(size_t)i * inner], acc[0]);
      }
    }
    TD* out = dst + (ou * (size_t)n_out + o) * inner + in;
    if (V == 4) {
      Vec4<TD> r;
#pragma unroll
      for (int j = 0; j < V; ++j) rs_store(&r.v[j], acc[j]);
      *reinterpret_cast<Vec4<TD>*>(out) = r;
    } else {
      rs_store(out, acc[0]);
    }
  }
}

// ---------------------------------------------------------------------------------------------- the fused way back
// The value read: the source form is this template parameter and nothing else.  Planes of scores, or one label volume whose
// class-c score is label == c ? 1 : 0 (a label >= ncls scores for nobody).
template <typename TS>
__device__ __forceinline__ float class_value(const TS* __restrict__ src, size_t plane, int c, size_t i) {
  return (float)src[(size_t)c * plane + i];
}
template <>
__device__ __forceinline__ float class_value<uint8_t>(const uint8_t* __restrict__ src, size_t, int c, size_t i) {
  return (int)src[i] == c ? 1.f : 0.f;
}

// four consecutive values of a row (i .. i + 3, all inside the volume) in one load of 4 x sizeof(TS) bytes at TS's own alignment
template <typename TS>
__device__ __forceinline__ void class_span(const TS* __restrict__ src, size_t plane, int c, size_t i, float* v) {
  struct Four { TS e[4]; } f;
  __builtin_memcpy(&f, src + (size_t)c * plane + i, sizeof(f));
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = (float)f.e[k];
}
template <>
__device__ __forceinline__ void class_span<uint8_t>(const uint8_t* __restrict__ src, size_t, int c, size_t i, float* v) {
  struct Four { uint8_t e[4]; } f;
  __builtin_memcpy(&f, src + i, sizeof(f));
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = (int)f.e[k] == c ? 1.f : 0.f;
}
// v[d], d in 0 .. 3, without indexing registers
__device__ __forceinline__ float pick4(const float* v, int d) { return d & 2 ? (d & 1 ? v[3] : v[2]) : (d & 1 ? v[1] : v[0]); }

struct ArgmaxGeom {
  int ncls, d, h, w, od, oh, ow;
  int gx;         // x groups of 4 per output row
  unsigned groups;  // od * oh * gx
};

// FAST: every axis has at most 2 taps -- the x weights live in registers and the 8 taps are written out
template <typename TS, bool FAST>
__global__ __launch_bounds__(256) void resample_argmax_kernel(const TS* __restrict__ src, uint8_t* __restrict__ out,
                                                              float* __restrict__ out_max, const ArgmaxGeom g, const AxisTable tz,
                                                              const AxisTable ty, const AxisTable tx, const bool span) {
  const unsigned grp = blockIdx.x * 256u + threadIdx.x;
  if (grp >= g.groups) return;
  const int xg = (int)(grp % (unsigned)g.gx);
  const unsigned rowi = grp / (unsigned)g.gx;
  const int oy = (int)(rowi % (unsigned)g.oh), oz = (int)(rowi / (unsigned)g.oh);
  const int x0 = xg * 4;
  const int nx = min(4, g.ow - x0);

  int sz, cz, sy, cy;
  table_row(tz, oz, g.d, sz, cz);
  table_row(ty, oy, g.h, sy, cy);
  const float* __restrict__ wz = tz.weight + (size_t)oz * tz.taps;
  const float* __restrict__ wy = ty.weight + (size_t)oy * ty.taps;
  int sx[4], cx[4];
  const float* wxp[4];
  float wx0[4], wx1[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ox = min(x0 + j, g.ow - 1);  // (a lane past the row repeats its last output and stores nothing)
    table_row(tx, ox, g.w, sx[j], cx[j]);
    wxp[j] = tx.weight + (size_t)ox * tx.taps;
    wx0[j] = wxp[j][0];
    wx1[j] = tx.taps > 1 ? wxp[j][1] : 0.f;
  }
  const size_t plane = (size_t)g.d * g.h * g.w;
  float best[4];
  int arg[4];

  // With at most 2 taps along x, up-sampling puts the x taps of the thread's four outputs into at most 4 consecutive source voxels:
  // then a (z-tap, y-tap) row is ONE 4-wide load per class instead of eight scalar ones, and the taps are picked from registers.
  const int bx = max(0, min(sx[0], g.w - 4));
  bool compact = span && tx.taps <= 2 && g.w >= 4;
  int da[4], db[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    da[j] = sx[j] - bx;
    db[j] = min(sx[j] + 1, g.w - 1) - bx;
    compact = compact && da[j] >= 0 && da[j] <= 3 && (cx[j] < 2 || db[j] <= 3);  // (a one-tap row's second index is never used)
  }

  if (FAST) {
    const int z1 = min(sz + 1, g.d - 1), y1 = min(sy + 1, g.h - 1);
    const size_t r00 = ((size_t)sz * g.h + sy) * g.w, r01 = ((size_t)sz * g.h + y1) * g.w;
    const size_t r10 = ((size_t)z1 * g.h + sy) * g.w, r11 = ((size_t)z1 * g.h + y1) * g.w;
    const float wz0 = wz[0], wz1 = tz.taps > 1 ? wz[1] : 0.f, wy0 = wy[0], wy1 = ty.taps > 1 ? wy[1] : 0.f;
    const bool z2 = cz > 1, y2 = cy > 1;
    // the eight taps of output j, x then y then z; a second tap outside a row's count has been read from a clamped (legal) address
    // and is dropped by the selects
    auto score = [&](int j, float p00, float q00, float p01, float q01, float p10, float q10, float p11, float q11) {
      const bool x2 = cx[j] > 1;
      float a00 = __fmul_rn(wx0[j], p00), a01 = __fmul_rn(wx0[j], p01), a10 = __fmul_rn(wx0[j], p10), a11 = __fmul_rn(wx0[j], p11);
      a00 = x2 ? fmaf(wx1[j], q00, a00) : a00;
      a01 = x2 ? fmaf(wx1[j], q01, a01) : a01;
      a10 = x2 ? fmaf(wx1[j], q10, a10) : a10;
      a11 = x2 ? fmaf(wx1[j], q11, a11) : a11;
      float b0 = __fmul_rn(wy0, a00), b1 = __fmul_rn(wy0, a10);
      b0 = y2 ? fmaf(wy1, a01, b0) : b0;
      b1 = y2 ? fmaf(wy1, a11, b1) : b1;
      const float s = __fmul_rn(wz0, b0);
      return z2 ? fmaf(wz1, b1, s) : s;
    };
    if (compact) {
      for (int c = 0; c < g.ncls; ++c) {
        float v00[4], v01[4], v10[4], v11[4];
        class_span<TS>(src, plane, c, r00 + bx, v00);
        class_span<TS>(src, plane, c, r01 + bx, v01);
        class_span<TS>(src, plane, c, r10 + bx, v10);
        class_span<TS>(src, plane, c, r11 + bx, v11);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float s = score(j, pick4(v00, da[j]), pick4(v00, db[j]), pick4(v01, da[j]), pick4(v01, db[j]), pick4(v10, da[j]),
                                pick4(v10, db[j]), pick4(v11, da[j]), pick4(v11, db[j]));
          if (c == 0 || s > best[j]) {
            best[j] = s;
            arg[j] = c;
          }
        }
      }
    } else {
      for (int c = 0; c < g.ncls; ++c) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int xa = sx[j], xb = min(sx[j] + 1, g.w - 1);
          const float s = score(j, class_value<TS>(src, plane, c, r00 + xa), class_value<TS>(src, plane, c, r00 + xb),
                                class_value<TS>(src, plane, c, r01 + xa), class_value<TS>(src, plane, c, r01 + xb),
                                class_value<TS>(src, plane, c, r10 + xa), class_value<TS>(src, plane, c, r10 + xb),
                                class_value<TS>(src, plane, c, r11 + xa), class_value<TS>(src, plane, c, r11 + xb));
          if (c == 0 || s > best[j]) {
            best[j] = s;
            arg[j] = c;
          }
        }
      }
    }
  } else if (compact) {  // the tap loop over z and y with the span loads along x (a shrinking z or y on the way back)
    for (int c = 0; c < g.ncls; ++c) {
      float s[4] = {0.f, 0.f, 0.f, 0.f};
      for (int kz = 0; kz < cz; ++kz) {
        const int zi = min(sz + kz, g.d - 1);
        float b[4] = {0.f, 0.f, 0.f, 0.f};
        for (int ky = 0; ky < cy; ++ky) {
          const int yi = min(sy + ky, g.h - 1);
          float v[4];
          class_span<TS>(src, plane, c, ((size_t)zi * g.h + yi) * g.w + bx, v);
          const float wyk = wy[ky];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float a = __fmul_rn(wx0[j], pick4(v, da[j]));
            a = cx[j] > 1 ? fmaf(wx1[j], pick4(v, db[j]), a) : a;
            b[j] = ky == 0 ? __fmul_rn(wyk, a) : fmaf(wyk, a, b[j]);
          }
        }
        const float wzk = wz[kz];
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = kz == 0 ? __fmul_rn(wzk, b[j]) : fmaf(wzk, b[j], s[j]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c == 0 || s[j] > best[j]) {
          best[j] = s[j];
          arg[j] = c;
        }
    }
  } else {
    for (int c = 0; c < g.ncls; ++c) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // (written out: sx, cx and wxp stay in registers)
        if (j >= nx) break;
        float s = 0.f;
        for (int kz = 0; kz < cz; ++kz) {
          const int zi = min(sz + kz, g.d - 1);
          float b = 0.f;
          for (int ky = 0; ky < cy; ++ky) {
            const int yi = min(sy + ky, g.h - 1);
            const size_t r = ((size_t)zi * g.h + yi) * g.w;
            float a = __fmul_rn(wxp[j][0], class_value<TS>(src, plane, c, r + sx[j]));
            for (int kx = 1; kx < cx[j]; ++kx)
              a = fmaf(wxp[j][kx], class_value<TS>(src, plane, c, r + min(sx[j] + kx, g.w - 1)), a);
            b = ky == 0 ? __fmul_rn(wy[0], a) : fmaf(wy[ky], a, b);
          }
          s = kz == 0 ? __fmul_rn(wz[0], b) : fmaf(wz[kz], b, s);
        }
        if (c == 0 || s > best[j]) {
          best[j] = s;
          arg[j] = c;
        }
      }
    }
  }

  const size_t at = ((size_t)oz * g.oh + oy) * g.ow + x0;
  uint8_t* o = out + at;
  if (nx == 4 && ((uintptr_t)o & 3) == 0) {
    *reinterpret_cast<uint32_t*>(o) = (uint32_t)arg[0] | (uint32_t)arg[1] << 8 | (uint32_t)arg[2] << 16 | (uint32_t)arg[3] << 24;
  } else {
    for (int j = 0; j < nx; ++j) o[j] = (uint8_t)arg[j];
  }
  if (out_max != nullptr)
    for (int j = 0; j < nx; ++j) out_max[at + j] = best[j];
}

static inline bool volume_32bit(int d, int h, int w) { return (int64_t)d * h * w < ((int64_t)1 << 31); }
static inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }
static inline bool float_dtype(int dt) { return dt == MEDNET_F32 || dt == MEDNET_F16; }

}  // namespace mednet

using namespace mednet;

#define RESAMPLE_REQUIRE_VOLUME(who, d, h, w)                                                                          \
  VOLUME_REQUIRE_EXTENTS(who, d, h, w);                                                                                \
  MEDNET_REQUIRE(volume_32bit(d, h, w), MEDNET_E_SHAPE, who ": %d x %d x %d voxels do not fit a 32-bit index (limit 2^31 - 1)", d, h, w)

extern "C" int mednet_resample_axis(const void* src, int src_dtype, void* dst, int dst_dtype, int c, int d, int h, int w, int axis,
                                    int n_out, const int* start, const int* count, const float* weight, int taps,
                                    mednet_stream stream) {
  MEDNET_REQUIRE(src && dst && start && count && weight, MEDNET_E_SHAPE, "resample_axis: null pointer");
  MEDNET_REQUIRE(axis >= 0 && axis <= 2, MEDNET_E_SHAPE, "resample_axis: axis %d (0, 1, 2)", axis);
  RESAMPLE_REQUIRE_VOLUME("resample_axis", d, h, w);
  const int od = axis == 0 ? n_out : d, oh = axis == 1 ? n_out : h, ow = axis == 2 ? n_out : w;
  RESAMPLE_REQUIRE_VOLUME("resample_axis", od, oh, ow);
  MEDNET_REQUIRE(c >= 1, MEDNET_E_SHAPE, "resample_axis: channels %d", c);
  MEDNET_REQUIRE(taps >= 1 && taps <= RESAMPLE_MAX_TAPS, MEDNET_E_SHAPE, "resample_axis: taps %d outside 1 .. %d", taps, RESAMPLE_MAX_TAPS);
  const bool s_ok = float_dtype(src_dtype) || src_dtype == MEDNET_U8, d_ok = float_dtype(dst_dtype) || dst_dtype == MEDNET_U8;
  MEDNET_REQUIRE(s_ok && d_ok, MEDNET_E_DTYPE, "resample_axis: dtype %d -> %d (supported: f32, f16, u8 on either side)", src_dtype, dst_dtype);
  MEDNET_REQUIRE(aligned4(start) && aligned4(count) && aligned4(weight), MEDNET_E_SHAPE, "resample_axis: tables not 4-byte aligned");

  const int n_in = axis == 0 ? d : axis == 1 ? h : w;
  // channel offsets are products of up to four extents: size_t throughout
  const size_t outer = axis == 0 ? (size_t)c : axis == 1 ? (size_t)c * d : (size_t)c * d * h;
  const size_t inner = axis == 0 ? (size_t)h * w : axis == 1 ? (size_t)w : 1;
  const size_t ssz = src_dtype == MEDNET_F32 ? 4 : src_dtype == MEDNET_F16 ? 2 : 1, dsz = dst_dtype == MEDNET_F32 ? 4 : dst_dtype == MEDNET_F16 ? 2 : 1;
  const bool vec = axis != 2 && w % 4 == 0 && ((uintptr_t)src & (4 * ssz - 1)) == 0 && ((uintptr_t)dst & (4 * dsz - 1)) == 0;
  const size_t total = outer * (size_t)n_out * (inner / (vec ? 4 : 1));
  const dim3 grid((unsigned)grid_blocks(total, 256, RESAMPLE_MAX_BLOCKS));
  const AxisTable t{start, count, weight, taps};
  hipStream_t s = (hipStream_t)stream;
#define RS_GO(TS_, TD_)                                                                                                             \
  do {                                                                                                                              \
    if (vec)                                                                                                                        \
      hipLaunchKernelGGL((resample_axis_kernel<TS_, TD_, 4>), grid, dim3(256), 0, s, (const TS_*)src, (TD_*)dst, outer, n_in, n_out, inner, t); \
    else                                                                                                                            \
      hipLaunchKernelGGL((resample_axis_kernel<TS_, TD_, 1>), grid, dim3(256), 0, s, (const TS_*)src, (TD_*)dst, outer, n_in, n_out, inner, t); \
  } while (0)
#define RS_DST(TS_)                                   \
  do {                                                \
    if (dst_dtype == MEDNET_F32) RS_GO(TS_, float);   \
    else if (dst_dtype == MEDNET_F16) RS_GO(TS_, f16); \
    else RS_GO(TS_, uint8_t);                         \
  } while (0)
  if (src_dtype == MEDNET_F32) RS_DST(float);
  else if (src_dtype == MEDNET_F16) RS_DST(f16);
  else RS_DST(uint8_t);
#undef RS_DST
#undef RS_GO
  return check_launch("resample_axis");
}

extern "C" int mednet_resample_argmax(const void* src, int src_dtype, int ncls, int d, int h, int w, uint8_t* out, float* out_max,
                                      int od, int oh, int ow, const int* start0, const int* count0, const float* weight0, int taps0,
                                      const int* start1, const int* count1, const float* weight1, int taps1, const int* start2,
                                      const int* count2, const float* weight2, int taps2, mednet_stream stream) {
  MEDNET_REQUIRE(src && out && start0 && count0 && weight0 && start1 && count1 && weight1 && start2 && count2 && weight2, MEDNET_E_SHAPE,
                 "resample_argmax: null pointer");
  RESAMPLE_REQUIRE_VOLUME("resample_argmax", d, h, w);
  RESAMPLE_REQUIRE_VOLUME("resample_argmax", od, oh, ow);
  MEDNET_REQUIRE(ncls >= 1 && ncls <= RESAMPLE_MAX_CLASSES, MEDNET_E_SHAPE, "resample_argmax: classes %d outside 1 .. %d", ncls,
                 RESAMPLE_MAX_CLASSES);
  MEDNET_REQUIRE(taps0 >= 1 && taps0 <= RESAMPLE_MAX_TAPS && taps1 >= 1 && taps1 <= RESAMPLE_MAX_TAPS && taps2 >= 1 && taps2 <= RESAMPLE_MAX_TAPS,
                 MEDNET_E_SHAPE, "resample_argmax: taps %d, %d, %d outside 1 .. %d", taps0, taps1, taps2, RESAMPLE_MAX_TAPS);
  MEDNET_REQUIRE(float_dtype(src_dtype) || src_dtype == MEDNET_U8, MEDNET_E_DTYPE,
                 "resample_argmax: dtype %d (supported: f32 / f16 score planes, u8 labels)", src_dtype);
  MEDNET_REQUIRE(aligned4(start0) && aligned4(count0) && aligned4(weight0) && aligned4(start1) && aligned4(count1) && aligned4(weight1) &&
                     aligned4(start2) && aligned4(count2) && aligned4(weight2) && aligned4(out_max),
                 MEDNET_E_SHAPE, "resample_argmax: tables or out_max not 4-byte aligned");

  ArgmaxGeom g;
  g.ncls = ncls, g.d = d, g.h = h, g.w = w, g.od = od, g.oh = oh, g.ow = ow;
  g.gx = (ow + 3) / 4;
  g.groups = (unsigned)((size_t)od * oh * g.gx);  // (< 2^31: od * oh * ow is)
  const AxisTable tz{start0, count0, weight0, taps0}, ty{start1, count1, weight1, taps1}, tx{start2, count2, weight2, taps2};
  const dim3 grid((unsigned)grid_blocks(g.groups, 256));
  const bool fast = taps0 <= 2 && taps1 <= 2 && taps2 <= 2;
  const bool span = tuning_option("resample_span", 1) != 0;  // an A/B knob only: results never depend on it
  hipStream_t s = (hipStream_t)stream;
#define RA_GO(TS_)                                                                                                               \
  do {                                                                                                                           \
    if (fast)                                                                                                                    \
      hipLaunchKernelGGL((resample_argmax_kernel<TS_, true>), grid, dim3(256), 0, s, (const TS_*)src, out, out_max, g, tz, ty, tx, span); \
    else                                                                                                                         \
      hipLaunchKernelGGL((resample_argmax_kernel<TS_, false>), grid, dim3(256), 0, s, (const TS_*)src, out, out_max, g, tz, ty, tx, span); \
  } while (0)
  if (src_dtype == MEDNET_F32) RA_GO(float);
  else if (src_dtype == MEDNET_F16) RA_GO(f16);
  else RA_GO(uint8_t);
#undef RA_GO
  return check_launch("resample_argmax");
}
