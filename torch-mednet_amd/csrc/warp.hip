// Spatial augmentation of training patches on the device: crop + affine (rotation, scale, mirror) + elastic displacement in ONE
// pass over a device-resident volume, straight into a slot / channel range of the batch tensors (the shape of mednet_crop_patches,
// predict.hip).  No oversize crop, no intermediate.  Images are interpolated trilinearly, heat maps trilinearly and rounded once,
// labels taken nearest-neighbour.
//
// THE ARITHMETIC, pinned (fp32 throughout; tests/warp_util.py restates it operation by operation).  Output voxel (z, y, x) of row i:
//   1. u_k = (float)idx_k - c_k, c_k = (p_k - 1) * 0.5f: integers minus half-integers, exact.
//   2. lattice (disp != NULL; gd x gh x gw control points per component, corners on the patch's corner voxels):
//        g_k  = fl((float)idx_k * r_k),  r_k = fl((float)(g_k_extent - 1) / (float)(p_k - 1))  (0 when p_k == 1), computed once on
//               the host as one fp32 division;
//        cell = min((int)floorf(g_k), extent - 2), weight q_k = g_k - (float)cell (exact; q may reach or pass 1 in the last cell);
//        D_j  = lerp over x, then y, then z of component j's eight control points, each lerp fmaf(q, b - a, a);
//        u_j  = fl(u_j + D_j), j = 0, 1, 2  (component 0 displaces z, 1 y, 2 x; patch voxels).
//   3. s_k = fmaf(A[k][0], u_0, fmaf(A[k][1], u_1, fmaf(A[k][2], u_2, t[k]))), A | t = the row's 12 floats, row-major 3 x 4.
//   4. index conversion: warp_index.h (clamp in float to [-2, n + 1], NaN outside, then floorf).
//      linear:  cell f = floorf(s), weight w = s - f; per channel the eight taps are lerped over x, then y, then z, each
//               fmaf(w, b - a, a): a weight of exactly 0 returns a bit for bit.  f16 taps are widened first.  u8 output: one
//               rintf (nearest-even) of the fp32 result; a convex combination of bytes needs no clamp.
//      nearest: index floorf(s + 0.5f) per axis.
//   5. border: MEDNET_BORDER_CONSTANT -- a tap outside the volume reads cval (scipy's 'grid-constant': the result is still
//      interpolated towards it); MEDNET_BORDER_EDGE -- tap indices are clamped (scipy's 'nearest').
//
// MAPPING.  One thread owns one output voxel for ALL channels of the call: the coordinate (steps 1-4, above all the 24 lattice
// taps) is computed once and only the 8 taps + 7 fmaf repeat per channel.  A workgroup of 256 threads covers a compact BX x BY x BZ
// brick of the patch, so its 8-tap footprint under any rotation stays within a few cache lines per plane; an x-row of 256 voxels
// rotates into a diagonal through the volume that touches a new line every few taps.  Brick variants (tuning option "warp_brick",
// an A/B knob only: results never depend on it): 0 = 8 x 8 x 4 (x, y, z), 1 = 16 x 4 x 4 (the default), 2 = 32 x 4 x 2, 3 = 256 x 1 x 1 (the
// row).  Measured at 128^3 patches in batches of 4 (profiles/spatial_augment.md): the three bricks lie within 2 % of each other, the row
// is 19 % slower; 16 x 4 x 4 had the lowest median and minimum and stores 64-byte segments.
// Ragged patch extents: threads past the patch return before any load or store.
#include "common.h"
#include "warp_index.h"

static_assert((int)MEDNET_WARP_CONSTANT == (int)MEDNET_BORDER_CONSTANT && (int)MEDNET_WARP_EDGE == (int)MEDNET_BORDER_EDGE,
              "warp_index.h and mednet_hip.h disagree about the border codes");

namespace mednet {

struct WarpGeom {
  int c, d, h, w;        // source volume
  int c_total, c_off;    // batch tensor
  int pd, ph, pw;        // patch
  int gd, gh, gw;        // lattice (0 without one)
  float rz, ry, rx;      // lattice coordinate per patch voxel
  int sx, sy;            // log2 of the brick's x and y extents (z gets the rest of the 256 threads)
  int nbx, nby;          // bricks along x and y
  float cval;
};

__device__ __forceinline__ float warp_lerp(float w, float a, float b) { return fmaf(w, b - a, a); }

// one component of the lattice at cell (cz, cy, cx) with weights (qz, qy, qx)
__device__ __forceinline__ float warp_lattice(const float* __restrict__ g, int gh, int gw, int cz, int cy, int cx, float qz, float qy,
                                              float qx) {
  const float* p = g + ((size_t)cz * gh + cy) * gw + cx;
  const size_t sy = gw, sz = (size_t)gh * gw;
  const float a00 = warp_lerp(qx, p[0], p[1]);
  const float a01 = warp_lerp(qx, p[sy], p[sy + 1]);
  const float a10 = warp_lerp(qx, p[sz], p[sz + 1]);
  const float a11 = warp_lerp(qx, p[sz + sy], p[sz + sy + 1]);
  return warp_lerp(qz, warp_lerp(qy, a00, a01), warp_lerp(qy, a10, a11));
}

__device__ __forceinline__ void warp_lattice_cell(int idx, float r, int extent, int* cell, float* q) {
  const float g = __fmul_rn((float)idx, r);  // (no contraction with the subtraction below)
  int c = (int)floorf(g);                    // 0 <= g <= about extent - 1: idx < p and r = (extent - 1) / (p - 1)
  c = c > extent - 2 ? extent - 2 : c;
  *cell = c;
  *q = g - (float)c;
}

template <typename TS, typename TD>
__device__ __forceinline__ TD warp_store_cast(float v) { return (TD)v; }
template <>
__device__ __forceinline__ uint8_t warp_store_cast<uint8_t, uint8_t>(float v) { return (uint8_t)(int)rintf(v); }

template <typename TS, typename TD, bool LINEAR>
__global__ __launch_bounds__(256) void warp_patches_kernel(const TS* __restrict__ src, const float* __restrict__ affine,
                                                           const float* __restrict__ disp, const int* __restrict__ slot,
                                                           TD* __restrict__ out, const WarpGeom g, const int border) {
  const int t = threadIdx.x;
  int bk = blockIdx.x;
  const int bx = bk % g.nbx;
  bk /= g.nbx;
  const int by = bk % g.nby, bz = bk / g.nby;
  const int x = (bx << g.sx) + (t & ((1 << g.sx) - 1));
  const int y = (by << g.sy) + ((t >> g.sx) & ((1 << g.sy) - 1));
  const int z = bz * (256 >> (g.sx + g.sy)) + (t >> (g.sx + g.sy));
  if (x >= g.pw || y >= g.ph || z >= g.pd) return;
  const int b = blockIdx.y;

  float u0 = (float)z - (float)(g.pd - 1) * 0.5f;
  float u1 = (float)y - (float)(g.ph - 1) * 0.5f;
  float u2 = (float)x - (float)(g.pw - 1) * 0.5f;
  if (disp != nullptr) {
    int cz, cy, cx;
    float qz, qy, qx;
    warp_lattice_cell(z, g.rz, g.gd, &cz, &qz);
    warp_lattice_cell(y, g.ry, g.gh, &cy, &qy);
    warp_lattice_cell(x, g.rx, g.gw, &cx, &qx);
    const size_t per = (size_t)g.gd * g.gh * g.gw;
    const float* lat = disp + (size_t)b * 3 * per;
    u0 = u0 + warp_lattice(lat, g.gh, g.gw, cz, cy, cx, qz, qy, qx);
    u1 = u1 + warp_lattice(lat + per, g.gh, g.gw, cz, cy, cx, qz, qy, qx);
    u2 = u2 + warp_lattice(lat + 2 * per, g.gh, g.gw, cz, cy, cx, qz, qy, qx);
  }
  const float* A = affine + (size_t)b * 12;
  const float s0 = fmaf(A[0], u0, fmaf(A[1], u1, fmaf(A[2], u2, A[3])));
  const float s1 = fmaf(A[4], u0, fmaf(A[5], u1, fmaf(A[6], u2, A[7])));
  const float s2 = fmaf(A[8], u0, fmaf(A[9], u1, fmaf(A[10], u2, A[11])));

  const size_t pvox = (size_t)g.pd * g.ph * g.pw;
  const size_t vvox = (size_t)g.d * g.h * g.w;
  TD* o = out + ((size_t)slot[b] * g.c_total + g.c_off) * pvox + ((size_t)z * g.ph + y) * g.pw + x;
  if (LINEAR) {
    const mednet_warp_cell kz = mednet_warp_linear_cell(s0, g.d, border);
    const mednet_warp_cell ky = mednet_warp_linear_cell(s1, g.h, border);
    const mednet_warp_cell kx = mednet_warp_linear_cell(s2, g.w, border);
    const size_t r00 = ((size_t)kz.i0 * g.h + ky.i0) * g.w, r01 = ((size_t)kz.i0 * g.h + ky.i1) * g.w;
    const size_t r10 = ((size_t)kz.i1 * g.h + ky.i0) * g.w, r11 = ((size_t)kz.i1 * g.h + ky.i1) * g.w;
    const bool i00 = kz.in0 && ky.in0, i01 = kz.in0 && ky.in1, i10 = kz.in1 && ky.in0, i11 = kz.in1 && ky.in1;
    for (int cc = 0; cc < g.c; ++cc) {
      const TS* p = src + (size_t)cc * vvox;
      // every index is inside the volume (clamped); a flag only selects cval
      const float v000 = i00 && kx.in0 ? (float)p[r00 + kx.i0] : g.cval, v001 = i00 && kx.in1 ? (float)p[r00 + kx.i1] : g.cval;
      const float v010 = i01 && kx.in0 ? (float)p[r01 + kx.i0] : g.cval, v011 = i01 && kx.in1 ? (float)p[r01 + kx.i1] : g.cval;
      const float v100 = i10 && kx.in0 ? (float)p[r10 + kx.i0] : g.cval, v101 = i10 && kx.in1 ? (float)p[r10 + kx.i1] : g.cval;
      const float v110 = i11 && kx.in0 ? (float)p[r11 + kx.i0] : g.cval, v111 = i11 && kx.in1 ? (float)p[r11 + kx.i1] : g.cval;
      const float a0 = warp_lerp(ky.w, warp_lerp(kx.w, v000, v001), warp_lerp(kx.w, v010, v011));
      const float a1 = warp_lerp(ky.w, warp_lerp(kx.w, v100, v101), warp_lerp(kx.w, v110, v111));
      o[(size_t)cc * pvox] = warp_store_cast<TS, TD>(warp_lerp(kz.w, a0, a1));
    }
  } else {
    int iz, iy, ix;
    const int nz = mednet_warp_nearest_index(s0, g.d, border, &iz);
    const int ny = mednet_warp_nearest_index(s1, g.h, border, &iy);
    const int nx = mednet_warp_nearest_index(s2, g.w, border, &ix);
    const bool inside = iz && iy && ix;
    const size_t at = ((size_t)nz * g.h + ny) * g.w + nx;
    for (int cc = 0; cc < g.c; ++cc) o[(size_t)cc * pvox] = inside ? (TD)src[(size_t)cc * vvox + at] : (TD)g.cval;
  }
}

}  // namespace mednet

using namespace mednet;

extern "C" int mednet_warp_patches(const void* src, int src_dtype, const float* affine, const float* disp, int gd, int gh, int gw,
                                   const int* slot, int count, void* out, int dst_dtype, int c, int d, int h, int w, int c_total,
                                   int c_off, int pd, int ph, int pw, int interp, int border, float cval, mednet_stream stream) {
  MEDNET_REQUIRE(src && affine && slot && out, MEDNET_E_SHAPE, "warp_patches: null pointer (src %p, affine %p, slot %p, out %p)", src,
                 (const void*)affine, (const void*)slot, out);
  MEDNET_REQUIRE(count > 0 && c > 0 && d > 0 && h > 0 && w > 0 && pd > 0 && ph > 0 && pw > 0, MEDNET_E_SHAPE,
                 "warp_patches: bad shape (count %d, patch %dx%dx%d, volume %dx%dx%dx%d)", count, pd, ph, pw, c, d, h, w);
  // (warp_index.h: n + 1 and every voxel index must be exact in fp32)
  MEDNET_REQUIRE(d <= MEDNET_WARP_MAX_EXTENT && h <= MEDNET_WARP_MAX_EXTENT && w <= MEDNET_WARP_MAX_EXTENT && pd <= MEDNET_WARP_MAX_EXTENT &&
                     ph <= MEDNET_WARP_MAX_EXTENT && pw <= MEDNET_WARP_MAX_EXTENT,
                 MEDNET_E_SHAPE, "warp_patches: bad shape: an extent above 2^24 - 2 (patch %dx%dx%d, volume %dx%dx%d)", pd, ph, pw, d, h, w);
  MEDNET_REQUIRE(c_off >= 0 && c_off + c <= c_total, MEDNET_E_SHAPE, "warp_patches: channels %d+%d of %d", c_off, c, c_total);
  // (upper limit: the lattice coordinate idx * r <= extent - 1 is converted to an int without a clamp of its own)
  MEDNET_REQUIRE(!disp || (gd >= 2 && gh >= 2 && gw >= 2 && gd <= MEDNET_WARP_MAX_EXTENT && gh <= MEDNET_WARP_MAX_EXTENT &&
                           gw <= MEDNET_WARP_MAX_EXTENT),
                 MEDNET_E_SHAPE, "warp_patches: lattice %dx%dx%d (every extent 2 .. 2^24 - 2)", gd, gh, gw);
  MEDNET_REQUIRE(interp == MEDNET_INTERP_LINEAR || interp == MEDNET_INTERP_NEAREST, MEDNET_E_UNSUPPORTED,
                 "warp_patches: interpolation %d (supported: linear, nearest)", interp);
  MEDNET_REQUIRE(border == MEDNET_BORDER_CONSTANT || border == MEDNET_BORDER_EDGE, MEDNET_E_UNSUPPORTED,
                 "warp_patches: border %d (supported: constant, edge)", border);
  const int pair = src_dtype == MEDNET_F16 && dst_dtype == MEDNET_F32   ? 0
                   : src_dtype == MEDNET_F32 && dst_dtype == MEDNET_F32 ? 1
                   : src_dtype == MEDNET_U8 && dst_dtype == MEDNET_U8   ? 2
                                                                        : -1;
  MEDNET_REQUIRE(pair >= 0, MEDNET_E_DTYPE, "warp_patches: %d -> %d (supported: f16->f32, f32->f32, u8->u8)", src_dtype, dst_dtype);
  // the byte pair converts cval as it converts a value of the source: it has to be one (NaN fails the comparison too)
  MEDNET_REQUIRE(pair != 2 || (cval >= 0.f && cval <= 255.f), MEDNET_E_UNSUPPORTED, "warp_patches: cval %g for a u8 output (0..255)",
                 (double)cval);
  MEDNET_REQUIRE(count <= 65535, MEDNET_E_SHAPE, "warp_patches: count %d (at most 65535 rows per call)", count);

  static const int BRICKS[4][2] = {{3, 3}, {4, 2}, {5, 2}, {8, 0}};  // log2 of the x and y extents
  int variant = tuning_option("warp_brick", 1);
  if (variant < 0 || variant > 3) variant = 1;
  WarpGeom g;
  g.c = c, g.d = d, g.h = h, g.w = w, g.c_total = c_total, g.c_off = c_off, g.pd = pd, g.ph = ph, g.pw = pw;
  g.gd = disp ? gd : 0, g.gh = disp ? gh : 0, g.gw = disp ? gw : 0;
  g.rz = disp && pd > 1 ? (float)(gd - 1) / (float)(pd - 1) : 0.f;
  g.ry = disp && ph > 1 ? (float)(gh - 1) / (float)(ph - 1) : 0.f;
  g.rx = disp && pw > 1 ? (float)(gw - 1) / (float)(pw - 1) : 0.f;
  g.sx = BRICKS[variant][0], g.sy = BRICKS[variant][1];
  const int bz = 256 >> (g.sx + g.sy);
  g.nbx = (pw + (1 << g.sx) - 1) >> g.sx;
  g.nby = (ph + (1 << g.sy) - 1) >> g.sy;
  g.cval = cval;
  const size_t bricks = (size_t)g.nbx * g.nby * ((pd + bz - 1) / bz);
  MEDNET_REQUIRE(bricks <= 0x7fffffffu, MEDNET_E_SHAPE, "warp_patches: patch %dx%dx%d is too large for one launch", pd, ph, pw);
  const dim3 grid((unsigned)bricks, (unsigned)count);
  hipStream_t s = (hipStream_t)stream;
#define WP_GO(TS_, TD_, LIN_) \
  hipLaunchKernelGGL((warp_patches_kernel<TS_, TD_, LIN_>), grid, dim3(256), 0, s, (const TS_*)src, affine, disp, slot, (TD_*)out, g, border)
  const bool lin = interp == MEDNET_INTERP_LINEAR;
  if (pair == 0) { if (lin) WP_GO(_Float16, float, true); else WP_GO(_Float16, float, false); }
  else if (pair == 1) { if (lin) WP_GO(float, float, true); else WP_GO(float, float, false); }
  else { if (lin) WP_GO(uint8_t, uint8_t, true); else WP_GO(uint8_t, uint8_t, false); }
#undef WP_GO
  return check_launch("warp_patches");
}
