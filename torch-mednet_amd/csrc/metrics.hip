// Case-level evaluation of a whole-volume prediction (additive to ABI 3): confusion counts, surface masks, the exact squared
// Euclidean distance transform and the surface statistics the Hausdorff / ASSD / surface-Dice figures are made of.
//   confusion      two launches: 32-bit counters per workgroup in LDS (integer LDS adds), one partial row per workgroup in the
//                  workspace, then one workgroup per entry sums it over the rows in int64
//   surface_mask   one launch for up to two volumes: out = (vol == cls) and a face neighbour differs or lies outside
//   edt_sq         three launches of ONE kernel, x then y then z, in place on the output: a workgroup stages a bundle of lines in LDS
//                  and takes, per output, the minimum over every candidate of the line (min-plus sweep)
//   surface_stats  two launches: {count, count within tolerance, max d2, sum sqrt(d2) in fp64} per workgroup, then one workgroup
// No float atomics, no loop without a bound given by an extent or a class count, nothing waits for another workgroup; every grid is a
// function of the extents alone and every sum has a fixed order, so the same inputs give the same bits.
#include <float.h>
#include "volume.h"

namespace mednet {

constexpr int METRIC_MAX_CLASSES = 32;

// ---------------------------------------------------------------------------------------------- confusion counts
// Entry l * ncls + p counts label l predicted as p, entry ncls^2 the voxels with label or prediction >= ncls.  A thread keeps the
// run of equal keys it is in and adds the run's length when the key changes: a volume that is mostly background costs few LDS adds.
__global__ __launch_bounds__(256) void confusion_partial_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ label,
                                                                size_t vox, size_t share, int ncls, int ignore,
                                                                unsigned* __restrict__ partial) {
  __shared__ unsigned cnt[METRIC_MAX_CLASSES * METRIC_MAX_CLASSES + 1];
  const int entries = ncls * ncls + 1;
  for (int e = threadIdx.x; e < entries; e += 256) cnt[e] = 0u;
  __syncthreads();
  size_t begin, end;
  row_range(vox, share, begin, end);
  int cur = -1;
  unsigned run = 0;
  for (size_t i = begin + threadIdx.x; i < end; i += 256) {
    const int l = label[i], p = pred[i];
    if (l == ignore) continue;
    const int key = (l < ncls && p < ncls) ? l * ncls + p : entries - 1;
    if (key != cur) {
      if (run) atomicAdd(&cnt[cur], run);
      cur = key;
      run = 0;
    }
    ++run;
  }
  if (run) atomicAdd(&cnt[cur], run);
  __syncthreads();
  unsigned* __restrict__ row = partial + (size_t)blockIdx.x * entries;
  for (int e = threadIdx.x; e < entries; e += 256) row[e] = cnt[e];
}

// one workgroup per entry: the rows in strides of 256, then the fixed-order tree (integers: any order gives the same sum)
__global__ __launch_bounds__(256) void confusion_finalize_kernel(const unsigned* __restrict__ partial, unsigned rows, int entries,
                                                                 int64_t* __restrict__ out) {
  __shared__ int64_t red[256];
  const int e = blockIdx.x;
  int64_t s = 0;
  for (unsigned r = threadIdx.x; r < rows; r += 256) s += (int64_t)partial[(size_t)r * entries + e];
  s = block_tree(s, red, [](int64_t a, int64_t b) { return a + b; });
  if (threadIdx.x == 0) out[e] = s;
}

// ---------------------------------------------------------------------------------------------- surface mask
// mask & ~binary_erosion(mask) with the 6-connected structuring element and background outside the volume
__device__ __forceinline__ uint8_t surface_voxel(const uint8_t* __restrict__ vol, size_t i, int z, int y, int x, int d, int h, int w,
                                                 int cls) {
  if (vol[i] != cls) return 0;
  const size_t sy = (size_t)w, sz = (size_t)h * w;
  bool inner = x > 0 && x < w - 1 && y > 0 && y < h - 1 && z > 0 && z < d - 1;
  if (inner)
    inner = vol[i - 1] == cls && vol[i + 1] == cls && vol[i - sy] == cls && vol[i + sy] == cls && vol[i - sz] == cls &&
            vol[i + sz] == cls;
  return inner ? 0 : 1;
}

__global__ __launch_bounds__(256) void surface_mask_kernel(const uint8_t* __restrict__ vol, uint8_t* __restrict__ out,
                                                           const uint8_t* __restrict__ vol2, uint8_t* __restrict__ out2, int cls,
                                                           int d, int h, int w) {
  const size_t vox = (size_t)d * h * w, stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < vox; i += stride) {
    const auto [z, y, x] = voxel_zyx(i, h, w);
    out[i] = surface_voxel(vol, i, z, y, x, d, h, w, cls);
    if (vol2) out2[i] = surface_voxel(vol2, i, z, y, x, d, h, w, cls);
  }
}

// ---------------------------------------------------------------------------------------------- squared distance transform
// One pass along one axis of extent n:  out[i] = min over j of  g[j] + T(i - j),   T(k) = (spacing * k)^2 rounded ONCE to fp32 (the
// product is formed in fp64 from the fp32 spacing, where spacing * k is exact).  The first pass reads the seeds as g = 0 / +inf.
// Every candidate of the line is evaluated -- no envelope, no early exit --, so the result is the minimum over all candidates of
// that one fp32 addition; with dyadic spacing every operand is exact and so is the result.
//
// A workgroup owns BX neighbouring lines (`line` = the index that is contiguous in memory for the y and z passes, a row for the x
// pass) over the whole extent: it loads them into LDS as g[j][BX + 1], every thread then keeps 8 CONSECUTIVE outputs of one line in
// registers and walks j eight at a time; the 64 candidates of such a step need 8 values of g and the 16 table values
// T(i0 - jb - 8 .. i0 - jb + 7), four 16-byte LDS reads of the two-sided table tab[m] = T(m - NP).  Lines are independent and a
// workgroup reads all of its lines before it writes any, so the y and z passes run in place.
constexpr int EDT_OUT = 8;                          // outputs per thread = candidates j per step
constexpr int EDT_NP_64 = 240, EDT_NP_32 = 464;     // largest padded extent with a bundle of 64 / 32 lines inside 64 KiB
static inline int edt_np(int n) { return (n + EDT_OUT - 1) / EDT_OUT * EDT_OUT; }
static inline int edt_bundle(int n) { return edt_np(n) <= EDT_NP_64 ? 64 : edt_np(n) <= EDT_NP_32 ? 32 : 16; }
// LDS of a workgroup: the two-sided table and the bundle.  Bundles of 16 lines reach 152 KiB of the CU's 160 at the largest extent.
constexpr size_t edt_lds_bytes(int np, int bx) { return ((size_t)2 * np + (size_t)np * (bx + 1)) * sizeof(float); }
template <int BX>
constexpr size_t edt_lds_cap() {
  return edt_lds_bytes(BX == 64 ? EDT_NP_64 : BX == 32 ? EDT_NP_32 : VOLUME_MAX_EXTENT, BX);
}

template <int BX, bool FIRST>
__global__ __launch_bounds__(256) void edt_pass_kernel(const void* in, float* out, int n, size_t nlines, size_t lstride,
                                                       size_t astride, size_t ostride, float spacing) {
  extern __shared__ __attribute__((aligned(16))) float edt_lds[];
  constexpr int BXP = BX + 1, NI = 256 / BX;
  const int np = (n + EDT_OUT - 1) / EDT_OUT * EDT_OUT;
  float* __restrict__ tab = edt_lds;           // 2 np entries: tab[m] = T(m - np), 0 beyond the extent (g is +inf there)
  float* __restrict__ g = edt_lds + 2 * np;    // np x BXP
  const float inf = __builtin_inff();
  const size_t base = (size_t)blockIdx.y * ostride, l0 = (size_t)blockIdx.x * BX;
  for (int m = threadIdx.x; m < 2 * np; m += 256) {
    const int k = m >= np ? m - np : np - m;
    const double sk = (double)spacing * (double)k;
    tab[m] = k < n ? (float)(sk * sk) : 0.f;
  }
  for (int e = threadIdx.x; e < np * BX; e += 256) {
    int j, l;
    if (FIRST) {  // x pass: memory runs along the axis
      j = e % np;
      l = e / np;
    } else {
      l = e % BX;
      j = e / BX;
    }
    float v = inf;
    if (j < n && l0 + l < nlines) {
      const size_t a = base + (l0 + l) * lstride + (size_t)j * astride;
      if (FIRST)
        v = static_cast<const uint8_t*>(in)[a] ? 0.f : inf;
      else
        v = static_cast<const float*>(in)[a];
    }
    g[j * BXP + l] = v;
  }
  __syncthreads();
  const int lx = threadIdx.x % BX, ig = threadIdx.x / BX;
  const bool live = l0 + lx < nlines;
  for (int i0 = ig * EDT_OUT; i0 < np; i0 += NI * EDT_OUT) {
    float best[EDT_OUT];
#pragma unroll
    for (int r = 0; r < EDT_OUT; ++r) best[r] = inf;
    for (int jb = 0; jb < np; jb += EDT_OUT) {
      // tw[t] = T(i0 - jb - 8 + t): the candidate (output i0 + r, source jb + jj) reads tw[8 + r - jj]
      const f32x4* __restrict__ tv = reinterpret_cast<const f32x4*>(tab + (i0 - jb - EDT_OUT + np));
      float tw[2 * EDT_OUT];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 t4 = tv[q];
#pragma unroll
        for (int k = 0; k < 4; ++k) tw[4 * q + k] = t4[k];
      }
#pragma unroll
      for (int jj = 0; jj < EDT_OUT; ++jj) {
        const float gj = g[(jb + jj) * BXP + lx];
#pragma unroll
        for (int r = 0; r < EDT_OUT; ++r) best[r] = fminf(best[r], gj + tw[EDT_OUT + r - jj]);
      }
    }
    if (live) {
#pragma unroll
      for (int r = 0; r < EDT_OUT; ++r)
        if (i0 + r < n) out[base + (l0 + lx) * lstride + (size_t)(i0 + r) * astride] = best[r];
    }
  }
}

// The dynamic-LDS limit of an instantiation is raised once, to the most any extent of its tier can ask for; a launch asks for what
// its own extent needs, so short lines leave room for more workgroups on a CU.
template <int BX, bool FIRST>
static int edt_launch(const char* what, dim3 grid, size_t lds, hipStream_t s, const void* in, float* out, int n, size_t nlines,
                      size_t lstride, size_t astride, size_t ostride, float spacing) {
  const auto kernel = edt_pass_kernel<BX, FIRST>;
  if (!lds_limit_raised((const void*)kernel, edt_lds_cap<BX>()))
    return fail(MEDNET_E_HIP, "edt_sq: cannot raise dynamic LDS to %zu", edt_lds_cap<BX>());
  hipLaunchKernelGGL(kernel, grid, dim3(256), lds, s, in, out, n, nlines, lstride, astride, ostride, spacing);
  return check_launch(what);
}

template <bool FIRST>
static int edt_pass(const char* what, const void* in, float* out, int n, size_t nlines, size_t lstride, size_t astride,
                    unsigned outer, size_t ostride, float spacing, hipStream_t s) {
  const int np = edt_np(n), bx = edt_bundle(n);
  const dim3 grid((unsigned)((nlines + bx - 1) / bx), outer);
  const size_t lds = edt_lds_bytes(np, bx);
  if (bx == 64) return edt_launch<64, FIRST>(what, grid, lds, s, in, out, n, nlines, lstride, astride, ostride, spacing);
  if (bx == 32) return edt_launch<32, FIRST>(what, grid, lds, s, in, out, n, nlines, lstride, astride, ostride, spacing);
  return edt_launch<16, FIRST>(what, grid, lds, s, in, out, n, nlines, lstride, astride, ostride, spacing);
}

// ---------------------------------------------------------------------------------------------- surface statistics
// Partial rows in the workspace, one array per field: int64 count[rows], int64 within[rows], double sum[rows], float max[rows].
struct StatsRows {
  int64_t* count;
  int64_t* within;
  double* sum;
  float* max;
};
static inline StatsRows stats_rows(void* ws, unsigned rows) {
  StatsRows r;
  r.count = static_cast<int64_t*>(ws);
  r.within = r.count + rows;
  r.sum = reinterpret_cast<double*>(r.within + rows);
  r.max = reinterpret_cast<float*>(r.sum + rows);
  return r;
}
constexpr size_t STATS_ROW_BYTES = 2 * sizeof(int64_t) + sizeof(double) + sizeof(float);

struct StatsShared {
  int64_t i[256];
  double d[256];
  float f[256];
};

__device__ __forceinline__ void stats_reduce_store(int64_t n, int64_t within, double sum, float mx, StatsShared& sh, int64_t* o_n,
                                                   int64_t* o_within, double* o_sum, float* o_max) {
  n = block_tree(n, sh.i, [](int64_t a, int64_t b) { return a + b; });
  within = block_tree(within, sh.i, [](int64_t a, int64_t b) { return a + b; });
  sum = block_tree(sum, sh.d, [](double a, double b) { return a + b; });
  mx = block_tree(mx, sh.f, [](float a, float b) { return fmaxf(a, b); });
  if (threadIdx.x == 0) {
    *o_n = n;
    *o_within = within;
    *o_sum = sum;
    *o_max = mx;
  }
}

__global__ __launch_bounds__(256) void surface_stats_partial_kernel(const uint8_t* __restrict__ surf, const float* __restrict__ d2,
                                                                    size_t vox, size_t share, float tol_sq, StatsRows rows) {
  __shared__ StatsShared sh;
  size_t begin, end;
  row_range(vox, share, begin, end);
  int64_t n = 0, within = 0;
  double sum = 0.0;
  float mx = -__builtin_inff();
  for (size_t i = begin + threadIdx.x; i < end; i += 256) {
    if (!surf[i]) continue;
    const float v = d2[i];
    ++n;
    within += v <= tol_sq ? 1 : 0;
    mx = fmaxf(mx, v);
    sum += (double)__fsqrt_rn(v);  // the correctly rounded fp32 root, added in fp64 from the first add on
  }
  stats_reduce_store(n, within, sum, mx, sh, rows.count + blockIdx.x, rows.within + blockIdx.x, rows.sum + blockIdx.x,
                     rows.max + blockIdx.x);
}

__global__ __launch_bounds__(256) void surface_stats_finalize_kernel(StatsRows rows, unsigned nrows, int64_t* __restrict__ counts,
                                                                     float* __restrict__ max_d2, double* __restrict__ sum_sqrt) {
  __shared__ StatsShared sh;
  int64_t n = 0, within = 0;
  double sum = 0.0;
  float mx = -__builtin_inff();
  for (unsigned r = threadIdx.x; r < nrows; r += 256) {
    n += rows.count[r];
    within += rows.within[r];
    sum += rows.sum[r];
    mx = fmaxf(mx, rows.max[r]);
  }
  stats_reduce_store(n, within, sum, mx, sh, counts, counts + 1, sum_sqrt, max_d2);
}

}  // namespace mednet

// =================================================================================================== C ABI
using namespace mednet;

extern "C" size_t mednet_confusion_ws_bytes(int d, int h, int w, int ncls) {
  if (!extents_ok(d, h, w) || ncls < 1 || ncls > METRIC_MAX_CLASSES) return 0;
  return (size_t)row_plan((size_t)d * h * w).rows * (size_t)(ncls * ncls + 1) * sizeof(unsigned);
}

extern "C" int mednet_confusion(const uint8_t* pred, const uint8_t* label, int d, int h, int w, int ncls, int ignore_index,
                                int64_t* counts, void* ws, size_t ws_bytes, mednet_stream stream) {
  MEDNET_REQUIRE(pred && label && counts && ws, MEDNET_E_SHAPE, "confusion: null pointer");
  VOLUME_REQUIRE_EXTENTS("confusion", d, h, w);
  MEDNET_REQUIRE(ncls >= 1, MEDNET_E_SHAPE, "confusion: ncls %d", ncls);
  MEDNET_REQUIRE(ncls <= METRIC_MAX_CLASSES, MEDNET_E_UNSUPPORTED, "confusion: ncls %d above %d", ncls, METRIC_MAX_CLASSES);
  const size_t need = mednet_confusion_ws_bytes(d, h, w, ncls);
  MEDNET_REQUIRE(ws_bytes >= need, MEDNET_E_WORKSPACE, "confusion: workspace %zu < %zu bytes", ws_bytes, need);
  MEDNET_REQUIRE(((uintptr_t)ws & 3) == 0 && ((uintptr_t)counts & 7) == 0, MEDNET_E_SHAPE,
                 "confusion: workspace not 4-byte or counts not 8-byte aligned");
  const size_t vox = (size_t)d * h * w;
  const auto [rows, share] = row_plan(vox);
  const int entries = ncls * ncls + 1;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(confusion_partial_kernel, dim3(rows), dim3(256), 0, s, pred, label, vox, share, ncls,
                     ignore_index, (unsigned*)ws);
  const int rc = check_launch("confusion(partials)");
  if (rc != MEDNET_OK) return rc;
  hipLaunchKernelGGL(confusion_finalize_kernel, dim3(entries), dim3(256), 0, s, (const unsigned*)ws, rows, entries, counts);
  return check_launch("confusion");
}

extern "C" int mednet_surface_mask(const uint8_t* vol, uint8_t* out, const uint8_t* vol2, uint8_t* out2, int cls, int d, int h,
                                   int w, mednet_stream stream) {
  MEDNET_REQUIRE(vol && out, MEDNET_E_SHAPE, "surface_mask: null pointer");
  MEDNET_REQUIRE((vol2 == nullptr) == (out2 == nullptr), MEDNET_E_SHAPE, "surface_mask: null pointer (second volume or its mask)");
  VOLUME_REQUIRE_EXTENTS("surface_mask", d, h, w);
  MEDNET_REQUIRE(cls >= 0 && cls <= 255, MEDNET_E_SHAPE, "surface_mask: class %d is no uint8 value", cls);
  const size_t vox = (size_t)d * h * w;
  const size_t blocks = grid_blocks(vox, 1024, 8 * VOLUME_MAX_ROWS);  // four voxels per thread until the grid is full
  hipLaunchKernelGGL(surface_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, vol, out, vol2, out2, cls, d, h,
                     w);
  return check_launch("surface_mask");
}

extern "C" int mednet_edt_sq(const uint8_t* seed, float* out, int d, int h, int w, float sz, float sy, float sx,
                             mednet_stream stream) {
  MEDNET_REQUIRE(seed && out, MEDNET_E_SHAPE, "edt_sq: null pointer");
  VOLUME_REQUIRE_EXTENTS("edt_sq", d, h, w);
  MEDNET_REQUIRE(sz > 0.f && sy > 0.f && sx > 0.f && sz <= FLT_MAX && sy <= FLT_MAX && sx <= FLT_MAX, MEDNET_E_SHAPE,
                 "edt_sq: spacing (%g, %g, %g) must be finite and positive", (double)sz, (double)sy, (double)sx);
  MEDNET_REQUIRE(((uintptr_t)out & 3) == 0, MEDNET_E_SHAPE, "edt_sq: output not 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const size_t W = (size_t)w, HW = (size_t)h * w;
  // x: the lines are the d * h rows; y: per z-plane, the lines are the w columns; z: the lines are the h * w voxels of a plane
  int rc = edt_pass<true>("edt_sq(x)", seed, out, w, (size_t)d * h, W, 1, 1, 0, sx, s);
  if (rc != MEDNET_OK) return rc;
  rc = edt_pass<false>("edt_sq(y)", out, out, h, W, 1, W, (unsigned)d, HW, sy, s);
  if (rc != MEDNET_OK) return rc;
  return edt_pass<false>("edt_sq(z)", out, out, d, HW, 1, HW, 1, 0, sz, s);
}

extern "C" size_t mednet_surface_stats_ws_bytes(int d, int h, int w) {
  if (!extents_ok(d, h, w)) return 0;
  return (size_t)row_plan((size_t)d * h * w).rows * STATS_ROW_BYTES;
}

extern "C" int mednet_surface_stats(const uint8_t* surf, const float* d2, int d, int h, int w, float tol_sq, int64_t* counts,
                                    float* max_d2, double* sum_sqrt, void* ws, size_t ws_bytes, mednet_stream stream) {
  MEDNET_REQUIRE(surf && d2 && counts && max_d2 && sum_sqrt && ws, MEDNET_E_SHAPE, "surface_stats: null pointer");
  VOLUME_REQUIRE_EXTENTS("surface_stats", d, h, w);
  MEDNET_REQUIRE(tol_sq >= 0.f, MEDNET_E_SHAPE, "surface_stats: squared tolerance %g is negative or NaN", (double)tol_sq);
  const size_t need = mednet_surface_stats_ws_bytes(d, h, w);
  MEDNET_REQUIRE(ws_bytes >= need, MEDNET_E_WORKSPACE, "surface_stats: workspace %zu < %zu bytes", ws_bytes, need);
  MEDNET_REQUIRE(((uintptr_t)ws & 7) == 0 && ((uintptr_t)counts & 7) == 0 && ((uintptr_t)sum_sqrt & 7) == 0 &&
                     ((uintptr_t)max_d2 & 3) == 0 && ((uintptr_t)d2 & 3) == 0,
                 MEDNET_E_SHAPE, "surface_stats: pointer not aligned to its element");
  const size_t vox = (size_t)d * h * w;
  const auto [rows, share] = row_plan(vox);
  const StatsRows r = stats_rows(ws, rows);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(surface_stats_partial_kernel, dim3(rows), dim3(256), 0, s, surf, d2, vox, share, tol_sq, r);
  const int rc = check_launch("surface_stats(partials)");
  if (rc != MEDNET_OK) return rc;
  hipLaunchKernelGGL(surface_stats_finalize_kernel, dim3(1), dim3(256), 0, s, r, rows, counts, max_d2, sum_sqrt);
  return check_launch("surface_stats");
}
