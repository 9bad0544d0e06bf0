// Image degradation of a training batch on the device: Gaussian noise from a counter-based generator, and one extent-preserving,
// table-driven axis pass per (sample, channel) row that Gaussian blur and simulated low resolution are made of.  Both entries work
// on rows x spatial dense fp32, rows = B * C of the batch tensor (include/mednet_hip.h states the contracts).
//
// THE ARITHMETIC, pinned (tests/degrade_util.py restates it operation by operation).
//   noise:   voxel v of row r: block j = v >> 2, lane v & 3; (r0, r1, r2, r3) = philox4x32-10(counter (j, r, 0, 0), key (seed low,
//            seed high)); lanes 0 / 1 are the even / odd normal of the pair (r0, r1), lanes 2 / 3 of (r2, r3).  A pair (a, b):
//            u1 = ((a >> 8) + 1) * 2^-24 in (0, 1], u2 = (b >> 8) * 2^-24, rad = sqrtf(-2 * logf(u1)), z_even = rad * cospif(2 u2),
//            z_odd = rad * sinpif(2 u2); out = fmaf(std[r], z, x).  A pure function of (seed, r, v): the grid, the other rows and the
//            batch size do not enter.  A row with std[r] == 0 is neither read nor written.
//   filter:  output i of a row with table t: acc = weight[(t n + i) taps] * v[index[(t n + i) taps]], then
//            acc = fmaf(weight[.. + k], v[index[.. + k]], acc) for k = 1 .. count[t n + i] - 1, in exactly this order, fp32
//            throughout: the chain of resample.hip with an explicit index per tap.  Slots at and above count are never read; a row
//            without a table is copied bit for bit.
//
// SAFETY.  count is clamped to 1 .. taps, every index to 0 .. n - 1 and a row_table entry outside its range counts as -1
// (degrade_index.h, swept on the host): any table is safe for memory.
//
// MAPPING.  Bandwidth kernels: no matrix cores, no atomics, one owning thread per output element.
//   noise:      a thread owns one block of four voxels: one 16-byte load and store where the block's address allows, scalar
//               accesses otherwise (an unaligned row base, the tail of a row when spatial % 4 != 0).
//   axes 0, 1:  a workgroup stays within one row and one output index i, so its table entries are wave-uniform and come through
//               scalar loads; its 256 threads walk the (outer, x) elements of that index, four consecutive x each (one 16-byte
//               load per tap) when w % 4 == 0 and the bases are aligned, one x otherwise.  Workgroups are numbered i fastest: the
//               workgroups in flight share all but one of their source planes / lines.
//   axis 2:     taps are arbitrary indices into a contiguous line, so the lines are staged in LDS (2048 floats, 8 KiB): a tile is
//               G * nl consecutive (z, y) lines of a row, one flat 16-byte copy in; a thread owns column i of nl <= 8 lines and
//               reads a tap's index and weight ONCE for all of them (per-thread vector loads: i differs between lanes).
//               G = 256 / (threads per line) line groups share the workgroup when w < 256.
//   identity:   rows without a table take a straight copy of the same elements in the same kernels, 16 bytes per thread where the
//               addresses allow.
#include "common.h"
#include "volume.h"
#include "degrade_index.h"

namespace mednet {

constexpr int DEGRADE_MAX_TAPS = 64;
constexpr size_t DEGRADE_MAX_BLOCKS = (size_t)1 << 22;  // capped grids are walked in grid strides
constexpr int DEGRADE_TILE = 2048;                      // floats of LDS per workgroup of the axis-2 pass (= VOLUME_MAX_EXTENT)
constexpr int DEGRADE_LINES = 8;                        // lines per thread of the axis-2 pass, at most

// ---------------------------------------------------------------------------------------------- noise
struct Philox4 { uint32_t v[4]; };

// philox4x32-10 from its definition (Salmon et al., SC 2011): ten rounds, the key bumped between them
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0, c1 = lo1, c2 = n2, c3 = lo0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  return {{c0, c1, c2, c3}};
}

// two normals from two words (Box-Muller); every conversion and product is exact except logf, sqrtf, the two trigonometric
// functions and the two final products
__device__ __forceinline__ void normal_pair(uint32_t a, uint32_t b, float& z_even, float& z_odd) {
  const float u1 = (float)((a >> 8) + 1u) * 0x1p-24f;  // (0, 1]: the logarithm is finite
  const float u2 = (float)(b >> 8) * 0x1p-24f;
  const float rad = sqrtf(__fmul_rn(-2.0f, logf(u1)));
  const float t = __fmul_rn(2.0f, u2);
  z_even = __fmul_rn(rad, cospif(t));
  z_odd = __fmul_rn(rad, sinpif(t));
}

__global__ __launch_bounds__(256) void noise_patches_kernel(float* __restrict__ data, const float* __restrict__ stdev, const uint32_t k0,
                                                            const uint32_t k1, const int rows, const size_t spatial) {
  const size_t nblk = (spatial + 3) / 4;  // (< 2^30 + 1: spatial < 2^32)
  const size_t total = (size_t)rows * nblk;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t r = e / nblk;
    const size_t j = e - r * nblk;
    const float s = stdev[r];
    if (s == 0.0f) continue;  // the row is neither read nor written
    const Philox4 p = philox4x32_10((uint32_t)j, (uint32_t)r, 0u, 0u, k0, k1);
    float z[4];
    normal_pair(p.v[0], p.v[1], z[0], z[1]);
    normal_pair(p.v[2], p.v[3], z[2], z[3]);
    float* q = data + r * spatial + 4 * j;
    const size_t left = spatial - 4 * j;  // >= 1
    if (left >= 4 && ((uintptr_t)q & 15) == 0) {
      f32x4 x = *reinterpret_cast<const f32x4*>(q);
#pragma unroll
      for (int k = 0; k < 4; ++k) x[k] = fmaf(s, z[k], x[k]);
      *reinterpret_cast<f32x4*>(q) = x;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if ((size_t)k < left) q[k] = fmaf(s, z[k], q[k]);
    }
  }
}

// ---------------------------------------------------------------------------------------------- the axis pass over rows
struct RowTables {
  const int* row_table;  // [rows]
  int n_tables;
  const int* count;      // [n_tables][n]
  const int* index;      // [n_tables][n][taps]
  const float* weight;   // [n_tables][n][taps]
  int taps;
};

// Axes 0 and 1.  A row is outer x n x inner (axis 0: 1 | d | h w; axis 1: d | h | w); workgroup blk = (row, chunk, i), i fastest,
// owns 256 * V consecutive elements of the (outer, inner) elements of output index i.
template <int V>
__global__ __launch_bounds__(256) void filter_rows_plane_kernel(const float* __restrict__ src, float* __restrict__ dst, const size_t vol,
                                                                const size_t outer, const int n, const size_t inner, const size_t chunks,
                                                                const size_t nblocks, const RowTables t) {
  const size_t inner_v = inner / V;
  const size_t items = outer * inner_v;
  for (size_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const int i = (int)(blk % (size_t)n);
    const size_t rest = blk / (size_t)n;
    const size_t chunk = rest % chunks, row = rest / chunks;
    const size_t e = chunk * 256 + threadIdx.x;
    if (e >= items) continue;
    const size_t oa = e / inner_v;
    const size_t x = (e - oa * inner_v) * V;
    const float* p = src + row * vol + oa * (size_t)n * inner + x;
    float* out = dst + row * vol + (oa * (size_t)n + (size_t)i) * inner + x;
    const int tb = mednet_degrade_table(t.row_table[row], t.n_tables);
    if (tb < 0) {  // the identity: bits are moved, nothing is computed
      if (V == 4) *reinterpret_cast<f32x4*>(out) = *reinterpret_cast<const f32x4*>(p + (size_t)i * inner);
      else *out = p[(size_t)i * inner];
      continue;
    }
    const size_t at = (size_t)tb * n + i;
    const int cnt = mednet_degrade_count(t.count[at], t.taps);
    const int* __restrict__ ix = t.index + at * t.taps;
    const float* __restrict__ wt = t.weight + at * t.taps;
    float acc[V];
    {
      const size_t s = (size_t)mednet_degrade_index(ix[0], n);
      const float w0 = wt[0];
      if (V == 4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p + s * inner);
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = __fmul_rn(w0, a[j]);
      } else {
        acc[0] = __fmul_rn(w0, p[s * inner]);
      }
    }
    for (int k = 1; k < cnt; ++k) {
      const size_t s = (size_t)mednet_degrade_index(ix[k], n);
      const float wk = wt[k];
      if (V == 4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p + s * inner);
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = fmaf(wk, a[j], acc[j]);
      } else {
        acc[0] = fmaf(wk, p[s * inner], acc[0]);
      }
    }
    if (V == 4) {
      f32x4 r;
#pragma unroll
      for (int j = 0; j < V; ++j) r[j] = acc[j];
      *reinterpret_cast<f32x4*>(out) = r;
    } else {
      *out = acc[0];
    }
  }
}

// `count` floats from s to o by the whole workgroup: 16 bytes per thread where both addresses allow, the tail and everything else
// scalar.  o may be LDS.
__device__ __forceinline__ void block_copy(const float* __restrict__ s, float* __restrict__ o, const int count) {
  int done = 0;
  if ((((uintptr_t)s | (uintptr_t)o) & 15) == 0) {
    const int n4 = count / 4;
    for (int q = threadIdx.x; q < n4; q += 256) reinterpret_cast<f32x4*>(o)[q] = reinterpret_cast<const f32x4*>(s)[q];
    done = n4 * 4;
  }
  for (int q = done + threadIdx.x; q < count; q += 256) o[q] = s[q];
}

// Axis 2.  A row is nlines = d * h lines of w; workgroup blk = (row, tile) owns the G * nl lines from line tile * G * nl, G =
// 256 / cpl line groups of cpl threads (cpl: a power of two >= min(w, 256)), G * nl * w <= DEGRADE_TILE.
__global__ __launch_bounds__(256) void filter_rows_line_kernel(const float* __restrict__ src, float* __restrict__ dst, const size_t vol,
                                                               const size_t nlines, const int w, const int cpl, const int nl,
                                                               const size_t tiles, const size_t nblocks, const RowTables t) {
  __shared__ __attribute__((aligned(16))) float tile[DEGRADE_TILE];
  const int per_tile = (256 / cpl) * nl;
  const int g = threadIdx.x / cpl, c = threadIdx.x - g * cpl;
  for (size_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const size_t tl = blk % tiles, row = blk / tiles;
    const size_t line0 = tl * (size_t)per_tile;
    const int lines = (int)(nlines - line0 < (size_t)per_tile ? nlines - line0 : (size_t)per_tile);  // >= 1
    const int count = lines * w;                                                                       // <= DEGRADE_TILE
    const float* s = src + row * vol + line0 * (size_t)w;
    float* o = dst + row * vol + line0 * (size_t)w;
    const int tb = mednet_degrade_table(t.row_table[row], t.n_tables);
    if (tb < 0) {  // (wave-uniform: no thread of the workgroup reaches the barriers below)
      block_copy(s, o, count);
      continue;
    }
    block_copy(s, tile, count);
    __syncthreads();
    for (int i = c; i < w; i += cpl) {
      const size_t at = (size_t)tb * w + i;
      const int cnt = mednet_degrade_count(t.count[at], t.taps);
      const int* __restrict__ ix = t.index + at * t.taps;
      const float* __restrict__ wt = t.weight + at * t.taps;
      int at_line[DEGRADE_LINES];  // LDS offsets of the thread's lines; a line past the tile repeats the last one and is not stored
#pragma unroll
      for (int l = 0; l < DEGRADE_LINES; ++l) at_line[l] = min(g * nl + min(l, nl - 1), lines - 1) * w;
      float acc[DEGRADE_LINES];
      {
        const int s0 = mednet_degrade_index(ix[0], w);
        const float w0 = wt[0];
#pragma unroll
        for (int l = 0; l < DEGRADE_LINES; ++l) acc[l] = __fmul_rn(w0, tile[at_line[l] + s0]);
      }
      for (int k = 1; k < cnt; ++k) {
        const int sk = mednet_degrade_index(ix[k], w);
        const float wk = wt[k];
#pragma unroll
        for (int l = 0; l < DEGRADE_LINES; ++l) acc[l] = fmaf(wk, tile[at_line[l] + sk], acc[l]);
      }
#pragma unroll
      for (int l = 0; l < DEGRADE_LINES; ++l) {
        const int line = g * nl + l;
        if (l < nl && line < lines) o[(size_t)line * w + i] = acc[l];
      }
    }
    __syncthreads();  // the tile is free for the next staging
  }
}

static inline bool degrade_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace mednet

using namespace mednet;

extern "C" int mednet_noise_patches(float* data, const float* stdev, uint64_t seed, int rows, size_t spatial, mednet_stream stream) {
  MEDNET_REQUIRE(data && stdev, MEDNET_E_SHAPE, "noise_patches: null pointer");
  MEDNET_REQUIRE(rows >= 1, MEDNET_E_SHAPE, "noise_patches: rows %d", rows);
  MEDNET_REQUIRE(spatial >= 1, MEDNET_E_SHAPE, "noise_patches: spatial %zu", spatial);
  MEDNET_REQUIRE((uint64_t)spatial < ((uint64_t)1 << 32), MEDNET_E_SHAPE,
                 "noise_patches: %zu voxels per row do not fit a 32-bit index (limit 2^32 - 1): the counter's word 0 would wrap", spatial);
  MEDNET_REQUIRE(degrade_aligned(stdev, 4) && degrade_aligned(data, 4), MEDNET_E_SHAPE, "noise_patches: std or data not 4-byte aligned");
  const size_t total = (size_t)rows * ((spatial + 3) / 4);
  const dim3 grid((unsigned)grid_blocks(total, 256, DEGRADE_MAX_BLOCKS));
  hipLaunchKernelGGL(noise_patches_kernel, grid, dim3(256), 0, (hipStream_t)stream, data, stdev, (uint32_t)(seed & 0xffffffffu),
                     (uint32_t)(seed >> 32), rows, spatial);
  return check_launch("noise_patches");
}

extern "C" int mednet_filter_rows(const float* src, float* dst, int rows, int d, int h, int w, int axis, const int* row_table, int n_tables,
                                  const int* count, const int* index, const float* weight, int taps, mednet_stream stream) {
  MEDNET_REQUIRE(src && dst && row_table && count && index && weight, MEDNET_E_SHAPE, "filter_rows: null pointer");
  VOLUME_REQUIRE_EXTENTS("filter_rows", d, h, w);
  MEDNET_REQUIRE((int64_t)d * h * w < ((int64_t)1 << 31), MEDNET_E_SHAPE,
                 "filter_rows: %d x %d x %d voxels do not fit a 32-bit index (limit 2^31 - 1)", d, h, w);
  MEDNET_REQUIRE(axis >= 0 && axis <= 2, MEDNET_E_SHAPE, "filter_rows: axis %d (0, 1, 2)", axis);
  MEDNET_REQUIRE(rows >= 1, MEDNET_E_SHAPE, "filter_rows: rows %d", rows);
  MEDNET_REQUIRE(n_tables >= 1, MEDNET_E_SHAPE, "filter_rows: n_tables %d", n_tables);
  MEDNET_REQUIRE(taps >= 1 && taps <= DEGRADE_MAX_TAPS, MEDNET_E_SHAPE, "filter_rows: taps %d outside 1 .. %d", taps, DEGRADE_MAX_TAPS);
  MEDNET_REQUIRE((const void*)src != (const void*)dst, MEDNET_E_SHAPE, "filter_rows: src == dst (the pass is out of place)");
  MEDNET_REQUIRE(degrade_aligned(row_table, 4) && degrade_aligned(count, 4) && degrade_aligned(index, 4) && degrade_aligned(weight, 4),
                 MEDNET_E_SHAPE, "filter_rows: tables not 4-byte aligned");
  MEDNET_REQUIRE(degrade_aligned(src, 4) && degrade_aligned(dst, 4), MEDNET_E_SHAPE, "filter_rows: src or dst not 4-byte aligned");

  const RowTables t{row_table, n_tables, count, index, weight, taps};
  const size_t vol = (size_t)d * h * w;
  hipStream_t s = (hipStream_t)stream;
  if (axis == 2) {
    int cpl = 256;
    while (cpl / 2 >= w) cpl /= 2;  // the power of two >= min(w, 256)
    const int groups = 256 / cpl;
    const int nl = std::max(1, std::min(DEGRADE_LINES, DEGRADE_TILE / (groups * w)));
    const size_t nlines = (size_t)d * h;
    const size_t tiles = (nlines + (size_t)(groups * nl) - 1) / (size_t)(groups * nl);
    const size_t nblocks = (size_t)rows * tiles;
    const dim3 grid((unsigned)std::min(nblocks, DEGRADE_MAX_BLOCKS));
    hipLaunchKernelGGL(filter_rows_line_kernel, grid, dim3(256), 0, s, src, dst, vol, nlines, w, cpl, nl, tiles, nblocks, t);
    return check_launch("filter_rows");
  }
  const int n = axis == 0 ? d : h;
  const size_t outer = axis == 0 ? 1 : (size_t)d;
  const size_t inner = axis == 0 ? (size_t)h * w : (size_t)w;
  const bool vec = w % 4 == 0 && degrade_aligned(src, 16) && degrade_aligned(dst, 16);
  const size_t items = outer * (inner / (vec ? 4 : 1));
  const size_t chunks = (items + 255) / 256;
  const size_t nblocks = (size_t)rows * chunks * (size_t)n;
  const dim3 grid((unsigned)std::min(nblocks, DEGRADE_MAX_BLOCKS));
  if (vec)
    hipLaunchKernelGGL((filter_rows_plane_kernel<4>), grid, dim3(256), 0, s, src, dst, vol, outer, n, inner, chunks, nblocks, t);
  else
    hipLaunchKernelGGL((filter_rows_plane_kernel<1>), grid, dim3(256), 0, s, src, dst, vol, outer, n, inner, chunks, nblocks, t);
  return check_launch("filter_rows");
}
