// Connected components of a uint8 volume on the device (additive to ABI 3): labelling, per-component statistics, selection.
//   cc_label   six launches on ONE int32 volume, which holds parents first and ids at the end:
//                init     every foreground voxel gets 1 + the linear index of the start of its x-run inside its 256-voxel wave chunk,
//                         found from four ballots of "does not continue its left neighbour" -- no walk, no chain along x
//                merge    label equivalence (Playne-Hawick / Komura): voxels whose earlier neighbours are not already joined through
//                         the x-predecessor unite their set with those neighbours' sets; atomicMin on the larger root
//                flatten  L[v] = find(v), and the roots of every numbering row are counted
//                scan     one workgroup: exclusive prefix sum over the rows, K
//                mark     roots get -(their id): ids in raster order of each component's first voxel, which IS its root
//                write    every foreground voxel takes |L[root]|
//   cc_stats   two launches: the table's neutral elements, then one set of integer atomics per x-run piece of a wave
//   cc_select  one launch: out = keep[label] ? vol : fill on labelled voxels
// Integer atomics only (order-independent), nothing waits for another workgroup inside a launch, every loop that follows parents
// has a step cap (see unite()), every neighbour test is on coordinates.
#include "volume.h"

namespace mednet {

constexpr size_t CC_MAX_BLOCKS = 8192;   // grid of the passes that have no numbering rows (the rows are volume.h's row plan)
constexpr int CC_CHUNK = 256;            // voxels of a wave in init: 64 lanes x one aligned 4-byte word of the volume

// 0 on background, else what two connected voxels must agree in
__device__ __forceinline__ int cc_key(int val, int cls, int invert) {
  if (cls < 0) return val;  // MEDNET_CC_ALL: every non-zero voxel, joined only with its own value
  return ((val == cls) != (invert != 0)) ? 1 : 0;
}

// The four voxels of the aligned 4-byte word `word` of the volume: voxel indices first .. first + 3 with first = 4 * word - off,
// off = the volume's byte address mod 4.  A word that lies inside the volume is ONE 4-byte load; the first and the last word are
// read byte by byte, so nothing outside [vol, vol + vox) is touched.  Out-of-range voxels get key 0.
__device__ __forceinline__ void cc_load4(const uint8_t* __restrict__ vol, int64_t first, int64_t vox, int cls, int invert, int k[4]) {
  if (first >= 0 && first + 4 <= vox) {
    const unsigned u = *reinterpret_cast<const unsigned*>(vol + first);
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = cc_key((int)((u >> (8 * j)) & 0xFFu), cls, invert);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t v = first + j;
      k[j] = (v >= 0 && v < vox) ? cc_key((int)vol[v], cls, invert) : 0;
    }
  }
}

__device__ __forceinline__ int cc_peek(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cc_poke(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cc_report(int64_t* info) {
  atomicOr(reinterpret_cast<unsigned long long*>(info + 1), 1ull);
}

// ---------------------------------------------------------------------------------------------- init
// Parents are stored as 1 + linear index, 0 is background.  Lane l of a wave holds word l of its chunk; brk_j says voxel j of the
// word starts a piece (background, x == 0, another key than its left neighbour, or the chunk's first voxel).  The start of a
// foreground voxel's piece is the last brk at or before it: inside the lane, else the highest set bit below the lane in the four
// ballots.  A run that crosses a chunk border is joined again by merge (one union per border, at most w / 256 of them per run).
__global__ __launch_bounds__(256) void cc_init_kernel(const uint8_t* __restrict__ vol, int off, int64_t vox, int w, int cls,
                                                      int invert, int* __restrict__ labels, int64_t* __restrict__ info) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    info[0] = 0;
    info[1] = 0;
  }
  const int lane = threadIdx.x & 63;
  const int64_t nwords = (vox + off + 3) / 4;
  const bool vec = ((reinterpret_cast<uintptr_t>(labels) & 15) == 0) && off == 0;
  for (int64_t wb = (int64_t)blockIdx.x * 256; wb < nwords; wb += (int64_t)gridDim.x * 256) {  // uniform: every lane takes part
    const int64_t word = wb + threadIdx.x;
    const int64_t first = 4 * word - off;
    int k[4];
    cc_load4(vol, first, vox, cls, invert, k);
    int left = __shfl_up(k[3], 1);
    if (lane == 0) left = (first > 0 && first <= vox) ? cc_key((int)vol[first - 1], cls, invert) : 0;
    const int x0 = (int)((first + 4 * (int64_t)w) % w);  // first >= -3: the x of voxel `first`, also left of voxel 0
    bool brk[4];
    unsigned long long ball[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = (x0 + j) % w;
      const int prev = j ? k[j - 1] : left;
      brk[j] = !(k[j] != 0 && x > 0 && prev == k[j]) || (j == 0 && lane == 0) || first + j <= 0;
      ball[j] = __ballot(brk[j]);
    }
    int start = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned long long m = ball[j] & below;
      if (m) {
        const int c = 4 * (63 - __clzll((long long)m)) + j;
        start = c > start ? c : start;
      }
    }
    const int64_t chunk_first = 4 * (word - lane) - off;
    int lab[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (brk[j]) start = 4 * lane + j;
      lab[j] = k[j] ? (int)(chunk_first + start) + 1 : 0;
    }
    if (first >= 0 && first + 4 <= vox && vec) {
      typedef __attribute__((ext_vector_type(4))) int i32x4;
      i32x4 o = {lab[0], lab[1], lab[2], lab[3]};
      *reinterpret_cast<i32x4*>(labels + first) = o;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (first + j >= 0 && first + j < vox) labels[first + j] = lab[j];
    }
  }
}

// ---------------------------------------------------------------------------------------------- union-find
// INVARIANT: a parent entry P[i] (1-based ids, P[i] stored at L[i - 1]) is written by init with a value <= i and, during merge, by
// atomicMin alone, so P[i] <= i always holds and every value ever stored in P[i] is a member of i's set.
//   * a step of find() moves to a strictly smaller id: at most vox - 1 steps;
//   * a round of unite() that does not end replaces the larger of its two ids by a value the atomicMin returned, which is smaller
//     than it, and find() only moves ids down: the larger id strictly decreases from round to round, at most vox - 1 rounds.
// A load may return ANY earlier value of an entry (eight private L2s): that is still a member of the set with a smaller or equal
// id, so a stale value only costs steps.  "Is a root" is never concluded from a load: unite() ends only when the value its own
// atomicMin RETURNED says the entry still pointed at itself, or when both sides reached the same id.  Each loop counts its steps
// against the voxel count; the invariant proves the cap unreachable -- it is there so that a coding error becomes info[1] != 0
// and a failed assertion instead of a wave that spins.
__device__ __forceinline__ int cc_find(const int* L, int id, unsigned cap, bool& bad) {
  int p = cc_peek(L + id - 1);
  unsigned steps = 0;
  while (p != id) {
    if (++steps > cap) {
      bad = true;
      break;
    }
    id = p;
    p = cc_peek(L + id - 1);
  }
  return id;
}

__device__ __forceinline__ void cc_unite(int* L, int a, int b, unsigned cap, int64_t* info) {
  bool bad = false;
  for (unsigned rounds = 0; rounds < cap && !bad; ++rounds) {
    a = cc_find(L, a, cap, bad);
    b = cc_find(L, b, cap, bad);
    if (bad) break;
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(L + a - 1, b);  // device scope
    if (old == a) return;                     // a was a root when the atomic landed and now hangs under b
    a = old;                                  // a had a parent already: its set (through old) and b's still have to meet
  }
  cc_report(info);
}

// Earlier neighbours of v = (z, y, x), apart from the x-predecessor (init joined it, or the chunk-border union below does): the rows
// (z, y - 1), (z - 1, y - 1), (z - 1, y), (z - 1, y + 1), each at x - 1, x, x + 1 as far as the connectivity allows (c = 1, 2, 3
// axes may differ: 6, 18, 26).  A union is left out where it is implied:
//   * v continues its x-predecessor p and the neighbour's own left neighbour n - 1 has the key too: n - 1 is the SAME neighbour of
//     p, p joins it (or leaves it to ITS predecessor; a run start joins for real), and n - 1, n are one run;
//   * the neighbour left of n in the same row is a neighbour of v as well and has the key: that union covers n.
__global__ __launch_bounds__(256) void cc_merge_kernel(const uint8_t* __restrict__ vol, int off, int64_t vox, int d, int h, int w,
                                                       int cls, int invert, int c, int* L, int64_t* info) {
  const int64_t nwords = (vox + off + 3) / 4;
  const unsigned cap = (unsigned)vox;
  for (int64_t word = (int64_t)blockIdx.x * 256 + threadIdx.x; word < nwords; word += (int64_t)gridDim.x * 256) {
    const int64_t first = 4 * word - off;
    int k[4];
    cc_load4(vol, first, vox, cls, invert, k);
    if (!(k[0] | k[1] | k[2] | k[3])) continue;
    const int left = (first > 0) ? cc_key((int)vol[first - 1], cls, invert) : 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int key = k[j];
      if (!key) continue;
      const int64_t v = first + j;
      const auto [z, y, x] = voxel_zyx(v, h, w);
      const bool cont = x > 0 && (j ? k[j - 1] : left) == key;
      if (cont && ((v + off) & (CC_CHUNK - 1)) == 0) cc_unite(L, (int)v + 1, (int)v, cap, info);  // a run cut by a chunk border
      for (int r = 0; r < 4; ++r) {
        const int dz = r ? -1 : 0, dy = r == 2 ? 0 : r == 3 ? 1 : -1;
        const int m = (dz != 0) + (dy != 0);
        const int zz = z + dz, yy = y + dy;
        if (m > c || zz < 0 || yy < 0 || yy >= h) continue;
        const int64_t base = ((int64_t)zz * h + yy) * w;
        int a[4];  // keys at x - 2 .. x + 1 of that row, 0 outside it
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int xx = x - 2 + q;
          a[q] = (xx >= 0 && xx < w) ? cc_key((int)vol[base + xx], cls, invert) : 0;
        }
        const bool side = m + 1 <= c;
        if (side && a[1] == key && !(cont && a[0] == key)) cc_unite(L, (int)v + 1, (int)(base + x - 1) + 1, cap, info);
        if (a[2] == key && !(a[1] == key && (side || cont))) cc_unite(L, (int)v + 1, (int)(base + x) + 1, cap, info);
        if (side && a[3] == key && a[2] != key) cc_unite(L, (int)v + 1, (int)(base + x + 1) + 1, cap, info);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- flatten, scan, mark, write
// After merge every set is a tree whose root r has P[r] = r, the smallest id of the set: its first voxel in raster order.
__global__ __launch_bounds__(256) void cc_flatten_kernel(int* L, int64_t vox, int64_t share, unsigned* __restrict__ rows,
                                                         int64_t* info) {
  __shared__ unsigned red[256];
  int64_t begin, end;
  row_range(vox, share, begin, end);
  const unsigned cap = (unsigned)vox;
  unsigned roots = 0;
  for (int64_t v = begin + threadIdx.x; v < end; v += 256) {
    const int p = L[v];  // only this thread writes L[v]
    if (p <= 0) continue;
    bool bad = false;
    const int r = cc_find(L, p, cap, bad);
    if (bad) cc_report(info);
    if (r != p) cc_poke(L + v, r);  // a root is never rewritten here: finds of other threads through v stay valid
    roots += r == (int)v + 1 ? 1u : 0u;
  }
  roots = block_tree(roots, red, [](unsigned a, unsigned b) { return a + b; });  // integer sum: any order gives the same result
  if (threadIdx.x == 0) rows[blockIdx.x] = roots;
}

// one workgroup: rows[r] becomes the number of roots in the rows before r, info[0] = K
__global__ __launch_bounds__(256) void cc_scan_kernel(unsigned* __restrict__ rows, unsigned nrows, int64_t* __restrict__ info) {
  __shared__ unsigned part[256];
  const unsigned per = (nrows + 255) / 256, r0 = threadIdx.x * per;
  unsigned s = 0;
  for (unsigned r = r0; r < r0 + per && r < nrows; ++r) s += rows[r];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned run = 0;
    for (int t = 0; t < 256; ++t) {
      const unsigned n = part[t];
      part[t] = run;
      run += n;
    }
    info[0] = (int64_t)run;
  }
  __syncthreads();
  unsigned run = part[threadIdx.x];
  for (unsigned r = r0; r < r0 + per && r < nrows; ++r) {
    const unsigned n = rows[r];
    rows[r] = run;
    run += n;
  }
}

// roots, in raster order inside the row: L[r] = -(roots before the row + roots before r in the row + 1)
__global__ __launch_bounds__(256) void cc_mark_kernel(int* __restrict__ L, int64_t vox, int64_t share,
                                                      const unsigned* __restrict__ rows) {
  __shared__ unsigned wave_n[4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int64_t begin, end;
  row_range(vox, share, begin, end);
  unsigned run = rows[blockIdx.x];
  for (int64_t base = begin; base < end; base += 256) {  // uniform: the barriers are reached by every thread
    const int64_t v = base + threadIdx.x;
    const bool root = v < end && L[v] == (int)v + 1;
    const unsigned long long b = __ballot(root);
    if (lane == 0) wave_n[wid] = (unsigned)__popcll(b);
    __syncthreads();
    unsigned before = (unsigned)__popcll(b & ((1ull << lane) - 1ull));
    unsigned total = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      before += q < wid ? wave_n[q] : 0u;
      total += wave_n[q];
    }
    if (root) L[v] = -(int)(run + before + 1u);
    run += total;
    __syncthreads();
  }
}

// A root holds -id until its own thread turns it into +id below; a reader of either takes the magnitude.
__global__ __launch_bounds__(256) void cc_write_kernel(int* L, int64_t vox) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < vox; v += (int64_t)gridDim.x * 256) {
    const int p = L[v];  // still what flatten / mark left: only this thread writes L[v]
    if (p == 0) continue;
    int id = -p;
    if (p > 0) {
      const int q = cc_peek(L + p - 1);
      id = q < 0 ? -q : q;
    }
    cc_poke(L + v, id);
  }
}

// ---------------------------------------------------------------------------------------------- statistics
constexpr int CC_COLS = 11;  // count, zmin, zmax, ymin, ymax, xmin, xmax, sum z, sum y, sum x, value

__global__ __launch_bounds__(256) void cc_table_init_kernel(int64_t* __restrict__ table, int64_t k) {
  const int64_t n = k * CC_COLS;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int col = (int)(e % CC_COLS);
    table[e] = (col == 1 || col == 3 || col == 5) ? (int64_t)VOLUME_MAX_EXTENT : (col == 2 || col == 4 || col == 6) ? -1 : 0;
  }
}

__device__ __forceinline__ void cc_add(int64_t* p, int64_t v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}
__device__ __forceinline__ void cc_min(int64_t* p, int64_t v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cc_max(int64_t* p, int64_t v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// A lane starts a piece where its label differs from the left lane's, at x == 0 and at lane 0; the piece ends before the next
// start of the ballot.  The starting lane adds the whole piece: its length, x0 .. x1 and the sum of x in closed form.
__global__ __launch_bounds__(256) void cc_stats_kernel(const uint8_t* __restrict__ vol, const int* __restrict__ labels, int64_t vox,
                                                       int h, int w, int64_t k, int64_t* __restrict__ table) {
  const int lane = threadIdx.x & 63;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < vox; base += (int64_t)gridDim.x * 256) {  // uniform: ballots see every lane
    const int64_t v = base + threadIdx.x;
    const bool valid = v < vox;
    const int lab = valid ? labels[v] : 0;
    const int left = __shfl_up(lab, 1);
    const auto [z, y, x] = valid ? voxel_zyx(v, h, w) : Zyx{0, 0, 0};
    const bool start = !valid || lane == 0 || x == 0 || lab != left;
    const unsigned long long b = __ballot(start);
    if (valid && start && lab > 0 && (int64_t)lab <= k) {
      const unsigned long long above = b & ~((2ull << lane) - 1ull);
      const int len = (above ? __ffsll((long long)above) - 1 : 64) - lane;
      int64_t* t = table + (int64_t)(lab - 1) * CC_COLS;
      cc_add(t + 0, len);
      cc_min(t + 1, z);
      cc_max(t + 2, z);
      cc_min(t + 3, y);
      cc_max(t + 4, y);
      cc_min(t + 5, x);
      cc_max(t + 6, x + len - 1);
      cc_add(t + 7, (int64_t)z * len);
      cc_add(t + 8, (int64_t)y * len);
      cc_add(t + 9, (int64_t)x * len + (int64_t)len * (len - 1) / 2);
      cc_max(t + 10, (int64_t)vol[v]);
    }
  }
}

// ---------------------------------------------------------------------------------------------- selection
__global__ __launch_bounds__(256) void cc_select_kernel(const uint8_t* vol, const int* __restrict__ labels,
                                                        const uint8_t* __restrict__ keep, uint8_t fill, uint8_t* out, int64_t vox) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < vox; v += (int64_t)gridDim.x * 256) {
    const int lab = labels[v];
    out[v] = (lab > 0 && !keep[lab]) ? fill : vol[v];  // out may be vol: a voxel is read and written by one thread
  }
}

}  // namespace mednet

// =================================================================================================== C ABI
using namespace mednet;

static inline bool cc_volume_ok(int d, int h, int w) { return (size_t)d * h * w < ((size_t)1 << 31); }
#define CC_REQUIRE_EXTENTS(who, d, h, w) \
  VOLUME_REQUIRE_EXTENTS(who, d, h, w);    \
  MEDNET_REQUIRE(cc_volume_ok(d, h, w), MEDNET_E_SHAPE, who ": %d x %d x %d voxels do not fit a 32-bit index (limit 2^31 - 1)", d, h, w)

extern "C" size_t mednet_cc_ws_bytes(int d, int h, int w) {
  if (!extents_ok(d, h, w) || !cc_volume_ok(d, h, w)) return 0;
  return (size_t)row_plan((size_t)d * h * w).rows * sizeof(unsigned);
}

extern "C" int mednet_cc_label(const uint8_t* vol, int cls, int invert, int connectivity, int d, int h, int w, int32_t* labels,
                               int64_t* info, void* ws, size_t ws_bytes, mednet_stream stream) {
  MEDNET_REQUIRE(vol && labels && info && ws, MEDNET_E_SHAPE, "cc_label: null pointer");
  CC_REQUIRE_EXTENTS("cc_label", d, h, w);
  MEDNET_REQUIRE(cls == MEDNET_CC_ALL || (cls >= 0 && cls <= 255), MEDNET_E_SHAPE,
                 "cc_label: class %d is neither a uint8 value nor MEDNET_CC_ALL", cls);
  MEDNET_REQUIRE(invert == 0 || invert == 1, MEDNET_E_SHAPE, "cc_label: invert %d is neither 0 nor 1", invert);
  MEDNET_REQUIRE(!(cls == MEDNET_CC_ALL && invert), MEDNET_E_SHAPE, "cc_label: invert with MEDNET_CC_ALL has no meaning");
  MEDNET_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, MEDNET_E_UNSUPPORTED,
                 "cc_label: connectivity %d (supported: 6, 18, 26)", connectivity);
  MEDNET_REQUIRE(((uintptr_t)labels & 3) == 0 && ((uintptr_t)info & 7) == 0 && ((uintptr_t)ws & 3) == 0, MEDNET_E_SHAPE,
                 "cc_label: labels or workspace not 4-byte or info not 8-byte aligned");
  const size_t need = mednet_cc_ws_bytes(d, h, w);
  MEDNET_REQUIRE(ws_bytes >= need, MEDNET_E_WORKSPACE, "cc_label: workspace %zu < %zu bytes", ws_bytes, need);
  const int64_t vox = (int64_t)d * h * w;
  const auto [rows, ushare] = row_plan((size_t)vox);
  const int64_t share = (int64_t)ushare;
  const int off = (int)((uintptr_t)vol & 3);
  const uint8_t* base = vol;  // word `k` of the kernels is the aligned word at vol - off + 4 k
  const size_t wblocks = grid_blocks((size_t)(vox + off + 3) / 4, 256, CC_MAX_BLOCKS), vblocks = grid_blocks((size_t)vox, 256, CC_MAX_BLOCKS);
  const int c = connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3;
  unsigned* r = static_cast<unsigned*>(ws);
  hipStream_t s = (hipStream_t)stream;
  int rc;
  hipLaunchKernelGGL(cc_init_kernel, dim3(wblocks), dim3(256), 0, s, base, off, vox, w, cls, invert, labels, info);
  if ((rc = check_launch("cc_label(init)")) != MEDNET_OK) return rc;
  hipLaunchKernelGGL(cc_merge_kernel, dim3(wblocks), dim3(256), 0, s, base, off, vox, d, h, w, cls, invert, c, labels, info);
  if ((rc = check_launch("cc_label(merge)")) != MEDNET_OK) return rc;
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(rows), dim3(256), 0, s, labels, vox, share, r, info);
  if ((rc = check_launch("cc_label(flatten)")) != MEDNET_OK) return rc;
  hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(256), 0, s, r, rows, info);
  if ((rc = check_launch("cc_label(scan)")) != MEDNET_OK) return rc;
  hipLaunchKernelGGL(cc_mark_kernel, dim3(rows), dim3(256), 0, s, labels, vox, share, (const unsigned*)r);
  if ((rc = check_launch("cc_label(mark)")) != MEDNET_OK) return rc;
  hipLaunchKernelGGL(cc_write_kernel, dim3(vblocks), dim3(256), 0, s, labels, vox);
  return check_launch("cc_label");
}

extern "C" int mednet_cc_stats(const uint8_t* vol, const int32_t* labels, int d, int h, int w, int64_t k, int64_t* table,
                               mednet_stream stream) {
  MEDNET_REQUIRE(vol && labels && (table || k == 0), MEDNET_E_SHAPE, "cc_stats: null pointer");
  CC_REQUIRE_EXTENTS("cc_stats", d, h, w);
  MEDNET_REQUIRE(k >= 0, MEDNET_E_SHAPE, "cc_stats: k %lld is negative", (long long)k);
  MEDNET_REQUIRE(k <= (int64_t)d * h * w, MEDNET_E_SHAPE, "cc_stats: k %lld above the voxel count", (long long)k);
  MEDNET_REQUIRE(((uintptr_t)labels & 3) == 0 && ((uintptr_t)table & 7) == 0, MEDNET_E_SHAPE,
                 "cc_stats: labels not 4-byte or table not 8-byte aligned");
  if (k == 0) return MEDNET_OK;
  const int64_t vox = (int64_t)d * h * w;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cc_table_init_kernel, dim3(grid_blocks((size_t)k * CC_COLS, 256, CC_MAX_BLOCKS)), dim3(256), 0, s, table, k);
  const int rc = check_launch("cc_stats(init)");
  if (rc != MEDNET_OK) return rc;
  hipLaunchKernelGGL(cc_stats_kernel, dim3(grid_blocks((size_t)vox, 256, CC_MAX_BLOCKS)), dim3(256), 0, s, vol, labels, vox, h, w, k, table);
  return check_launch("cc_stats");
}

extern "C" int mednet_cc_select(const uint8_t* vol, const int32_t* labels, const uint8_t* keep, int fill, uint8_t* out, int d, int h,
                                int w, mednet_stream stream) {
  MEDNET_REQUIRE(vol && labels && keep && out, MEDNET_E_SHAPE, "cc_select: null pointer");
  CC_REQUIRE_EXTENTS("cc_select", d, h, w);
  MEDNET_REQUIRE(fill >= 0 && fill <= 255, MEDNET_E_SHAPE, "cc_select: fill %d is no uint8 value", fill);
  MEDNET_REQUIRE(((uintptr_t)labels & 3) == 0, MEDNET_E_SHAPE, "cc_select: labels not 4-byte aligned");
  const int64_t vox = (int64_t)d * h * w;
  hipLaunchKernelGGL(cc_select_kernel, dim3(grid_blocks((size_t)vox, 256, CC_MAX_BLOCKS)), dim3(256), 0, (hipStream_t)stream, vol, labels, keep,
                     (uint8_t)fill, out, vox);
  return check_launch("cc_select");
}
