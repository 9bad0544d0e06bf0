// Intensity normalisation of device-resident volumes: exact order statistics (a masked multi-level radix select), two-pass fp64
// moments, the apply table of a scheme, the fused clip / shift / scale / convert pass, and the non-zero mask with its box.
//
// MEMBERSHIP.  Voxel (z, y, x) of channel c takes part iff mask[z, y, x] != 0 (no mask: every voxel) and its value is not NaN.  The
// mask is d x h x w uint8, shared by the channels, read where it lies and never past its last voxel.  n_nan counts the NaN voxels
// of a channel inside the mask.  +-inf are values like any other.  Every source value (f32, f16, i16, u8) is converted to fp32
// first, which is exact for all four.
//
// SELECT, pinned.  key(x): u = bits(x), x == 0 -> u = 0 (so -0.0 is +0.0); key = u < 2^31 ? u | 2^31 : ~u -- the order of the keys
// is the order of the values.  The key is resolved in three levels of 11, 11 and 10 bits.  A level is one pass over the volume into
// LDS histograms (one per channel at level 0, one per (channel, rank) afterwards, counting only keys whose higher bits equal the
// rank's prefix), added into 64-bit global histograms with integer adds, and a walk kernel that moves each rank's prefix and
// remaining rank on in device memory.  Integers only: the result is a pure function of the input, whatever the order of the adds.
// A rank outside [0, n) gives NaN in its slot.  Duplicates: before the LDS add the lanes of a wave that carry the leading lane's bin
// are added as one (twice), so a wave of equal values costs two adds, not 64 serialised ones.
//
// MOMENTS, pinned.  Pass A: n, n_nan, min, max and sum x, each thread in fp64, block_tree, one partial row per workgroup, rows summed
// in fixed order.  mean = sum / n in fp64 on the device.  Pass B: sum (x - mean)^2 with d = x - mean, acc = acc + d * d, unfused.
// std = sqrt(sum / n), the population form.  No float atomics.  n = 0: mean, std, min, max are NaN.
//
// PARAMETERS, pinned (fp64, rounded to fp32 once).  Percentile q of n: pos = q / 100 * (n - 1), ranks floor(pos) and
// min(floor(pos) + 1, n - 1), t = pos - floor(pos), value = t == 0 ? a : a + (b - a) * t with __dmul_rn / __dadd_rn.
//     zscore   (-inf, +inf, mean, 1 / max(std, eps))
//     ct       (p_lo, p_hi, mean, 1 / max(std, eps))
//     rescale  (p_lo, p_hi, p_lo, 1 / max(p_hi - p_lo, eps))
//
// APPLY, pinned (fp32).  y = __fmul_rn(__fsub_rn(fminf(fmaxf(x, lo), hi), sub), mul), one round-to-nearest-even store for f16.  A
// voxel outside the mask, and a NaN voxel, gets `fill`.  In place is legal for equal dtypes: a thread reads what it owns first.
//
// MAPPING.  Bandwidth kernels over the row plan of volume.h (grid rows x channels): 16-byte loads per lane (8 bytes for u8) over the
// aligned body of a row, scalar head and tail.
#include <math.h>
#include "common.h"
#include "volume.h"

namespace mednet {

constexpr int SEL_BINS = 2048;
constexpr int SEL_LEVELS = 3;

struct SelState {
  unsigned prefix, invalid;
  int64_t rem;
};
struct MomRow {
  int64_t n, n_nan;
  double s;
  float mn, mx;
};
struct MomState {
  int64_t n, n_nan;
  double sum;
  float mn, mx;
  double mean, m2;
};
struct MomTable {  // one row of the public table: MEDNET_INTENSITY_TABLE_BYTES
  int64_t n, n_nan;
  float mn, mx;
  double mean, sd;
};
static_assert(sizeof(MomTable) == MEDNET_INTENSITY_TABLE_BYTES, "table row");
static_assert(sizeof(MomRow) == 32 && sizeof(MomState) == 48 && sizeof(SelState) == 16, "workspace rows");

__device__ __forceinline__ unsigned key_of(float x) {
  unsigned u = __float_as_uint(x);
  if (x == 0.f) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// ---------------------------------------------------------------------------------------------- the walk over a row
template <typename T, int V>
struct Pack { T e[V]; } __attribute__((aligned(V * sizeof(T))));
template <int V>
struct Bytes { uint8_t e[V]; };

// f(x, in_mask) for every voxel of [begin, end) of the channel at p; the aligned body in V-wide loads
template <typename T, typename F>
__device__ __forceinline__ void row_visit(const T* __restrict__ p, const uint8_t* __restrict__ mask, unsigned begin, unsigned end, F f) {
  constexpr int V = sizeof(T) == 1 ? 8 : 16 / (int)sizeof(T);
  if (begin >= end) return;
  const unsigned len = end - begin;
  unsigned head = (unsigned)((0 - (uintptr_t)(p + begin)) & (V * sizeof(T) - 1)) / (unsigned)sizeof(T);
  if (head > len) head = len;
  const unsigned nvec = (len - head) / V;
  for (unsigned i = begin + threadIdx.x; i < begin + head; i += 256) f((float)p[i], mask == nullptr || mask[i] != 0);
  const unsigned b0 = begin + head;
  for (unsigned v = threadIdx.x; v < nvec; v += 256) {
    const unsigned i = b0 + v * V;
    const Pack<T, V> a = *reinterpret_cast<const Pack<T, V>*>(p + i);
    Bytes<V> m;
    if (mask != nullptr) __builtin_memcpy(&m, mask + i, V);
#pragma unroll
    for (int j = 0; j < V; ++j) f((float)a.e[j], mask == nullptr || m.e[j] != 0);
  }
  for (unsigned i = b0 + nvec * V + threadIdx.x; i < end; i += 256) f((float)p[i], mask == nullptr || mask[i] != 0);
}

// ---------------------------------------------------------------------------------------------- select
// one LDS add per matching lane, after the lanes that share the leading lane's bin have been added as one (twice)
__device__ __forceinline__ void hist_add(unsigned* h, unsigned bin, bool match) {
  unsigned long long todo = __ballot(match);
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    if (todo == 0) return;
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned lb = (unsigned)__builtin_amdgcn_readlane((int)bin, leader);
    const unsigned long long same = __ballot(match && bin == lb);
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&h[lb], (unsigned)__popcll(same));
    todo &= ~same;
    match = match && bin != lb;
  }
  if (match) atomicAdd(&h[bin], 1u);
}

__host__ __device__ __forceinline__ int level_shift(int level) { return level == 0 ? 21 : level == 1 ? 10 : 0; }
__host__ __device__ __forceinline__ int level_bits(int level) { return level == 2 ? 10 : 11; }

template <typename T>
__global__ __launch_bounds__(256) void select_hist_kernel(const T* __restrict__ src, const uint8_t* __restrict__ mask, const unsigned vox,
                                                          const unsigned share, const int level, const int nr,
                                                          const SelState* __restrict__ st, unsigned long long* __restrict__ hist,
                                                          unsigned long long* __restrict__ nan) {
  extern __shared__ unsigned lds[];  // nh x SEL_BINS counters, then the NaN counter
  const int c = blockIdx.y;
  const int nh = level == 0 ? 1 : nr;
  for (int i = threadIdx.x; i <= nh * SEL_BINS; i += 256) lds[i] = 0u;
  unsigned pre[MEDNET_INTENSITY_MAX_RANKS];
#pragma unroll
  for (int r = 0; r < MEDNET_INTENSITY_MAX_RANKS; ++r) {
    const bool on = level > 0 && r < nr && st[c * nr + r].invalid == 0;
    pre[r] = on ? st[c * nr + r].prefix : 0xFFFFFFFFu;  // (no 11- or 22-bit prefix equals it)
  }
  __syncthreads();
  unsigned begin, end;
  row_range(vox, share, begin, end);
  const int shift = level_shift(level), hs = shift + level_bits(level);
  const unsigned bmask = (1u << level_bits(level)) - 1u;
  unsigned nn = 0;
  row_visit(src + (size_t)c * vox, mask, begin, end, [&](float x, bool in) {
    const bool isnan = x != x;
    nn += (in && isnan) ? 1u : 0u;
    const bool member = in && !isnan;
    const unsigned key = key_of(x);
    const unsigned bin = (key >> shift) & bmask;
    if (level == 0) {
      hist_add(lds, bin, member);
    } else {
      const unsigned hi = key >> hs;
#pragma unroll
      for (int r = 0; r < MEDNET_INTENSITY_MAX_RANKS; ++r)
        if (r < nr) hist_add(lds + r * SEL_BINS, bin, member && hi == pre[r]);
    }
  });
  if (level == 0 && nn) atomicAdd(&lds[SEL_BINS], nn);
  __syncthreads();
  for (int i = threadIdx.x; i < nh * SEL_BINS; i += 256)
    if (lds[i]) atomicAdd(&hist[(size_t)c * nr * SEL_BINS + i], (unsigned long long)lds[i]);
  if (level == 0 && threadIdx.x == 0 && lds[SEL_BINS]) atomicAdd(&nan[c], (unsigned long long)lds[SEL_BINS]);
}

// one workgroup per (rank, channel): find the bin that holds the remaining rank, move the prefix on
__global__ __launch_bounds__(256) void select_walk_kernel(const int level, const int nr, const int64_t* __restrict__ ranks,
                                                          SelState* __restrict__ st, const unsigned long long* __restrict__ hist,
                                                          const unsigned long long* __restrict__ nan, int64_t* __restrict__ counts,
                                                          float* __restrict__ out) {
  __shared__ unsigned long long part[256];
  const int r = blockIdx.x, c = blockIdx.y;
  const unsigned long long* h = hist + ((size_t)c * nr + (level == 0 ? 0 : r)) * SEL_BINS;
  unsigned long long s = 0;
  for (int k = 0; k < 8; ++k) s += h[threadIdx.x * 8 + k];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  SelState me = st[c * nr + r];
  if (level == 0) {
    unsigned long long total = 0;
    for (int t = 0; t < 256; ++t) total += part[t];
    me.rem = ranks[c * nr + r];
    me.invalid = (me.rem < 0 || (unsigned long long)me.rem >= total) ? 1u : 0u;
    me.prefix = 0u;
    if (r == 0 && counts != nullptr) {
      counts[2 * c] = (int64_t)total;
      counts[2 * c + 1] = (int64_t)nan[c];
    }
  }
  if (!me.invalid) {
    unsigned long long cum = 0;
    int t = 0;
    while (t < 255 && cum + part[t] <= (unsigned long long)me.rem) cum += part[t++];
    int b = t * 8;
    while (b < t * 8 + 7 && cum + h[b] <= (unsigned long long)me.rem) cum += h[b++];
    me.prefix = (me.prefix << level_bits(level)) | (unsigned)b;
    me.rem -= (int64_t)cum;
  }
  st[c * nr + r] = me;
  if (level == SEL_LEVELS - 1) out[c * nr + r] = me.invalid ? __uint_as_float(0x7FC00000u) : value_of(me.prefix);
}

// ---------------------------------------------------------------------------------------------- moments
union MomShared {
  double d[256];
  int64_t i[256];
  float f[256];
};

template <typename T>
__global__ __launch_bounds__(256) void moments_a_kernel(const T* __restrict__ src, const uint8_t* __restrict__ mask, const unsigned vox,
                                                        const unsigned share, MomRow* __restrict__ rows) {
  __shared__ MomShared sh;
  const int c = blockIdx.y;
  unsigned begin, end;
  row_range(vox, share, begin, end);
  int64_t n = 0, nn = 0;
  double s = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  row_visit(src + (size_t)c * vox, mask, begin, end, [&](float x, bool in) {
    const bool isnan = x != x;
    nn += (in && isnan) ? 1 : 0;
    if (in && !isnan) {
      ++n;
      s = __dadd_rn(s, (double)x);
      mn = fminf(mn, x);
      mx = fmaxf(mx, x);
    }
  });
  n = block_tree(n, sh.i, [](int64_t a, int64_t b) { return a + b; });
  nn = block_tree(nn, sh.i, [](int64_t a, int64_t b) { return a + b; });
  s = block_tree(s, sh.d, [](double a, double b) { return __dadd_rn(a, b); });
  mn = block_tree(mn, sh.f, [](float a, float b) { return fminf(a, b); });
  mx = block_tree(mx, sh.f, [](float a, float b) { return fmaxf(a, b); });
  if (threadIdx.x == 0) rows[(size_t)c * gridDim.x + blockIdx.x] = MomRow{n, nn, s, mn, mx};
}

template <typename T>
__global__ __launch_bounds__(256) void moments_b_kernel(const T* __restrict__ src, const uint8_t* __restrict__ mask, const unsigned vox,
                                                        const unsigned share, const MomState* __restrict__ st, MomRow* __restrict__ rows) {
  __shared__ MomShared sh;
  const int c = blockIdx.y;
  unsigned begin, end;
  row_range(vox, share, begin, end);
  const double mean = st[c].mean;
  double s = 0.0;
  row_visit(src + (size_t)c * vox, mask, begin, end, [&](float x, bool in) {
    if (in && x == x) {
      const double dv = __dsub_rn((double)x, mean);
      s = __dadd_rn(s, __dmul_rn(dv, dv));
    }
  });
  s = block_tree(s, sh.d, [](double a, double b) { return __dadd_rn(a, b); });
  if (threadIdx.x == 0) rows[(size_t)c * gridDim.x + blockIdx.x] = MomRow{0, 0, s, 0.f, 0.f};
}

__device__ __forceinline__ void table_write(MomTable* t, const MomState& a, bool with_std) {
  const double qnan = __longlong_as_double(0x7FF8000000000000ll);
  const float fnan = __uint_as_float(0x7FC00000u);
  const bool none = a.n == 0;
  *t = MomTable{a.n, a.n_nan, none ? fnan : a.mn, none ? fnan : a.mx, none ? qnan : a.mean,
                (none || !with_std) ? qnan : sqrt(a.m2 / (double)a.n)};
}

// one workgroup per channel: the rows of this call in fixed order, then onto the running state
__global__ __launch_bounds__(256) void moments_reduce_kernel(const MomRow* __restrict__ rows, const unsigned nrows, const int pass,
                                                             const int first, const int last, MomState* __restrict__ st,
                                                             MomTable* __restrict__ table) {
  __shared__ MomShared sh;
  const int c = blockIdx.x;
  int64_t n = 0, nn = 0;
  double s = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  for (unsigned r = threadIdx.x; r < nrows; r += 256) {
    const MomRow a = rows[(size_t)c * nrows + r];
    n += a.n, nn += a.n_nan;
    s = __dadd_rn(s, a.s);
    if (pass == 0) mn = fminf(mn, a.mn), mx = fmaxf(mx, a.mx);
  }
  n = block_tree(n, sh.i, [](int64_t a, int64_t b) { return a + b; });
  nn = block_tree(nn, sh.i, [](int64_t a, int64_t b) { return a + b; });
  s = block_tree(s, sh.d, [](double a, double b) { return __dadd_rn(a, b); });
  mn = block_tree(mn, sh.f, [](float a, float b) { return fminf(a, b); });
  mx = block_tree(mx, sh.f, [](float a, float b) { return fmaxf(a, b); });
  if (threadIdx.x != 0) return;
  MomState a = st[c];
  if (pass == 0) {
    if (first) a = MomState{0, 0, 0.0, INFINITY, -INFINITY, 0.0, 0.0};
    a.n += n, a.n_nan += nn;
    a.sum = __dadd_rn(a.sum, s);
    a.mn = fminf(a.mn, mn), a.mx = fmaxf(a.mx, mx);
    if (last) a.mean = a.sum / (double)a.n;
  } else {
    a.m2 = first ? s : __dadd_rn(a.m2, s);
  }
  st[c] = a;
  if (last) table_write(table + c, a, pass == 1);
}

// ---------------------------------------------------------------------------------------------- ranks and parameters
struct Quantiles { double q[MEDNET_INTENSITY_MAX_RANKS / 2]; };

__global__ void ranks_kernel(const MomTable* __restrict__ table, const int c, const Quantiles qs, const int nq, int64_t* __restrict__ ranks,
                             double* __restrict__ frac) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c * nq) return;
  const int ch = i / nq, k = i - ch * nq;
  const int64_t n = table[ch].n;
  int64_t lo = 0, hi = 0;
  double t = 0.0;
  if (n > 0) {
    const double pos = __dmul_rn(__ddiv_rn(qs.q[k], 100.0), (double)(n - 1));
    const double fl = floor(pos);
    lo = (int64_t)fl;
    if (lo > n - 1) lo = n - 1;
    hi = lo + 1 < n - 1 ? lo + 1 : n - 1;
    t = __dsub_rn(pos, fl);
  }
  ranks[(size_t)ch * 2 * nq + 2 * k] = lo;
  ranks[(size_t)ch * 2 * nq + 2 * k + 1] = hi;
  frac[i] = t;
}

__device__ __forceinline__ double percentile_of(float a, float b, double t) {
  if (t == 0.0) return (double)a;
  return __dadd_rn((double)a, __dmul_rn(__dsub_rn((double)b, (double)a), t));
}

__global__ __launch_bounds__(256) void params_kernel(const int scheme, const MomTable* __restrict__ table, const float* __restrict__ order,
                                                     const double* __restrict__ frac, const int nq, const int c, const double eps,
                                                     double* __restrict__ pct, float* __restrict__ out) {
  for (int i = threadIdx.x; i < c * nq && pct != nullptr; i += 256) {
    const int ch = i / nq, k = i - ch * nq;
    pct[i] = percentile_of(order[(size_t)ch * 2 * nq + 2 * k], order[(size_t)ch * 2 * nq + 2 * k + 1], frac[i]);
  }
  for (int ch = threadIdx.x; ch < c && out != nullptr; ch += 256) {
    double lo = -INFINITY, hi = INFINITY, sub, mul;
    if (scheme != MEDNET_INTENSITY_ZSCORE) {
      lo = percentile_of(order[(size_t)ch * 2 * nq], order[(size_t)ch * 2 * nq + 1], frac[ch * nq]);
      hi = percentile_of(order[(size_t)ch * 2 * nq + 2], order[(size_t)ch * 2 * nq + 3], frac[ch * nq + 1]);
    }
    if (scheme == MEDNET_INTENSITY_RESCALE) {
      const double span = __dsub_rn(hi, lo);
      sub = lo;
      mul = __ddiv_rn(1.0, span > eps ? span : eps);  // (a NaN span takes eps, like max(NaN, eps) of the restatement)
    } else {
      const double sd = table[ch].sd;
      sub = table[ch].mean;
      mul = __ddiv_rn(1.0, sd > eps ? sd : eps);
    }
    out[4 * ch] = (float)lo, out[4 * ch + 1] = (float)hi, out[4 * ch + 2] = (float)sub, out[4 * ch + 3] = (float)mul;
  }
}

// ---------------------------------------------------------------------------------------------- apply
__device__ __forceinline__ float apply_one(float x, bool in, const float* __restrict__ t, float fill) {
  if (!in || x != x) return fill;
  return __fmul_rn(__fsub_rn(fminf(fmaxf(x, t[0]), t[1]), t[2]), t[3]);
}
__device__ __forceinline__ void ap_store(float* p, float v) { *p = v; }
__device__ __forceinline__ void ap_store(f16* p, float v) { *p = (f16)v; }

template <typename TS, typename TD>
__global__ __launch_bounds__(256) void apply_kernel(const TS* src, TD* dst, const uint8_t* __restrict__ mask, const size_t total,
                                                    const unsigned vox, const float* __restrict__ table, const float fill,
                                                    const size_t groups) {
  const size_t stride = (size_t)gridDim.x * 256, tid = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (size_t g = tid; g < groups; g += stride) {
    const size_t i = g * 4;
    const Pack<TS, 4> a = *reinterpret_cast<const Pack<TS, 4>*>(src + i);
    unsigned c = (unsigned)(i / vox), m = (unsigned)(i - (size_t)c * vox);
    Pack<TD, 4> r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool in = mask == nullptr || mask[m] != 0;
      ap_store(&r.e[j], apply_one((float)a.e[j], in, table + 4 * c, fill));
      if (++m == vox) m = 0, ++c;
    }
    *reinterpret_cast<Pack<TD, 4>*>(dst + i) = r;
  }
  for (size_t i = groups * 4 + tid; i < total; i += stride) {
    const unsigned c = (unsigned)(i / vox), m = (unsigned)(i - (size_t)c * vox);
    ap_store(dst + i, apply_one((float)src[i], mask == nullptr || mask[m] != 0, table + 4 * c, fill));
  }
}

// ---------------------------------------------------------------------------------------------- non-zero mask and box
__global__ void box_init_kernel(int* box, int d, int h, int w, int after) {
  if (!after) {
    box[0] = d, box[1] = h, box[2] = w, box[3] = box[4] = box[5] = -1;
  } else if (box[3] < 0) {
    box[0] = box[1] = box[2] = 0;
  }
}

// V = 1 or 4 consecutive voxels per thread and trip (4: vox % 4 == 0 and aligned bases -- one load per channel, one 32-bit store);
// a capped grid walked in grid strides, the box in registers, then LDS, then six global integer min / max per workgroup
template <typename T, int V>
__global__ __launch_bounds__(256) void nonzero_kernel(const T* __restrict__ src, const int c, const int h, const int w, const unsigned vox,
                                                      uint8_t* __restrict__ mask, int* __restrict__ box) {
  __shared__ int sb[6];
  if (threadIdx.x < 6) sb[threadIdx.x] = threadIdx.x < 3 ? 0x7FFFFFFF : -1;
  __syncthreads();
  int lo[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, hi[3] = {-1, -1, -1};
  const unsigned groups = vox / V;
  for (unsigned g = blockIdx.x * 256u + threadIdx.x; g < groups; g += gridDim.x * 256u) {
    const unsigned i = g * V;
    bool nz[V];
#pragma unroll
    for (int j = 0; j < V; ++j) nz[j] = false;
    for (int k = 0; k < c; ++k) {
      const Pack<T, V> a = *reinterpret_cast<const Pack<T, V>*>(src + (size_t)k * vox + i);
#pragma unroll
      for (int j = 0; j < V; ++j) nz[j] = nz[j] || !((float)a.e[j] == 0.f);  // (NaN != 0)
    }
    Pack<uint8_t, V> m;
#pragma unroll
    for (int j = 0; j < V; ++j) m.e[j] = nz[j] ? 1 : 0;
    *reinterpret_cast<Pack<uint8_t, V>*>(mask + i) = m;
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (nz[j]) {
        const Zyx p = voxel_zyx(i + j, h, w);
        lo[0] = min(lo[0], p.z), lo[1] = min(lo[1], p.y), lo[2] = min(lo[2], p.x);
        hi[0] = max(hi[0], p.z), hi[1] = max(hi[1], p.y), hi[2] = max(hi[2], p.x);
      }
  }
  if (hi[0] >= 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) atomicMin(&sb[k], lo[k]), atomicMax(&sb[3 + k], hi[k]);
  }
  __syncthreads();
  if (threadIdx.x < 6 && sb[3] >= 0) {
    if (threadIdx.x < 3) atomicMin(&box[threadIdx.x], sb[threadIdx.x]);
    else atomicMax(&box[threadIdx.x], sb[threadIdx.x]);
  }
}

static inline bool volume_32bit(int d, int h, int w) { return (int64_t)d * h * w < ((int64_t)1 << 31); }
static inline bool aligned_to(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
static inline bool source_dtype(int dt) { return dt == MEDNET_F32 || dt == MEDNET_F16 || dt == MEDNET_I16 || dt == MEDNET_U8; }
static inline size_t source_size(int dt) { return dt == MEDNET_F32 ? 4 : dt == MEDNET_U8 ? 1 : 2; }
static inline size_t select_ws(int c, int nr) {
  return (size_t)c * nr * SEL_BINS * 8 + (size_t)c * 8 + (size_t)c * nr * sizeof(SelState);
}

}  // namespace mednet

using namespace mednet;

#define INTENSITY_REQUIRE_VOLUME(who, c, d, h, w)                                                                            \
  VOLUME_REQUIRE_EXTENTS(who, d, h, w);                                                                                      \
  MEDNET_REQUIRE(volume_32bit(d, h, w), MEDNET_E_SHAPE, who ": %d x %d x %d voxels do not fit a 32-bit index (limit 2^31 - 1)", d, h, w); \
  MEDNET_REQUIRE(c >= 1, MEDNET_E_SHAPE, who ": channels %d", c)
#define INTENSITY_REQUIRE_SOURCE(who, dt) \
  MEDNET_REQUIRE(source_dtype(dt), MEDNET_E_DTYPE, who ": dtype %d (supported: f32, f16, i16, u8)", dt)
// body(T) for the source type
#define INTENSITY_BY_SOURCE(dt, GO)         \
  do {                                      \
    if (dt == MEDNET_F32) GO(float);        \
    else if (dt == MEDNET_F16) GO(f16);     \
    else if (dt == MEDNET_I16) GO(int16_t); \
    else GO(uint8_t);                       \
  } while (0)

extern "C" size_t mednet_intensity_select_ws_bytes(int channels, int nranks) {
  if (channels < 1 || nranks < 1 || nranks > MEDNET_INTENSITY_MAX_RANKS) return 0;
  return select_ws(channels, nranks);
}

extern "C" int mednet_intensity_select(const void* src, int dtype, const uint8_t* mask, int c, int d, int h, int w, const int64_t* ranks,
                                       int nranks, float* out, int64_t* counts, int level, int flags, void* ws, size_t ws_bytes,
                                       mednet_stream stream) {
  MEDNET_REQUIRE(src && ranks && out && ws, MEDNET_E_SHAPE, "intensity_select: null pointer");
  INTENSITY_REQUIRE_VOLUME("intensity_select", c, d, h, w);
  INTENSITY_REQUIRE_SOURCE("intensity_select", dtype);
  MEDNET_REQUIRE(nranks >= 1 && nranks <= MEDNET_INTENSITY_MAX_RANKS, MEDNET_E_SHAPE, "intensity_select: ranks %d outside 1 .. %d", nranks,
                 MEDNET_INTENSITY_MAX_RANKS);
  MEDNET_REQUIRE(level >= MEDNET_INTENSITY_ALL && level < SEL_LEVELS, MEDNET_E_SHAPE, "intensity_select: level %d (-1: all, 0 .. %d)", level,
                 SEL_LEVELS - 1);
  MEDNET_REQUIRE(aligned_to(ranks, 8) && aligned_to(out, 4) && aligned_to(counts, 8) && aligned_to(ws, 8) &&
                     aligned_to(src, source_size(dtype)),
                 MEDNET_E_SHAPE, "intensity_select: misaligned ranks, out, counts, workspace or source");
  const size_t need = select_ws(c, nranks);
  MEDNET_REQUIRE(ws_bytes >= need, MEDNET_E_WORKSPACE, "intensity_select: workspace %zu < %zu bytes", ws_bytes, need);

  const unsigned vox = (unsigned)((size_t)d * h * w);
  const auto [rows, share] = row_plan(vox);
  unsigned long long* hist = (unsigned long long*)ws;
  unsigned long long* nan = hist + (size_t)c * nranks * SEL_BINS;
  SelState* st = (SelState*)(nan + c);
  hipStream_t s = (hipStream_t)stream;
  const int l0 = level == MEDNET_INTENSITY_ALL ? 0 : level, l1 = level == MEDNET_INTENSITY_ALL ? SEL_LEVELS - 1 : level;
  const bool first = level == MEDNET_INTENSITY_ALL || (flags & MEDNET_INTENSITY_FIRST), last = level == MEDNET_INTENSITY_ALL || (flags & MEDNET_INTENSITY_LAST);
  for (int lv = l0; lv <= l1; ++lv) {
    if (first) {
      // the histograms of this level start at zero; at level 0 the NaN counts too (they lie behind the histograms)
      const size_t bytes = (size_t)c * nranks * SEL_BINS * 8 + (lv == 0 ? (size_t)c * 8 : 0);
      if (hipMemsetAsync(ws, 0, bytes, s) != hipSuccess) return check_launch("intensity_select(clear)");
    }
    const size_t lds = ((size_t)(lv == 0 ? 1 : nranks) * SEL_BINS + 1) * sizeof(unsigned);
    const dim3 grid(rows, (unsigned)c);
    int rc = MEDNET_OK;
#define SEL_GO(T_)                                                                                                              \
  rc = launch_lds("intensity_select(histogram)", select_hist_kernel<T_>, grid, dim3(256), lds, s, (const T_*)src, mask, vox, \
                  (unsigned)share, lv, nranks, (const SelState*)st, hist, nan)
    INTENSITY_BY_SOURCE(dtype, SEL_GO);
#undef SEL_GO
    if (rc != MEDNET_OK) return rc;
    if (last) {
      hipLaunchKernelGGL(select_walk_kernel, dim3((unsigned)nranks, (unsigned)c), dim3(256), 0, s, lv, nranks, ranks, st,
                         (const unsigned long long*)hist, (const unsigned long long*)nan, counts, out);
      rc = check_launch("intensity_select(walk)");
      if (rc != MEDNET_OK) return rc;
    }
  }
  return MEDNET_OK;
}

extern "C" size_t mednet_intensity_moments_ws_bytes(int c, int d, int h, int w) {
  if (c < 1 || !extents_ok(d, h, w) || !volume_32bit(d, h, w)) return 0;
  return (size_t)c * sizeof(MomState) + (size_t)c * row_plan((size_t)d * h * w).rows * sizeof(MomRow);
}

extern "C" int mednet_intensity_moments(const void* src, int dtype, const uint8_t* mask, int c, int d, int h, int w, int pass, int flags,
                                        void* table, void* ws, size_t ws_bytes, mednet_stream stream) {
  MEDNET_REQUIRE(src && table && ws, MEDNET_E_SHAPE, "intensity_moments: null pointer");
  INTENSITY_REQUIRE_VOLUME("intensity_moments", c, d, h, w);
  INTENSITY_REQUIRE_SOURCE("intensity_moments", dtype);
  MEDNET_REQUIRE(pass >= MEDNET_INTENSITY_ALL && pass <= 1, MEDNET_E_SHAPE, "intensity_moments: pass %d (-1: both, 0, 1)", pass);
  MEDNET_REQUIRE(aligned_to(table, 8) && aligned_to(ws, 8) && aligned_to(src, source_size(dtype)), MEDNET_E_SHAPE,
                 "intensity_moments: misaligned table, workspace or source");
  const size_t need = mednet_intensity_moments_ws_bytes(c, d, h, w);
  MEDNET_REQUIRE(ws_bytes >= need, MEDNET_E_WORKSPACE, "intensity_moments: workspace %zu < %zu bytes", ws_bytes, need);

  const unsigned vox = (unsigned)((size_t)d * h * w);
  const auto [rows, share] = row_plan(vox);
  MomState* st = (MomState*)ws;
  MomRow* part = (MomRow*)(st + c);
  hipStream_t s = (hipStream_t)stream;
  const bool all = pass == MEDNET_INTENSITY_ALL;
  const int first = all || (flags & MEDNET_INTENSITY_FIRST) ? 1 : 0, last = all || (flags & MEDNET_INTENSITY_LAST) ? 1 : 0;
  const dim3 grid(rows, (unsigned)c);
  for (int p = all ? 0 : pass; p <= (all ? 1 : pass); ++p) {
    if (p == 0) {
#define MA_GO(T_) hipLaunchKernelGGL(moments_a_kernel<T_>, grid, dim3(256), 0, s, (const T_*)src, mask, vox, (unsigned)share, part)
      INTENSITY_BY_SOURCE(dtype, MA_GO);
#undef MA_GO
    } else {
#define MB_GO(T_) \
  hipLaunchKernelGGL(moments_b_kernel<T_>, grid, dim3(256), 0, s, (const T_*)src, mask, vox, (unsigned)share, (const MomState*)st, part)
      INTENSITY_BY_SOURCE(dtype, MB_GO);
#undef MB_GO
    }
    int rc = check_launch("intensity_moments(rows)");
    if (rc != MEDNET_OK) return rc;
    hipLaunchKernelGGL(moments_reduce_kernel, dim3((unsigned)c), dim3(256), 0, s, (const MomRow*)part, rows, p, first, last, st,
                       (MomTable*)table);
    rc = check_launch("intensity_moments(reduce)");
    if (rc != MEDNET_OK) return rc;
  }
  return MEDNET_OK;
}

extern "C" int mednet_intensity_ranks(const void* table, int c, double q0, double q1, double q2, double q3, int nq, int64_t* ranks,
                                      double* frac, mednet_stream stream) {
  MEDNET_REQUIRE(table && ranks && frac, MEDNET_E_SHAPE, "intensity_ranks: null pointer");
  MEDNET_REQUIRE(c >= 1, MEDNET_E_SHAPE, "intensity_ranks: channels %d", c);
  MEDNET_REQUIRE(nq >= 1 && nq <= MEDNET_INTENSITY_MAX_RANKS / 2, MEDNET_E_SHAPE, "intensity_ranks: percentiles %d outside 1 .. %d", nq,
                 MEDNET_INTENSITY_MAX_RANKS / 2);
  const Quantiles qs{{q0, q1, q2, q3}};
  for (int k = 0; k < nq; ++k)
    MEDNET_REQUIRE(qs.q[k] >= 0.0 && qs.q[k] <= 100.0, MEDNET_E_SHAPE, "intensity_ranks: percentile %g outside 0 .. 100", qs.q[k]);
  MEDNET_REQUIRE(aligned_to(table, 8) && aligned_to(ranks, 8) && aligned_to(frac, 8), MEDNET_E_SHAPE, "intensity_ranks: misaligned tables");
  hipLaunchKernelGGL(ranks_kernel, dim3((unsigned)((c * nq + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (const MomTable*)table, c, qs, nq,
                     ranks, frac);
  return check_launch("intensity_ranks");
}

extern "C" int mednet_intensity_params(int scheme, const void* table, const float* order, const double* frac, int nq, int c, double eps,
                                       double* pct, float* out, mednet_stream stream) {
  MEDNET_REQUIRE(scheme >= MEDNET_INTENSITY_ZSCORE && scheme <= MEDNET_INTENSITY_PERCENTILES, MEDNET_E_SHAPE,
                 "intensity_params: scheme %d (0 zscore, 1 ct, 2 rescale, 3 percentiles only)", scheme);
  const bool need_table = scheme == MEDNET_INTENSITY_ZSCORE || scheme == MEDNET_INTENSITY_CT;
  const bool need_order = scheme != MEDNET_INTENSITY_ZSCORE;
  MEDNET_REQUIRE((!need_table || table) && (!need_order || (order && frac)) && (out || pct) &&
                     (scheme == MEDNET_INTENSITY_PERCENTILES ? pct != nullptr : out != nullptr),
                 MEDNET_E_SHAPE, "intensity_params: null pointer");
  MEDNET_REQUIRE(c >= 1, MEDNET_E_SHAPE, "intensity_params: channels %d", c);
  if (need_order || pct) {
    const int least = scheme == MEDNET_INTENSITY_PERCENTILES ? 1 : 2;
    MEDNET_REQUIRE(nq >= least && nq <= MEDNET_INTENSITY_MAX_RANKS / 2, MEDNET_E_SHAPE, "intensity_params: percentiles %d outside %d .. %d",
                   nq, least, MEDNET_INTENSITY_MAX_RANKS / 2);
    MEDNET_REQUIRE(order && frac, MEDNET_E_SHAPE, "intensity_params: null pointer");
  }
  MEDNET_REQUIRE(eps >= 0.0, MEDNET_E_SHAPE, "intensity_params: eps %g", eps);
  MEDNET_REQUIRE(aligned_to(table, 8) && aligned_to(order, 4) && aligned_to(frac, 8) && aligned_to(pct, 8) && aligned_to(out, 4),
                 MEDNET_E_SHAPE, "intensity_params: misaligned tables");
  hipLaunchKernelGGL(params_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, scheme, (const MomTable*)table, order, frac, nq, c, eps,
                     need_order || pct ? pct : nullptr, scheme == MEDNET_INTENSITY_PERCENTILES ? nullptr : out);
  return check_launch("intensity_params");
}

extern "C" int mednet_intensity_apply(const void* src, int src_dtype, void* dst, int dst_dtype, const uint8_t* mask, int c, int d, int h,
                                      int w, const float* table, float fill, mednet_stream stream) {
  MEDNET_REQUIRE(src && dst && table, MEDNET_E_SHAPE, "intensity_apply: null pointer");
  INTENSITY_REQUIRE_VOLUME("intensity_apply", c, d, h, w);
  MEDNET_REQUIRE(source_dtype(src_dtype) && (dst_dtype == MEDNET_F32 || dst_dtype == MEDNET_F16), MEDNET_E_DTYPE,
                 "intensity_apply: dtype %d -> %d (supported: f32, f16, i16, u8 -> f32, f16)", src_dtype, dst_dtype);
  const size_t ssz = source_size(src_dtype), dsz = dst_dtype == MEDNET_F32 ? 4 : 2;
  MEDNET_REQUIRE(aligned_to(table, 4) && aligned_to(src, ssz) && aligned_to(dst, dsz), MEDNET_E_SHAPE,
                 "intensity_apply: misaligned table, source or destination");
  MEDNET_REQUIRE(src != dst || src_dtype == dst_dtype, MEDNET_E_DTYPE, "intensity_apply: dtype %d -> %d in place (equal dtypes only)",
                 src_dtype, dst_dtype);
  const unsigned vox = (unsigned)((size_t)d * h * w);
  const size_t total = (size_t)c * vox;
  const size_t groups = aligned_to(src, 4 * ssz) && aligned_to(dst, 4 * dsz) ? total / 4 : 0;
  const dim3 grid((unsigned)grid_blocks(groups ? groups : total, 256, (size_t)1 << 20));
  hipStream_t s = (hipStream_t)stream;
#define AP_GO(T_)                                                                                                                      \
  do {                                                                                                                                 \
    if (dst_dtype == MEDNET_F32)                                                                                                       \
      hipLaunchKernelGGL((apply_kernel<T_, float>), grid, dim3(256), 0, s, (const T_*)src, (float*)dst, mask, total, vox, table, fill, groups); \
    else                                                                                                                               \
      hipLaunchKernelGGL((apply_kernel<T_, f16>), grid, dim3(256), 0, s, (const T_*)src, (f16*)dst, mask, total, vox, table, fill, groups); \
  } while (0)
  INTENSITY_BY_SOURCE(src_dtype, AP_GO);
#undef AP_GO
  return check_launch("intensity_apply");
}

extern "C" int mednet_nonzero_mask(const void* src, int dtype, int c, int d, int h, int w, uint8_t* mask, int32_t* box,
                                   mednet_stream stream) {
  MEDNET_REQUIRE(src && mask && box, MEDNET_E_SHAPE, "nonzero_mask: null pointer");
  INTENSITY_REQUIRE_VOLUME("nonzero_mask", c, d, h, w);
  INTENSITY_REQUIRE_SOURCE("nonzero_mask", dtype);
  MEDNET_REQUIRE(aligned_to(box, 4) && aligned_to(src, source_size(dtype)), MEDNET_E_SHAPE, "nonzero_mask: misaligned box or source");
  const unsigned vox = (unsigned)((size_t)d * h * w);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(box_init_kernel, dim3(1), dim3(1), 0, s, box, d, h, w, 0);
  const bool vec = vox % 4 == 0 && aligned_to(src, 4 * source_size(dtype)) && aligned_to(mask, 4);
  const dim3 grid((unsigned)grid_blocks(vox / (vec ? 4 : 1), 256, VOLUME_MAX_ROWS));
#define NZ_GO(T_)                                                                                                      \
  do {                                                                                                                 \
    if (vec) hipLaunchKernelGGL((nonzero_kernel<T_, 4>), grid, dim3(256), 0, s, (const T_*)src, c, h, w, vox, mask, box); \
    else hipLaunchKernelGGL((nonzero_kernel<T_, 1>), grid, dim3(256), 0, s, (const T_*)src, c, h, w, vox, mask, box);     \
  } while (0)
  INTENSITY_BY_SOURCE(dtype, NZ_GO);
#undef NZ_GO
  hipLaunchKernelGGL(box_init_kernel, dim3(1), dim3(1), 0, s, box, d, h, w, 1);
  return check_launch("nonzero_mask");
}
