// Coordinate -> index conversion of mednet_warp_patches (warp.hip), free of any HIP dependency: the kernel and a host program
// (tests/test_warp_index_host.py builds one with the host compiler's sanitizers) compile this very text.
//
// A source coordinate s (fp32, volume voxels along one axis of extent n) may be anything: NaN, +-inf, |s| >= 2^31.  A float is
// therefore never converted to an int before it has been clamped IN FLOAT to [-2, n + 1]:
//   * NaN counts as outside: !(s >= -2) sends it to -2;
//   * at -2 the linear cell is (-2, -1) and at n + 1 it is (n + 1, n + 2): both taps outside, weight 0, so a clamped coordinate
//     gives what the unclamped one would -- cval under the constant border, the edge voxel under the edge border.
// Precondition: n <= MEDNET_WARP_MAX_EXTENT = 2^24 - 2, so that n + 1 and every index of [-2, n + 2] are exact in fp32;
// mednet_warp_patches refuses a larger volume, patch or lattice extent before it launches (the lattice coordinate, at most
// extent - 1, is converted without a clamp of its own).
#ifndef MEDNET_WARP_INDEX_H
#define MEDNET_WARP_INDEX_H
#include <math.h>

#define MEDNET_WARP_MAX_EXTENT 16777214

#ifndef MEDNET_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define MEDNET_HD __host__ __device__
#else
#define MEDNET_HD
#endif
#endif

enum { MEDNET_WARP_CONSTANT = 0, MEDNET_WARP_EDGE = 1 };  // = MEDNET_BORDER_CONSTANT / MEDNET_BORDER_EDGE of mednet_hip.h

struct mednet_warp_cell {
  int i0, i1;    // tap indices, always in [0, n): an outside tap is clamped AND flagged, so that it is never dereferenced wrongly
  int in0, in1;  // 1: the tap reads the volume; 0: it reads cval (constant border only; the edge border never clears a flag)
  float w;       // weight of tap i1, s - floor(s), in [0, 1]
};

MEDNET_HD static inline float mednet_warp_clamp(float s, int n) {
  const float hi = (float)n + 1.0f;
  if (!(s >= -2.0f)) return -2.0f;  // below, -inf and NaN
  return s > hi ? hi : s;
}

MEDNET_HD static inline int mednet_warp_clampi(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// linear: cell floor(s), weight s - floor(s) (exact: both below 2^23 after the clamp)
MEDNET_HD static inline mednet_warp_cell mednet_warp_linear_cell(float s, int n, int border) {
  mednet_warp_cell c;
  const float sc = mednet_warp_clamp(s, n);
  const float f = floorf(sc);
  c.w = sc - f;
  const int i0 = (int)f, i1 = i0 + 1;  // in [-2, n + 2]
  const int edge = border == MEDNET_WARP_EDGE;
  c.in0 = edge || (i0 >= 0 && i0 < n);
  c.in1 = edge || (i1 >= 0 && i1 < n);
  c.i0 = mednet_warp_clampi(i0, n);
  c.i1 = mednet_warp_clampi(i1, n);
  return c;
}

// nearest: floor(s + 0.5f) of the clamped coordinate; *inside as in0 above
MEDNET_HD static inline int mednet_warp_nearest_index(float s, int n, int border, int* inside) {
  const float sc = mednet_warp_clamp(s, n);
  const int i = (int)floorf(sc + 0.5f);  // in [-2, n + 2]
  *inside = border == MEDNET_WARP_EDGE || (i >= 0 && i < n);
  return mednet_warp_clampi(i, n);
}

#endif
