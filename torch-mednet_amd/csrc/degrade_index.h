// The clamps of mednet_filter_rows (degrade.hip), free of any HIP dependency: the kernels and a host program
// (tests/degrade_index_sweep.py builds one with the host compiler's sanitizers) compile this very text.
//
// A table handed to mednet_filter_rows may hold anything: every tap index is clamped to [0, n), every count to [1, taps] and a
// row_table entry outside [0, n_tables) counts as -1 (the row is copied), so any table is safe for memory.  Integer comparisons
// only: nothing here can overflow, also at INT_MIN and INT_MAX.
#ifndef MEDNET_DEGRADE_INDEX_H
#define MEDNET_DEGRADE_INDEX_H

#ifndef MEDNET_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define MEDNET_HD __host__ __device__
#else
#define MEDNET_HD
#endif
#endif

// a tap's source index along an axis of extent n >= 1
MEDNET_HD static inline int mednet_degrade_index(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// the taps of an output, taps >= 1
MEDNET_HD static inline int mednet_degrade_count(int count, int taps) { return count < 1 ? 1 : (count > taps ? taps : count); }

// the table of a row: -1 (identity) for every entry outside [0, n_tables)
MEDNET_HD static inline int mednet_degrade_table(int t, int n_tables) { return (t < 0 || t >= n_tables) ? -1 : t; }

#endif
