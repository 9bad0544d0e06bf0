"""csrc/degrade_index.h on the host: the clamps of mednet_filter_rows compiled with a stand-alone main and swept over the indices 0,
-1, -5, n - 1, n, 2^30, INT_MIN and INT_MAX at extents 1, 2, 7 and 2048, the counts 0, -1, taps and 1000 at taps 1, 13 and 64, and
the row_table entries -1, 0, T - 1, T, 99, INT_MIN and INT_MAX.  Shared by tests/test_degrade_host.py (CPU suite: under the host
compiler's address and undefined-behaviour sanitizers, and once in a plain build) and by the hostile-table case of
tests/test_gpu_degrade.py, which runs the PLAIN build only and launches nothing unless the sweep is green.  Compilers are found and
probed by tests/warp_index_sweep.py."""
import os

import warp_index_sweep as S

CHECKED = 4 * 8 + 3 * 6 + 3 * 7

MAIN = r"""
#include <stdio.h>
#include <limits.h>
#include "degrade_index.h"
int main(void) {
  int bad = 0, checked = 0;
  const int extents[4] = {1, 2, 7, 2048};
  for (int e = 0; e < 4; ++e) {
    const int n = extents[e];
    const int idx[8] = {0, -1, -5, n - 1, n, 1 << 30, INT_MIN, INT_MAX};
    for (int k = 0; k < 8; ++k) {
      const int got = mednet_degrade_index(idx[k], n);
      const int want = idx[k] < 0 ? 0 : (idx[k] > n - 1 ? n - 1 : idx[k]);
      ++checked;
      if (got != want || got < 0 || got >= n) { ++bad; printf("BAD index %d n %d -> %d\n", idx[k], n, got); }
    }
  }
  const int tap_counts[3] = {1, 13, 64};
  for (int e = 0; e < 3; ++e) {
    const int taps = tap_counts[e];
    const int cnt[6] = {0, -1, taps, 1000, INT_MIN, INT_MAX};
    for (int k = 0; k < 6; ++k) {
      const int got = mednet_degrade_count(cnt[k], taps);
      const int want = cnt[k] < 1 ? 1 : (cnt[k] > taps ? taps : cnt[k]);
      ++checked;
      if (got != want || got < 1 || got > taps) { ++bad; printf("BAD count %d taps %d -> %d\n", cnt[k], taps, got); }
    }
  }
  const int table_counts[3] = {1, 2, 50};
  for (int e = 0; e < 3; ++e) {
    const int nt = table_counts[e];
    const int row[7] = {-1, 0, nt - 1, nt, 99, INT_MIN, INT_MAX};
    for (int k = 0; k < 7; ++k) {
      const int got = mednet_degrade_table(row[k], nt);
      const int want = (row[k] >= 0 && row[k] < nt) ? row[k] : -1;
      ++checked;
      if (got != want) { ++bad; printf("BAD table %d of %d -> %d\n", row[k], nt, got); }
    }
  }
  printf("checked %d bad %d\n", checked, bad);
  return bad != 0;
}
"""


def sweep(tmp, compiler, sanitize):
    """Build and run the sweep.  Raises AssertionError with the compiler's or the program's output on any failure."""
    cxx, extra = compiler
    src, exe = os.path.join(tmp, "degrade_index_main.cpp"), os.path.join(tmp, "degrade_index_main")
    with open(src, "w") as f:
        f.write(MAIN)
    flags = (extra + S.SANITIZE) if sanitize else []
    build = S._runs([cxx, "-std=c++17", "-O1", "-g"] + flags + ["-I", S.HEADER_DIR, src, "-o", exe])
    assert build.returncode == 0, f"{cxx} does not compile csrc/degrade_index.h with the sweep:\n{build.stderr[-3000:]}"
    run = S._runs([exe])
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-2000:]
    assert f"checked {CHECKED} bad 0" in run.stdout, run.stdout[-500:]
