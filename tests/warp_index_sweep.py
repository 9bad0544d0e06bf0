"""csrc/warp_index.h on the host: the kernel's coordinate -> index functions compiled with a stand-alone main and swept over 0, +-0.5,
n - 1, n - 0.5, +-2^23, +-2^31, +-2^62, +-inf and NaN at extents 1, 2, 7 and 512.  Shared by tests/test_warp_index_host.py (CPU suite: under the
host compiler's address and undefined-behaviour sanitizers, and once in a plain build) and by the GPU case with non-finite matrices
in tests/test_gpu_warp.py, which runs the PLAIN build only -- sanitizer builds stay in the CPU suite -- and launches nothing unless
the sweep is green.

A compiler is PROBED first with a trivial program under -fsanitize=address,undefined.  Only "no compiler here has the sanitizer
runtimes" is a reason to go without them; once a compiler passed the probe, a failure to compile the header or the sweep is a
failure of the code under test."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "torch-mednet_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
CHECKED = 27 * 2 * 4      # coordinates x borders x extents

PROBE = "int main(void) { return 0; }\n"

MAIN = r"""
#include <stdio.h>
#include <math.h>
#include "warp_index.h"
int main(void) {
  const int extents[4] = {1, 2, 7, 512};
  int bad = 0, checked = 0;
  for (int e = 0; e < 4; ++e) {
    const int n = extents[e];
    const float base[] = {0.f, 0.5f, -0.5f, (float)n - 1.f, (float)n - 0.5f, 8388608.f, -8388608.f, 2147483648.f, -2147483648.f,
                          4611686018427387904.f, -4611686018427387904.f, INFINITY, -INFINITY, NAN, -NAN, -1.f, -1.5f, -2.f, -2.5f,
                          (float)n, (float)n + 0.5f, (float)n + 1.f, (float)n + 1.5f, 1e-30f, -1e-30f, 3.4e38f, -3.4e38f};
    for (unsigned k = 0; k < sizeof(base) / sizeof(base[0]); ++k) {
      for (int border = 0; border < 2; ++border) {
        const float s = base[k];
        const mednet_warp_cell c = mednet_warp_linear_cell(s, n, border);
        int inside = -1;
        const int i = mednet_warp_nearest_index(s, n, border, &inside);
        ++checked;
        int ok = c.i0 >= 0 && c.i0 < n && c.i1 >= 0 && c.i1 < n && i >= 0 && i < n && c.w >= 0.f && c.w <= 1.f;
        if (border == MEDNET_WARP_EDGE) ok = ok && c.in0 && c.in1 && inside;
        else {
          /* the flags of a finite coordinate are those of floor(s), floor(s) + 1 and floor(s + 0.5); anything else is outside */
          const int finite = s == s && fabsf(s) < 1e6f;
          const double f = finite ? floor((double)s) : -5.0, r = finite ? floor((double)(s + 0.5f)) : -5.0;
          ok = ok && c.in0 == (f >= 0 && f < n) && c.in1 == (f + 1 >= 0 && f + 1 < n) && inside == (r >= 0 && r < n);
          if (finite && c.in0) ok = ok && c.i0 == (int)f && c.w == (float)((double)s - f);
          if (finite && inside) ok = ok && i == (int)r;
        }
        if (!ok) {
          ++bad;
          printf("BAD n=%d s=%g border=%d: cell %d,%d in %d,%d w %g nearest %d in %d\n", n, (double)s, border, c.i0, c.i1, c.in0, c.in1,
                 (double)c.w, i, inside);
        }
      }
    }
  }
  printf("checked %d bad %d\n", checked, bad);
  return bad != 0;
}
"""


def _candidates():
    """(compiler, extra flags): the sanitizer runtimes linked statically where the compiler offers it, so the program stands alone."""
    out = []
    gxx = shutil.which("g++")
    if gxx:
        out.append((gxx, ["-static-libasan", "-static-libubsan"]))
    for cxx in (shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and os.path.exists(cxx):
            out.append((cxx, []))
    if gxx:
        out.append((gxx, []))
    return out


def _runs(cmd):
    return subprocess.run(cmd, capture_output=True, text=True)


def sanitizing_compiler(tmp):
    """The first compiler that builds AND runs a trivial program under the sanitizers, or (None, why)."""
    src, exe = os.path.join(tmp, "probe.cpp"), os.path.join(tmp, "probe")
    with open(src, "w") as f:
        f.write(PROBE)
    why = []
    for cxx, extra in _candidates():
        b = _runs([cxx] + extra + SANITIZE + [src, "-o", exe])
        if b.returncode == 0:
            r = _runs([exe])
            if r.returncode == 0:
                return (cxx, extra), None
            why.append(f"{cxx}: the probe does not run: {r.stderr[-200:]}")
        else:
            why.append(f"{cxx}: {b.stderr[-200:]}")
    return None, " | ".join(why) or "no host C++ compiler"


def plain_compiler():
    c = _candidates()
    return (c[-1][0], []) if c else None


def sweep(tmp, compiler, sanitize):
    """Build and run the sweep.  Raises AssertionError with the compiler's or the program's output on any failure."""
    cxx, extra = compiler
    src, exe = os.path.join(tmp, "warp_index_main.cpp"), os.path.join(tmp, "warp_index_main")
    with open(src, "w") as f:
        f.write(MAIN)
    flags = (extra + SANITIZE) if sanitize else []
    build = _runs([cxx, "-std=c++17", "-O1", "-g"] + flags + ["-I", HEADER_DIR, src, "-o", exe])
    assert build.returncode == 0, f"{cxx} does not compile csrc/warp_index.h with the sweep:\n{build.stderr[-3000:]}"
    run = _runs([exe])
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-2000:]
    assert f"checked {CHECKED} bad 0" in run.stdout, run.stdout[-500:]
