"""csrc/warp_index.h under the host compiler's address and undefined-behaviour sanitizers (a float -> int conversion out of range is
what -fsanitize=undefined reports): tests/warp_index_sweep.py sweeps 0, +-0.5, n - 1, n - 0.5, +-2^23, +-2^31, +-2^62, +-inf and NaN at
extents 1, 2, 7 and 512; every tap index is inside [0, n), outside taps are flagged under the constant border, and the sanitizers stay
silent.  Skipped only if no compiler on the machine can build and run a TRIVIAL program with the sanitizers; with one that can, a
compile error in the header or the sweep fails the test."""
import pytest

import warp_index_sweep as S


def test_index_header_under_host_sanitizers(tmp_path):
    compiler, why = S.sanitizing_compiler(str(tmp_path))
    if compiler is None:
        pytest.skip("no host compiler with sanitizer runtimes: " + why)
    S.sweep(str(tmp_path), compiler, sanitize=True)


def test_index_header_sweep_without_sanitizers(tmp_path):
    """The same sweep with a plain build: the index ranges themselves, on every machine that can build the library."""
    compiler = S.plain_compiler()
    assert compiler is not None, "no host C++ compiler"
    S.sweep(str(tmp_path), compiler, sanitize=False)
