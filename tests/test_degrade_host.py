"""The host half of the degradation transforms (mednet_hip/sampler.py) without a GPU: the draw protocol of ImageDegradation, pickling,
table deduplication, the tap limit, and csrc/degrade_index.h under the host compiler's sanitizers in a stand-alone program."""
import itertools
import pickle

import numpy as np
import pytest

from mednet_hip import sampler as HS

import degrade_index_sweep as DS
import warp_index_sweep as S


def _state_after(calls, seed):
    np.random.seed(seed)
    for _ in range(calls):
        np.random.uniform()
    return np.random.get_state()


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("channels", [1, 4])
def test_calls_per_sample_for_every_combination_of_probabilities(channels):
    for ps in itertools.product((0.0, 1.0), repeat=5):
        deg = HS.ImageDegradation(p_noise=ps[0], p_blur=ps[1], p_blur_channel=ps[2], p_low_resolution=ps[3], p_low_resolution_channel=ps[4])
        assert deg.calls_per_sample(channels) == 4 + 4 * channels
        np.random.seed(11)
        out = deg.draw(channels)
        assert _same_state(np.random.get_state(), _state_after(deg.calls_per_sample(channels), 11)), ps
        assert out.shape == (channels, 3)
        on = (ps[0] == 1, ps[1] == ps[2] == 1, ps[3] == ps[4] == 1)
        assert ((out[:, 0] > 0).all() if on[0] else (out[:, 0] == 0).all()), ps
        assert ((out[:, 1] >= 0.5).all() if on[1] else (out[:, 1] == 0).all()), ps
        assert ((out[:, 2] < 1).all() if on[2] else (out[:, 2] == 1).all()), ps
        if on[0]:
            assert (out[:, 0] == out[0, 0]).all() and 0 <= out[0, 0] <= 0.1       # one standard deviation per sample
        if on[1] and channels > 1:
            assert len(set(out[:, 1])) == channels                                # one sigma per channel
    # a switched-off transform makes no call at all
    only_noise = HS.ImageDegradation(blur=None, low_resolution=None)
    assert only_noise.calls_per_sample(channels) == 2
    np.random.seed(5)
    only_noise.draw(channels)
    assert _same_state(np.random.get_state(), _state_after(2, 5))
    assert HS.ImageDegradation(noise=None, blur=None, low_resolution=None).calls_per_sample(channels) == 0


def test_defaults_are_nnunets_and_the_class_pickles():
    deg = HS.ImageDegradation()
    assert (deg.noise, deg.blur, deg.low_resolution) == ((0.0, 0.1), (0.5, 1.0), (0.5, 1.0))
    assert (deg.p_noise, deg.p_blur, deg.p_blur_channel, deg.p_low_resolution, deg.p_low_resolution_channel) == (0.1, 0.2, 0.5, 0.25, 0.5)
    again = pickle.loads(pickle.dumps(HS.ImageDegradation(noise=(0.0, 0.2), blur=None, p_low_resolution=0.7)))
    assert again.__dict__ == HS.ImageDegradation(noise=(0.0, 0.2), blur=None, p_low_resolution=0.7).__dict__
    np.random.seed(3)
    a = again.draw(2)
    np.random.seed(3)
    assert np.array_equal(a, HS.ImageDegradation(noise=(0.0, 0.2), blur=None, p_low_resolution=0.7).draw(2))


def test_tables_of_a_pass_are_deduplicated_and_padded():
    built = []

    def table_of(n, sigma):
        built.append((n, sigma))
        return HS.blur_table(n, sigma)

    params = [0.5, 0.0, 1.0, 0.5, 1.0, 0.0, 0.5]
    row_table, count, index, weight = HS.stack_tables(9, params, table_of)
    assert built == [(9, 0.5), (9, 0.0), (9, 1.0)]                       # each distinct (n, parameter) once
    assert row_table.tolist() == [0, -1, 1, 0, 1, -1, 0] and row_table.dtype == np.int32
    assert count.shape == (2, 9) and index.shape == weight.shape == (2, 9, 9)
    assert (count[0] == 5).all() and (count[1] == 9).all()              # sigma 0.5: r = 2; sigma 1: r = 4, padded to 9 slots
    assert (weight[0, :, 5:] == 0).all() and np.array_equal(weight[0, :, :5], HS.blur_table(9, 0.5)[2])
    assert np.array_equal(index[1], HS.blur_table(9, 1.0)[1])
    assert HS.stack_tables(9, [0.0, 0.0], table_of) is None              # no row has a table: the pass launches nothing
    assert HS.stack_tables(9, [1.0, 2.5, 0.3], HS.low_resolution_table)[0].tolist() == [-1, -1, 0]


def test_a_sigma_too_large_for_64_taps_is_refused():
    assert HS.blur_table(16, 7.8)[3] == 63                               # r = 31
    for sigma in (7.9, 8.0, 100.0):                                      # r = 32: 65 taps
        with pytest.raises(ValueError, match="taps"):
            HS.blur_table(16, sigma)
    with pytest.raises(ValueError, match="taps"):
        HS.ImageDegradation(blur=(0.5, 9.0))
    with pytest.raises(ValueError):
        HS.blur_table(16, float("nan"))
    with pytest.raises(ValueError):
        HS.low_resolution_table(16, 0.0)


def test_clamp_header_under_host_sanitizers(tmp_path):
    compiler, why = S.sanitizing_compiler(str(tmp_path))
    if compiler is None:
        pytest.skip("no host compiler with sanitizer runtimes: " + why)
    DS.sweep(str(tmp_path), compiler, sanitize=True)


def test_clamp_header_sweep_without_sanitizers(tmp_path):
    """The same sweep with a plain build: the clamps themselves, on every machine that can build the library."""
    compiler = S.plain_compiler()
    assert compiler is not None, "no host C++ compiler"
    DS.sweep(str(tmp_path), compiler, sanitize=False)
