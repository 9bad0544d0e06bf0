"""The host side of the spatial augmentation (mednet_hip/sampler.py), without a GPU: SpatialAugmentation.draw() consumes the
documented, fixed number of calls into numpy's global generator; identity ranges give the identity matrix bit for bit; a mirror is a
sign flip of one column; the matrix is R_z R_y R_x * scale * mirror; and DevicePatchSampler draws position -> spatial -> intensity per
sample, with `spatial=None` leaving the sequence of generator calls exactly as it was."""
import numpy as np
import pytest
import torch

from mednet_hip import sampler as HS
from mednet_hip.sampler import SpatialAugmentation


class _Counter:
    """Counts calls into numpy's global generator, by name."""
    NAMES = ("uniform", "normal", "randint", "choice", "random")

    def __init__(self, monkeypatch):
        self.calls = []
        for name in self.NAMES:
            monkeypatch.setattr(np.random, name, self._wrap(name, getattr(np.random, name)))

    def _wrap(self, name, fn):
        def inner(*a, **k):
            self.calls.append(name)
            return fn(*a, **k)
        return inner


FULL = dict(rotation=((-0.3, 0.3), (-0.2, 0.2), (-0.1, 0.4)), scale=(0.8, 1.2), mirror_axes=(0, 2), elastic=(4, 1.5))


@pytest.mark.parametrize("kw,want", [
    (dict(), []),
    (dict(rotation=FULL["rotation"]), ["uniform"] * 4),
    (dict(scale=(0.8, 1.2)), ["uniform"] * 2),
    (dict(mirror_axes=(0, 1, 2)), ["uniform"] * 3),
    (dict(elastic=(4, 1.5)), ["uniform", "normal"]),
    (FULL, ["uniform"] * 4 + ["uniform"] * 2 + ["uniform"] * 2 + ["uniform", "normal"]),
    (dict(FULL, p_rotation=0.0, p_scale=0.0, p_elastic=0.0), ["uniform"] * 9 + ["normal"]),
])
def test_draw_consumes_a_fixed_documented_number_of_generator_calls(monkeypatch, kw, want):
    sp = SpatialAugmentation(**kw)
    counter = _Counter(monkeypatch)
    np.random.seed(3)
    for _ in range(4):
        counter.calls.clear()
        sp.draw([1, 2, 3], [8, 9, 10])
        assert counter.calls == want and len(want) == sp.calls_per_sample()


def test_identity_ranges_give_the_identity_bit_for_bit_and_the_centre_offset():
    sp = SpatialAugmentation(rotation=((0, 0),) * 3, scale=(1, 1))
    np.random.seed(0)
    a, lattice = sp.draw([3, 0, 7], [4, 5, 7])
    assert lattice is None and a.dtype == np.float32 and a.shape == (12,)
    want = np.concatenate([np.eye(3), [[3 + 1.5], [0 + 2.0], [7 + 3.0]]], axis=1).astype(np.float32)
    assert a.tobytes() == want.tobytes()          # also no negative zero
    off = SpatialAugmentation(**dict(FULL, mirror_axes=(), p_rotation=0.0, p_scale=0.0, p_elastic=0.0))
    a, lattice = off.draw([3, 0, 7], [4, 5, 7])
    assert a.tobytes() == want.tobytes() and lattice.shape == (3, 2, 3, 3) and not lattice.any()


def test_a_mirror_is_a_sign_flip_of_one_column(monkeypatch):
    base = dict(rotation=((0.3, 0.3), (-0.2, -0.2), (0.5, 0.5)), scale=(1.25, 1.25))
    np.random.seed(1)
    plain = SpatialAugmentation(**base).draw([0, 0, 0], [8, 8, 8])[0].reshape(3, 4)
    for axis in (0, 1, 2):
        flipped = None
        for seed in range(20):            # until the coin of the mirror falls on "flip"
            np.random.seed(seed)
            a = SpatialAugmentation(mirror_axes=(axis,), **base).draw([0, 0, 0], [8, 8, 8])[0].reshape(3, 4)
            if not np.array_equal(a, plain):
                flipped = a
                break
        assert flipped is not None
        want = plain.copy()
        want[:, axis] = -want[:, axis]
        assert flipped.tobytes() == want.tobytes()


def test_the_matrix_is_rz_ry_rx_times_scale_rounded_once():
    ax, ay, az, f = 0.3, -0.2, 0.5, 1.25
    sp = SpatialAugmentation(rotation=((ax, ax), (ay, ay), (az, az)), scale=(f, f))
    np.random.seed(2)
    a = sp.draw([0, 0, 0], [8, 8, 8])[0].reshape(3, 4)
    rx = np.array([[np.cos(ax), -np.sin(ax), 0], [np.sin(ax), np.cos(ax), 0], [0, 0, 1]])
    ry = np.array([[np.cos(ay), 0, -np.sin(ay)], [0, 1, 0], [np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[1, 0, 0], [0, np.cos(az), -np.sin(az)], [0, np.sin(az), np.cos(az)]])
    assert a[:, :3].tobytes() == ((rz @ ry @ rx) * f).astype(np.float32).tobytes()
    m = a[:, :3].astype(np.float64) / f
    assert np.allclose(m @ m.T, np.eye(3), atol=1e-6) and np.linalg.det(m) > 0
    assert np.array_equal(a[:, 3], np.float32([3.5, 3.5, 3.5]))


def _volumes(rng):
    images = [rng.standard_normal((1, 12, 12, 12)).astype(np.float16) for _ in range(2)]
    labels = [rng.integers(0, 3, (1, 12, 12, 12)).astype(np.uint8) for _ in range(2)]
    return images, labels


def _host_only(monkeypatch):
    """batch() without a device: the launches are cut out, the draws stay."""
    monkeypatch.setattr(HS.L, "require_gpu", lambda *a, **k: None)
    monkeypatch.setattr(HS.DevicePatchSampler, "_crop_batch", lambda self, *a: None)
    monkeypatch.setattr(HS, "warp_patches", lambda *a, **k: None)
    monkeypatch.setattr(HS, "augment_", lambda data, params: data)


@pytest.mark.parametrize("augment", [False, True])
def test_spatial_none_leaves_the_generator_calls_unchanged_and_spatial_draws_sit_between(monkeypatch, augment):
    _host_only(monkeypatch)
    images, labels = _volumes(np.random.default_rng(0))
    kw = dict(samples_per_subject=2, class_probabilities=[0.2, 0.4, 0.4], device="cpu", augment=augment)
    indices = [0, 1, 2, 3]
    # the sequence as it was before the option existed: position, then the intensity draws, per sample
    plain = HS.DevicePatchSampler(images, labels, [6, 6, 6], **kw)
    np.random.seed(7)
    want_pos = []
    for i in indices:
        want_pos.append(plain.position(i)[1])
        if augment:
            HS.draw_augmentation(1)
    want_state = np.random.get_state()[1].copy()
    np.random.seed(7)
    b = plain.batch(indices)
    assert np.array_equal(np.random.get_state()[1], want_state) and np.array_equal(b["patch_position"], np.stack(want_pos))
    assert "spatial" not in b and plain.last_spatial is None
    # an augmentation that draws nothing: still the same sequence, and identity matrices
    np.random.seed(7)
    b = HS.DevicePatchSampler(images, labels, [6, 6, 6], spatial=SpatialAugmentation(), **kw).batch(indices)
    assert np.array_equal(np.random.get_state()[1], want_state) and np.array_equal(b["patch_position"], np.stack(want_pos))
    assert b["spatial"].shape == (4, 3, 4) and np.array_equal(b["spatial"][:, :, :3], np.stack([np.eye(3, dtype=np.float32)] * 4))
    assert np.array_equal(b["spatial"][:, :, 3], np.stack(want_pos) + 2.5)
    # with draws: position -> spatial -> intensity, per sample
    sp = SpatialAugmentation(**FULL)
    ds = HS.DevicePatchSampler(images, labels, [6, 6, 6], spatial=sp, **kw)
    np.random.seed(7)
    want = []
    for i in indices:
        pos = ds.position(i)[1]
        want.append(sp.draw(pos, [6, 6, 6]))
        if augment:
            HS.draw_augmentation(1)
    want_state = np.random.get_state()[1].copy()
    np.random.seed(7)
    b = ds.batch(indices)
    assert np.array_equal(np.random.get_state()[1], want_state)
    assert np.array_equal(b["spatial"].reshape(4, 12), np.stack([a for a, _ in want]))
    assert np.array_equal(ds.last_spatial["lattice"], np.stack([g for _, g in want])) and ds.last_spatial["lattice"].shape == (4, 3, 3, 3, 3)
