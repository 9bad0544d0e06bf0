"""The host side of mednet_hip.intensity without a GPU: bad arguments are refused in Python with the caller's name in the message,
the scheme classes pickle, and CTWindow.from_stats round-trips a hand-made IntensityStats."""
import pickle

import numpy as np
import pytest
import torch

import intensity_util as U
import mednet_hip
from mednet_hip import intensity as M
from mednet_hip import predict as HP


def test_the_module_is_part_of_the_package():
    assert mednet_hip.intensity is M and "intensity" in mednet_hip.__all__
    for name in ("order_statistics", "intensity_stats", "nonzero_mask", "crop_to_nonzero", "normalize", "ZScore", "CTWindow", "Rescale",
                 "IntensityStats"):
        assert hasattr(M, name), name
    assert M.MAX_RANKS == U.MAX_RANKS == 8


def test_cpu_tensors_are_refused():
    vol = torch.zeros((1, 4, 4, 4))
    for who, call in (("order_statistics", lambda: M.order_statistics(vol, [0])), ("intensity_stats", lambda: M.intensity_stats(vol)),
                      ("intensity_stats", lambda: M.intensity_stats([vol, vol])), ("nonzero_mask", lambda: M.nonzero_mask(vol)),
                      ("crop_to_nonzero", lambda: M.crop_to_nonzero(vol)), ("ZScore", lambda: M.ZScore()(vol)),
                      ("Rescale", lambda: M.normalize(vol, M.Rescale())), ("CTWindow", lambda: M.CTWindow(0, 1, 0, 1)(vol))):
        with pytest.raises(RuntimeError, match=rf"mednet_hip\.{who}: expected a HIP"):
            call()
    with pytest.raises(TypeError, match="order_statistics: a tensor expected"):
        M.order_statistics(np.zeros((4, 4, 4), np.float32), [0])


def test_percentiles_and_scheme_arguments_are_checked_before_any_tensor():
    for bad in ((-0.1, 50), (50, 100.5), (float("nan"), 50)):
        with pytest.raises(ValueError, match=r"intensity_stats: percentile .* outside \[0, 100\]"):
            M.intensity_stats(torch.zeros((1, 4, 4, 4)), percentiles=bad)
        with pytest.raises(ValueError, match=r"Rescale: percentile .* outside \[0, 100\]"):
            M.Rescale(percentiles=bad)
    with pytest.raises(ValueError, match="intensity_stats: 5 percentiles"):
        M.intensity_stats(torch.zeros((1, 4, 4, 4)), percentiles=(1, 2, 3, 4, 5))
    with pytest.raises(ValueError, match="intensity_stats: 0 percentiles"):
        M.intensity_stats(torch.zeros((1, 4, 4, 4)), percentiles=())
    with pytest.raises(ValueError, match="Rescale: percentiles"):
        M.Rescale(percentiles=(99.5, 0.5))
    with pytest.raises(ValueError, match="Rescale: percentiles"):
        M.Rescale(percentiles=(1, 50, 99))
    for cls in (M.ZScore, M.Rescale):
        with pytest.raises(ValueError, match=f"{cls.__name__}: mask 'body'"):
            cls(mask="body")
        with pytest.raises(ValueError, match=f"{cls.__name__}: dtype torch.bfloat16"):
            cls(dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="Rescale: mask"):
        M.Rescale(mask=torch.ones((4, 4, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match="CTWindow: dtype torch.uint8"):
        M.CTWindow(0, 1, 0, 1, dtype=torch.uint8)
    with pytest.raises(ValueError, match="CTWindow: window"):
        M.CTWindow(5, 1, 0, 1)
    with pytest.raises(ValueError, match="CTWindow: window"):
        M.CTWindow(float("nan"), 1, 0, 1)
    with pytest.raises(ValueError, match="CTWindow: lower, upper, mean and std"):
        M.CTWindow([0, 0], [1, 1], [0], [1])
    with pytest.raises(TypeError, match="normalize: a ZScore, CTWindow or Rescale expected"):
        M.normalize(torch.zeros((1, 4, 4, 4)), lambda v: v)
    with pytest.raises(ValueError, match="crop_to_nonzero: margin -1"):
        M.crop_to_nonzero(torch.zeros((1, 4, 4, 4)), margin=-1)


@pytest.mark.gpu
def test_wrong_ranks_shapes_masks_on_the_device():
    """The refusals that look at a device tensor's shape (they need a device tensor to get that far)."""
    dev = "cuda:0"
    vol = torch.zeros((2, 4, 5, 6), device=dev)
    for bad in (torch.zeros((4, 5), device=dev), torch.zeros((1, 2, 4, 5, 6), device=dev)):
        with pytest.raises(ValueError, match="order_statistics: a C x D x H x W or D x H x W volume expected"):
            M.order_statistics(bad, [0])
    with pytest.raises(ValueError, match="nonzero_mask: a float32, float16, int16 or uint8 volume expected"):
        M.nonzero_mask(vol.to(torch.bfloat16))
    with pytest.raises(ValueError, match="intensity_stats: an empty volume"):
        M.intensity_stats(torch.zeros((1, 0, 5, 6), device=dev))
    with pytest.raises(ValueError, match="order_statistics: 9 ranks"):
        M.order_statistics(vol, list(range(9)))
    with pytest.raises(ValueError, match="order_statistics: 0 ranks"):
        M.order_statistics(vol, [])
    with pytest.raises(ValueError, match="order_statistics: ranks as a tensor are int64 2 x R"):
        M.order_statistics(vol, torch.zeros((3, 2), dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="order_statistics: ranks as a tensor are int64 2 x R"):
        M.order_statistics(vol, torch.zeros((2, 2), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="order_statistics: mask .* does not match the volume's grid"):
        M.order_statistics(vol, [0], mask=torch.ones((4, 5, 7), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="ZScore: a D x H x W volume expected"):
        M.ZScore(mask=torch.ones((2, 4, 5, 6), dtype=torch.uint8, device=dev))(vol)
    with pytest.raises(ValueError, match="ZScore: a uint8 volume expected"):
        M.ZScore(mask=torch.ones((4, 5, 6), device=dev))(vol)
    with pytest.raises(RuntimeError, match=r"mednet_hip\.intensity_stats: expected a HIP"):
        M.intensity_stats(vol, masks=torch.ones((4, 5, 6), dtype=torch.uint8))
    with pytest.raises(ValueError, match="intensity_stats: 1 masks for 2 volumes"):
        M.intensity_stats([vol, vol], masks=[None])
    with pytest.raises(ValueError, match="intensity_stats: volumes with 2 and 1 channels"):
        M.intensity_stats([vol, vol[:1]])
    with pytest.raises(ValueError, match='intensity_stats: mask \'body\''):
        M.intensity_stats(vol, masks="body")
    with pytest.raises(ValueError, match="CTWindow: a scheme for 1 channels on a volume with 2"):
        M.CTWindow(0, 1, 0, 1)(vol)
    with pytest.raises(ValueError, match="ZScore: out must be a contiguous torch.float16 tensor"):
        M.ZScore()(vol, out=torch.empty((2, 4, 5, 7), dtype=torch.float16, device=dev))
    with pytest.raises(ValueError, match="crop_to_nonzero: every other tensor must end in the volume's grid"):
        M.crop_to_nonzero(vol, torch.zeros((4, 5, 7), device=dev))


def test_schemes_pickle():
    mask = torch.ones((2, 3, 4), dtype=torch.uint8)
    for s in (M.ZScore(), M.ZScore(mask="nonzero", eps=1e-5, fill=-1.0, dtype=torch.float32), M.ZScore(mask=mask),
              M.Rescale(), M.Rescale(percentiles=(1, 99), mask="nonzero", fill=0.5, dtype=torch.float32),
              M.CTWindow(-958.0, 270.5, 100.25, 76.5), M.CTWindow([0, 1], [2, 3], [1, 2], [0.5, 0.25], eps=1e-6, fill=2.0, dtype=torch.float32)):
        t = pickle.loads(pickle.dumps(s))
        assert type(t) is type(s)
        a, b = dict(s.__dict__), dict(t.__dict__)
        a.pop("_tables", None), b.pop("_tables", None)
        ma, mb = a.pop("mask", None), b.pop("mask", None)
        assert a == b and (torch.equal(ma, mb) if torch.is_tensor(ma) else ma == mb)
    ct = pickle.loads(pickle.dumps(M.CTWindow(-958.0, 270.5, 100.25, 76.5)))
    assert ct._tables == {} and ct.table().dtype == torch.float32


def hand_made_stats():
    q = (0.5, 99.5)
    return M.IntensityStats(q, n=torch.tensor([1000, 10]), n_nan=torch.tensor([0, 2]), min=torch.tensor([-1024.0, 0.0]),
                            max=torch.tensor([3071.0, 9.0]), mean=torch.tensor([100.25, 4.5], dtype=torch.float64),
                            std=torch.tensor([76.5, 2.0], dtype=torch.float64),
                            percentiles=torch.tensor([[-958.125, 270.5], [0.25, 8.75]], dtype=torch.float64),
                            order=torch.zeros((2, 2, 2)), frac=torch.zeros((2, 2), dtype=torch.float64))


def test_ct_window_from_stats_round_trip():
    stats = hand_made_stats()
    assert stats.to_host().q == stats.q and "channels=2" in repr(stats)
    ct = M.CTWindow.from_stats(stats, channel=0)
    assert (ct.lower, ct.upper, ct.mean, ct.std) == ((-958.125,), (270.5,), (100.25,), (76.5,))
    assert ct.fill == 0.0 and ct.dtype == torch.float16
    want = U.apply_table("ct", 100.25, 76.5, -958.125, 270.5, 1e-8)
    assert np.array_equal(ct.table().numpy(), want[None])
    both = M.CTWindow.from_stats(stats, eps=1e-6, dtype=torch.float32)
    assert both.lower == (-958.125, 0.25) and both.std == (76.5, 2.0) and both.dtype == torch.float32 and both.eps == 1e-6
    assert np.array_equal(both.table().numpy()[1], U.apply_table("ct", 4.5, 2.0, 0.25, 8.75, 1e-6))
    one = M.CTWindow.from_stats(stats, channel=1)
    assert one.mean == (4.5,)
    with pytest.raises(ValueError, match="CTWindow.from_stats: the statistics need two percentiles"):
        s = hand_made_stats()
        s.percentiles = s.percentiles[:, :1]
        M.CTWindow.from_stats(s)
    # a tiny std takes eps
    assert M.CTWindow(0, 1, 0, 0.0, eps=0.5).table()[0, 3] == 2.0


def test_predictor_takes_normalize_and_defaults_to_none():
    import inspect
    sig = inspect.signature(HP.GridPredictor.__init__)
    assert sig.parameters["normalize"].default is None
    net = torch.nn.Conv3d(1, 2, 1)
    assert HP.GridPredictor(net, (8, 8, 8), (1, 1, 1)).normalize is None
    s = M.ZScore()
    assert HP.GridPredictor(net, (8, 8, 8), (1, 1, 1), normalize=s).normalize is s
