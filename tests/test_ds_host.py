"""Deep supervision, host side (no GPU): the model keyword and its state_dict keys, the level weights, the ValueErrors, and the
label pick rule i << s against F.interpolate(mode="nearest")."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mednet_hip import nn as hnn
from mednet_hip import train
from mednet_hip.unet import model as HM
from oracle import ref_cpu as O

import ds_util as U

CTOR = dict(in_channels=1, out_channels=4, final_sigmoid=False, f_maps=[32, 64, 128, 256])


def test_without_the_keyword_the_module_tree_is_the_reference_s():
    ora = O.ResidualUNet3D(**CTOR)
    for net in (HM.ResidualUNet3D(**CTOR), HM.ResidualUNet3D(**CTOR, deep_supervision=0)):
        assert set(net.state_dict().keys()) == set(ora.state_dict().keys())
        assert not hasattr(net, "ds_heads") and net.deep_supervision == 0
    u = dict(CTOR, f_maps=[16, 32, 64])
    assert set(HM.UNet3D(**u, deep_supervision=0).state_dict().keys()) == set(O.UNet3D(**u).state_dict().keys())


@pytest.mark.parametrize("cls", [HM.ResidualUNet3D, HM.UNet3D])
@pytest.mark.parametrize("k", [1, 2])
def test_the_keyword_adds_one_planar_1x1x1_head_per_level(cls, k):
    base = set(cls(**CTOR).state_dict().keys())
    net = cls(**CTOR, deep_supervision=k)
    new = set(net.state_dict().keys()) - base
    assert new == {f"ds_heads.{i}.{p}" for i in range(k) for p in ("weight", "bias")}
    assert net.deep_supervision == k and len(net.ds_heads) == k
    for s, head in enumerate(net.ds_heads, start=1):
        assert isinstance(head, hnn.Conv3d) and head.planar_output and head.kernel_size[0] == 1
        assert (head.in_channels, head.out_channels) == (CTOR["f_maps"][s], CTOR["out_channels"])
    assert set(U.oracle_with_heads(CTOR, k).state_dict().keys()) == set(HM.ResidualUNet3D(**CTOR, deep_supervision=k).state_dict().keys())


@pytest.mark.parametrize("k", [-1, 3, 7])
def test_a_depth_outside_the_decoder_raises(k):
    with pytest.raises(ValueError):
        HM.ResidualUNet3D(**CTOR, deep_supervision=k)
    with pytest.raises(ValueError):
        HM.UNet3D(**CTOR, deep_supervision=k)


def test_default_level_weights_halve_and_sum_to_one():
    assert train.deep_supervision_weights(0) == [1.0]
    assert train.deep_supervision_weights(2) == [4 / 7, 2 / 7, 1 / 7]
    for k in range(5):
        w = train.deep_supervision_weights(k)
        assert w == U.default_weights(k) and abs(sum(w) - 1.0) < 1e-15
        assert all(a == 2 * b for a, b in zip(w, w[1:]))
    assert train.deep_supervision_weights(2, (1, 0.5, 0)) == [1.0, 0.5, 0.0]


@pytest.mark.parametrize("bad", [(1.0,), (1.0, 0.5), (1.0, 0.5, 0.25, 0.1), (1.0, -0.5, 0.25), (1.0, float("nan"), 0.25)])
def test_wrong_level_weights_raise(bad):
    with pytest.raises(ValueError):
        train.deep_supervision_weights(2, bad)


@pytest.mark.parametrize("full", [(8, 8, 16), (12, 12, 12), (9, 13, 11), (17, 8, 23), (48, 48, 32)])
@pytest.mark.parametrize("s", [1, 2, 3])
def test_the_pick_rule_is_nearest_neighbour_interpolation(full, s):
    """label[z << s][y << s][x << s] for the level extents D >> s equals F.interpolate(scale_factor=2^-s, mode="nearest") -- which
    reads source index floor(i * 2^s) and gives floor(D * 2^-s) outputs --, also where D != (D >> s) << s; and it equals
    interpolation to the level's size of the volume cropped to (D >> s) << s, which is what a stride-2 pooling chain sees."""
    lev = tuple(v >> s for v in full)
    assert min(lev) > 0
    g = np.random.Generator(np.random.PCG64(3 + s))
    lab = torch.from_numpy(g.integers(0, 200, size=(2,) + full).astype(np.uint8))
    got = U.pick(lab, s)
    assert tuple(got.shape[1:]) == lev
    crop = lab[:, :lev[0] << s, :lev[1] << s, :lev[2] << s]
    want = F.interpolate(crop[:, None].float(), size=lev, mode="nearest")[:, 0].to(torch.uint8)
    assert torch.equal(got, want)
    zz, yy, xx = (torch.arange(v) << s for v in lev)
    assert torch.equal(got, lab[:, zz[:, None, None], yy[None, :, None], xx[None, None, :]])
    assert torch.equal(got, F.interpolate(lab[:, None].float(), scale_factor=2.0 ** -s, mode="nearest")[:, 0].to(torch.uint8))
