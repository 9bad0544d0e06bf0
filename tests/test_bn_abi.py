"""BatchNorm3d of the 'b' layer orders (components.py:58-63) without a GPU: the C ABI carries the mednet_bn_* entry points
(header, library, ctypes table) and the order grammar builds this package's module, interchangeable with torch.nn.BatchNorm3d."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mednet_hip.h")
BN_SYMBOLS = ["mednet_bn_act_bwd", "mednet_bn_act_bwd_fused", "mednet_bn_eval_coef", "mednet_bn_stats"]


def test_bn_symbols_declared_exported_and_listed():
    from mednet_hip import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(s for s in set(re.findall(r"\b(mednet_[a-z0-9_]+)\s*\(", text)) if s.startswith("mednet_bn_"))
    assert declared == BN_SYMBOLS
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    h = ctypes.CDLL(_lib.LIB_PATH)
    for s in BN_SYMBOLS:
        assert hasattr(h, s), f"not exported: {s}"
        assert s in _lib.SIGNATURES, f"not in the ctypes table: {s}"
    assert _lib.lib().mednet_abi_version() == 3  # (additive change)


def test_order_b_builds_the_package_module_with_torch_state_dict():
    from mednet_hip import nn as hnn
    from mednet_hip.unet import components as HC
    bn = HC.SingleConv(8, 16, 3, "cbe", 8).batchnorm
    assert isinstance(bn, hnn.BatchNorm3d) and not isinstance(bn, torch.nn.BatchNorm3d)
    stock = torch.nn.BatchNorm3d(16)
    assert (bn.eps, bn.momentum, bn.affine, bn.track_running_stats) == (stock.eps, stock.momentum, stock.affine, stock.track_running_stats)
    a, b = bn.state_dict(), stock.state_dict()
    assert list(a) == list(b) == ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert torch.equal(a[k], b[k]), k  # (same defaults: ones / zeros / 0)
    with torch.no_grad():
        for i, t in enumerate(stock.state_dict().values()):
            t.copy_(torch.arange(t.numel()).reshape(t.shape) + i)
    bn.load_state_dict(stock.state_dict())
    for k, v in stock.state_dict().items():
        assert torch.equal(bn.state_dict()[k], v), k
    back = torch.nn.BatchNorm3d(16)
    back.load_state_dict(bn.state_dict())
    for k, v in stock.state_dict().items():
        assert torch.equal(back.state_dict()[k], v), k
    assert [k for k, _ in bn.named_parameters()] == ["weight", "bias"]
    assert [k for k, _ in bn.named_buffers()] == ["running_mean", "running_var", "num_batches_tracked"]


def test_module_options():
    from mednet_hip import nn as hnn
    with pytest.raises(NotImplementedError, match="momentum=None"):
        hnn.BatchNorm3d(8, momentum=None)
    m = hnn.BatchNorm3d(8, affine=False, track_running_stats=False)
    ref = torch.nn.BatchNorm3d(8, affine=False, track_running_stats=False)
    assert list(m.state_dict()) == list(ref.state_dict()) == []
    assert m.weight is None and m.running_mean is None and m.num_batches_tracked is None


def test_every_b_order_of_the_grammar_uses_it():
    from mednet_hip import nn as hnn
    from mednet_hip.unet import model as HM
    for net in (HM.ResidualUNet3D(1, 3, False, f_maps=[16, 32], conv_layer_order="cbe"),
                HM.UNet3D(1, 3, False, f_maps=[16, 32], layer_order="cbr")):
        kinds = {type(m) for m in net.modules() if "BatchNorm" in type(m).__name__}
        assert kinds == {hnn.BatchNorm3d}, kinds
