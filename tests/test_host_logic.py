"""Host-side logic of the product package that needs no GPU: module tree / state_dict compatibility with the oracle
(hence with the reference), the order-string grammar and its error conventions, the import alias, and the loud
failure on CPU tensors (there is no CPU fallback)."""
import pytest
import torch

from oracle import ref_cpu as O
from mednet_hip.unet import components as HC
from mednet_hip.unet import loss as HL
from mednet_hip.unet import model as HM


@pytest.mark.parametrize("cls,ocls,kw", [
    (HM.ResidualUNet3D, O.ResidualUNet3D, dict(f_maps=[8])),
    (HM.ResidualUNet3D, O.ResidualUNet3D, dict(f_maps=[32, 64, 128, 256])),
    (HM.ResidualUNet3D, O.ResidualUNet3D, dict(f_maps=16)),
    (HM.ResidualUNet3D, O.ResidualUNet3D, dict(f_maps=[8, 16], conv_layer_order="cgr", num_groups=4)),
    (HM.UNet3D, O.UNet3D, dict(f_maps=[32, 64, 128, 256])),
    (HM.UNet3D, O.UNet3D, dict(f_maps=16)),
    (HM.UNet3D, O.UNet3D, dict(f_maps=[8, 16], layer_order="crg")),
])
def test_state_dict_interchange(cls, ocls, kw):
    a, b = cls(1, 4, False, **kw), ocls(1, 4, False, **kw)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa.keys()) == list(sb.keys())
    for k in sa:
        assert sa[k].shape == sb[k].shape, k
    a.load_state_dict(sb)  # oracle/reference checkpoint loads into the HIP module ...
    b.load_state_dict(a.state_dict())  # ... and back
    assert [n for n, _ in a.named_modules()] == [n for n, _ in b.named_modules()]


def test_param_counts():
    assert sum(p.numel() for p in HM.ResidualUNet3D(1, 2, False, f_maps=[8]).parameters()) == 3738
    assert sum(p.numel() for p in HM.ResidualUNet3D(1, 4, False, f_maps=[32, 64, 128, 256]).parameters()) == 8769860
    assert sum(p.numel() for p in HM.UNet3D(1, 4, False, f_maps=[32, 64, 128, 256]).parameters()) == 4081366
    assert HM.create_feature_maps(32, 5) == [32, 64, 128, 256, 512]


def test_default_init_statistics_match_torch():
    torch.manual_seed(0)
    a = HM.ResidualUNet3D(1, 4, False, f_maps=[32, 64])
    torch.manual_seed(0)
    b = O.ResidualUNet3D(1, 4, False, f_maps=[32, 64])
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(pa, pb), k  # same RNG consumption order and same init formulas


def test_order_grammar_errors():
    with pytest.raises(AssertionError, match="Conv layer MUST be present"):
        HC.create_conv(4, 8, 3, "ge", 8)
    with pytest.raises(AssertionError, match="Non-linearity cannot be the first"):
        HC.create_conv(4, 8, 3, "rcg", 8)
    with pytest.raises(ValueError, match="Unsupported layer type"):
        HC.create_conv(4, 8, 3, "cxg", 8)
    with pytest.raises(AssertionError, match="divisible by num_groups"):
        HC.create_conv(4, 12, 3, "cg", 8)
    names = [n for n, _ in HC.create_conv(4, 8, 3, "cge", 8)]
    assert names == ["conv", "groupnorm", "ELU"]
    mods = dict(HC.create_conv(4, 4, 3, "cg", 8))
    assert mods["groupnorm"].num_groups == 1 and mods["conv"].bias is None  # C < groups -> 1 group; no bias with norm
    assert dict(HC.create_conv(4, 8, 3, "cr", 8))["conv"].bias is not None
    assert dict(HC.create_conv(8, 16, 3, "gcr", 8))["groupnorm"].num_channels == 8


def test_double_conv_channel_rule():
    enc = HC.DoubleConv(1, 32, encoder=True, order="gcr")
    assert enc.SingleConv1.conv.weight.shape[:2] == (16, 1) and enc.SingleConv2.conv.weight.shape[:2] == (32, 16)
    enc = HC.DoubleConv(32, 40, encoder=True, order="gcr")
    assert enc.SingleConv1.conv.weight.shape[0] == 32  # max(out//2, in)
    dec = HC.DoubleConv(96, 32, encoder=False, order="gcr")
    assert dec.SingleConv1.conv.weight.shape[:2] == (32, 96) and dec.SingleConv2.conv.weight.shape[:2] == (32, 32)


def test_import_alias_resolves_to_hip_modules():
    import midasmednet.unet.components as c
    import midasmednet.unet.loss as l
    import midasmednet.unet.model as m
    assert m.ResidualUNet3D is HM.ResidualUNet3D and m.UNet3D is HM.UNet3D
    assert c.ExtResNetBlock is HC.ExtResNetBlock and l.DiceLoss is HL.DiceLoss
    for name in ["flatten", "compute_per_channel_dice", "dice_metric", "expand_as_one_hot", "DiceLoss", "CELoss",
                 "WeightedCrossEntropyLoss", "BCELossWrapper", "PixelWiseCrossEntropyLoss", "LandmarkLoss"]:
        assert hasattr(l, name)


def test_overlay_keeps_the_rest_of_the_reference_package_importable(tmp_path):
    """The shipped `midasmednet/` overlay must shadow ONLY `midasmednet.unet.*`: with it first on the path and a second
    `midasmednet` tree behind it (a stub standing in for the reference checkout: its own unet/, segmentation, dataset,
    utils), the callers' import lines (segmentation.py:16-18) get the MI355X classes while `midasmednet.segmentation`,
    `.dataset`, `.utils.*` still resolve from the second tree.  Fresh interpreter: `__path__` is fixed at first import."""
    import os
    import subprocess
    import sys
    import textwrap
    ref = tmp_path / "refcheckout" / "midasmednet"
    (ref / "unet").mkdir(parents=True)
    (ref / "utils").mkdir()
    (ref / "__init__.py").write_text("")
    (ref / "unet" / "__init__.py").write_text("")
    (ref / "unet" / "model.py").write_text("class ResidualUNet3D:\n    STUB = True\n")
    (ref / "unet" / "loss.py").write_text("STUB = True\n")
    (ref / "utils" / "__init__.py").write_text("")
    (ref / "utils" / "misc.py").write_text("WHERE = 'second tree'\n")
    (ref / "dataset.py").write_text("WHERE = 'second tree'\n")
    (ref / "segmentation.py").write_text(textwrap.dedent("""
        from midasmednet.unet.model import ResidualUNet3D
        from midasmednet.unet.loss import DiceLoss, WeightedCrossEntropyLoss, dice_metric
        from midasmednet.unet.loss import expand_as_one_hot
        from midasmednet.dataset import WHERE
        class SegmentationNet(ResidualUNet3D):
            pass
    """))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(root, "torch-mednet_amd"), str(ref.parent)]),
               PYTHONDONTWRITEBYTECODE="1")
    code = textwrap.dedent("""
        import midasmednet, midasmednet.segmentation as s, midasmednet.dataset as d, midasmednet.utils.misc as u
        import midasmednet.unet.model as m, mednet_hip.unet.model as hm, mednet_hip.unet.loss as hl
        assert m.ResidualUNet3D is hm.ResidualUNet3D and not hasattr(m.ResidualUNet3D, "STUB")
        assert s.SegmentationNet.__mro__[1] is hm.ResidualUNet3D and s.DiceLoss is hl.DiceLoss
        assert d.WHERE == u.WHERE == s.WHERE == "second tree"
        assert len(midasmednet.__path__) == 2
        print("overlay ok")
    """)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "overlay ok" in out.stdout, out.stderr[-2000:]


def _pl09_checkpoint(path, fmaps):
    """A checkpoint shaped like pytorch_lightning 0.9.0 writes it for the reference's SegmentationNet (train_seg.py:118-132):
    the oracle's weights (= the reference's state_dict keys) plus PL's bookkeeping keys."""
    import argparse
    hp = dict(in_channels=1, out_channels=2, fmaps=fmaps, learning_rate=1e-3, num_workers=0, batch_size=2, loss="DICE",
              loss_weight=[0.05, 1.0])
    ora = O.keyed_init_(O.ResidualUNet3D(1, 2, False, f_maps=fmaps))
    sd = ora.state_dict()
    sd["loss.weight"] = torch.tensor(hp["loss_weight"])  # DiceLoss registers its weight as a buffer (loss.py:99)
    torch.save({"epoch": 3, "global_step": 120, "pytorch-lightning_version": "0.9.0", "state_dict": sd,
                "optimizer_states": [{"state": {}, "param_groups": [{"lr": 1e-3}]}], "lr_schedulers": [],
                "hparams_name": "hparams", "hyper_parameters": hp, "checkpoint_callback_best_model_score": 0.5}, path)
    return ora, argparse.Namespace(**hp)


def _segmentation_net_like_the_reference():
    """The constructor contract of midasmednet/segmentation.py:22-49 on top of the product model (a stub of the caller, not
    its file): hparams object in, ResidualUNet3D.__init__(in, out, final_sigmoid=False, f_maps=hparams.fmaps), loss chosen
    from hparams."""
    class SegmentationNet(HM.ResidualUNet3D):
        def __init__(self, hparams, training_dataset=None, validation_dataset=None):
            super().__init__(hparams.in_channels, hparams.out_channels, final_sigmoid=False, f_maps=hparams.fmaps)
            self.hparams = hparams
            self.learning_rate = hparams.learning_rate
            self.loss = HL.DiceLoss(weight=torch.tensor(hparams.loss_weight))
    return SegmentationNet


def test_pl_checkpoint_interchange_and_freeze(tmp_path):
    """examples/predict.py:47-50: `SegmentationNet.load_from_checkpoint(path)`; `model.freeze()` on a PL-0.9-shaped
    checkpoint, with pytorch_lightning absent (the product model then supplies both with PL's semantics)."""
    path = tmp_path / "epoch=3.ckpt"
    ora, hp = _pl09_checkpoint(path, [8, 16])
    Net = _segmentation_net_like_the_reference()
    model = Net.load_from_checkpoint(str(path))
    assert isinstance(model, HM.ResidualUNet3D) and vars(model.hparams) == vars(hp)
    for (k, a), (k2, b) in zip(model.state_dict().items(), {**ora.state_dict(), "loss.weight": torch.tensor(hp.loss_weight)}.items()):
        assert k == k2 and torch.equal(a, b), k
    assert model.training
    model.freeze()
    assert not model.training and all(not p.requires_grad for p in model.parameters())
    model.unfreeze()
    assert model.training and all(p.requires_grad for p in model.parameters())
    # a checkpoint whose state_dict does not fit must fail loudly (strict load), as in PL
    bad = torch.load(path, weights_only=False)
    bad["state_dict"].pop("final_conv.bias")
    torch.save(bad, tmp_path / "bad.ckpt")
    with pytest.raises(RuntimeError, match="Missing key"):
        Net.load_from_checkpoint(str(tmp_path / "bad.ckpt"))
    # the product's own checkpoint loads back into the oracle (= the reference's module tree)
    ora2 = O.ResidualUNet3D(1, 2, False, f_maps=[8, 16])
    ora2.load_state_dict({k: v for k, v in model.state_dict().items() if not k.startswith("loss.")})


def test_no_cpu_fallback():
    net = HM.ResidualUNet3D(1, 2, False, f_maps=[8])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.zeros(1, 1, 8, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HL.DiceLoss()(torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 4, 4, 4, dtype=torch.long))


def test_testing_flag_and_final_activation():
    assert HM.ResidualUNet3D(1, 2, False, f_maps=[8]).testing is False
    assert HM.ResidualUNet3D(1, 2, False, f_maps=[8], testing=True).testing is True
    assert HM.ResidualUNet3D(1, 2, False, f_maps=[8], skip_final_activation=True).final_activation is None
    assert isinstance(HM.UNet3D(1, 2, True, f_maps=[8]).final_activation, torch.nn.Sigmoid)


def test_unsupported_shapes_raise():
    from mednet_hip import nn as hnn
    with pytest.raises(NotImplementedError):
        hnn.Conv3d(4, 4, 5)
    with pytest.raises(NotImplementedError):
        hnn.MaxPool3d(kernel_size=(1, 2, 2))
    with pytest.raises(NotImplementedError):
        hnn.ConvTranspose3d(4, 4, kernel_size=3, stride=(1, 2, 2))


def test_one_hot_and_generic_dice_helpers_match_oracle():
    y = torch.randint(0, 4, (2, 3, 4, 5))
    assert torch.equal(HL.expand_as_one_hot(y, 4), O.expand_as_one_hot(y, 4))
    assert torch.equal(HL.expand_as_one_hot(y, 4, ignore_index=2), O.expand_as_one_hot(y, 4, ignore_index=2))
    p = torch.softmax(torch.randn(2, 4, 3, 4, 5), 1)
    t = O.expand_as_one_hot(y, 4)
    assert torch.equal(HL.compute_per_channel_dice(p, t), O.compute_per_channel_dice(p, t))
    assert torch.equal(HL.flatten(p), O.flatten(p))


def test_predict_grid_and_crop_window_follow_the_reference():
    """mednet_hip.predict host logic (no GPU): grid positions and the crop window of the reference's slicing."""
    import numpy as np
    from mednet_hip import predict as HP
    from oracle import ref_predict as P
    for tag, shape, patch, ov, mode, nh, ncls, bs in P.PREDICT_CASES:
        img, _ = P.predict_inputs(tag, shape, patch, nh, ncls)
        ref = np.stack([i for _, i, _ in P.grid_patch_generator(img, patch, ov, mode=mode)])
        assert np.array_equal(HP.grid_positions(shape[1:], patch, ov), ref), tag
        s0, n0 = HP.crop_window(patch, ov)
        s1, n1 = P.crop_window(patch, ov)
        assert list(s0) == list(s1) and list(n0) == list(n1)
    assert HP.crop_window([8, 8, 8], [0, 2, 2]) == ([0, 2, 2], [6, 4, 4])  # the reference's first-axis quirk (dataset.py:453)
    import pytest
    with pytest.raises(ValueError):
        HP.grid_positions([8, 8, 8], [4, 4, 4], [2, 2, 2])


def test_exact_products_policy_follows_the_activation_kind():
    """fp32 storage mode: networks with kinked activations (ReLU 'r', LeakyReLU 'l' -- piecewise linear, gradient discontinuous
    in the pre-activations) ask for exact fp32 products (ALGO_EXACT), the smooth default order 'cge' takes the split-bf16
    contraction (ALGO_AUTO); a scope only turns the request on, and backward replays the forward's choice."""
    from mednet_hip import _lib as L, config
    assert config.conv_algo() == L.ALGO_AUTO
    assert not HC.SingleConv(8, 8, 3, "cge", 8)._kinked and not HC.SingleConv(8, 8, 3, "cg", 8)._kinked
    assert HC.SingleConv(8, 8, 3, "gcr", 8)._kinked and HC.SingleConv(8, 8, 3, "cl", 8)._kinked
    assert not HC.ExtResNetBlock(8, 8, order="cge")._kinked and HC.ExtResNetBlock(8, 8, order="cgr")._kinked
    assert not any(getattr(m, "_kinked", False) for m in HM.ResidualUNet3D(1, 2, False, f_maps=[8, 16]).modules())
    assert any(getattr(m, "_kinked", False) for m in HM.UNet3D(1, 2, False, f_maps=[8, 16]).modules())
    with config.exact_products(False):
        assert config.conv_algo() == L.ALGO_AUTO
    with config.exact_products(True):
        assert config.conv_algo() == L.ALGO_EXACT
        with config.exact_products(False):  # an inner smooth layer inside a kinked network stays exact
            assert config.conv_algo() == L.ALGO_EXACT
        with config.algo_scope(L.ALGO_AUTO):  # a backward whose forward ran outside the scope
            assert config.conv_algo() == L.ALGO_AUTO
        assert config.conv_algo() == L.ALGO_EXACT
    with config.algo_scope(L.ALGO_EXACT):
        assert config.conv_algo() == L.ALGO_EXACT
    with config.algo_scope(None):
        assert config.conv_algo() == L.ALGO_AUTO
    config.set_conv_algo("direct")
    try:
        with config.exact_products(True):  # an explicit algorithm choice is not overridden
            assert config.conv_algo() == L.ALGO_DIRECT
    finally:
        config.set_conv_algo("auto")
    assert config.conv_algo() == L.ALGO_AUTO


def test_exact_request_is_separate_from_the_algorithm_and_per_thread():
    """with set_conv_algo('mfma') a ReLU network in fp32 storage must still get exact products (the request rides on
    the base choice as MEDNET_ALGO_EXACT_BIT instead of being dropped), a backward replays base + request, and a scope opened in
    one thread is invisible to another (autograd's worker thread, or a second model driven from a second thread)."""
    import threading
    from mednet_hip import _lib as L, config
    config.set_conv_algo("mfma")
    try:
        assert config.conv_algo() == L.ALGO_MFMA
        with config.exact_products(True):
            assert config.conv_algo() == (L.ALGO_MFMA | L.ALGO_EXACT_BIT)
            captured = config.conv_algo()
            with config.algo_scope(L.ALGO_MFMA):  # replaying a forward that ran WITHOUT the request
                assert config.conv_algo() == L.ALGO_MFMA
        with config.algo_scope(captured):  # ... and one that ran with it, from outside the scope
            assert config.conv_algo() == (L.ALGO_MFMA | L.ALGO_EXACT_BIT)
        assert config.conv_algo() == L.ALGO_MFMA
    finally:
        config.set_conv_algo("auto")
    seen = []
    with config.exact_products(True):
        t = threading.Thread(target=lambda: seen.append(config.conv_algo()))
        t.start()
        t.join()
        assert config.conv_algo() == L.ALGO_EXACT
    assert seen == [L.ALGO_AUTO]


def test_optimizer_and_scaler_state_round_trip():
    """FlatAdam.load_state_dict restores the hyper-parameters it saved and refuses to resume a scaled run without the
    scaler's state; LossScaler.load_state_dict accepts the 4-entry state of earlier builds (new counters start at 0)."""
    from mednet_hip.train import FlatAdam, FlatParams, LossScaler
    lin = torch.nn.Linear(8, 8)
    flat = FlatParams(lin)
    opt = FlatAdam(flat, lr=3e-4, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.01)
    opt.t = 7
    sd = opt.state_dict()
    opt2 = FlatAdam(FlatParams(torch.nn.Linear(8, 8)), lr=1e-3)
    opt2.load_state_dict(sd)
    assert (opt2.lr, opt2.betas, opt2.eps, opt2.wd, opt2.t) == (3e-4, (0.8, 0.95), 1e-6, 0.01, 7)
    sc = LossScaler("cpu")
    with pytest.raises(KeyError):
        opt2.load_state_dict(sd, scaler=sc)  # saved without a scaler: resuming WITH one must not silently restart at 65536
    sc.load_state_dict({"state": torch.tensor([1024.0, 5.0, 40.0, 0.0]), "growth_factor": 2.0, "backoff_factor": 0.5,
                        "growth_interval": 100})
    assert sc.state.tolist() == [1024.0, 5.0, 40.0, 0.0, 0.0, 0.0, 0.0, 0.0] and sc.growth_interval == 100
    with pytest.raises(ValueError):
        sc.load_state_dict({"state": torch.zeros(9), "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 100})


def test_algo_mfma_is_satisfied_by_the_fp32_mode_matrix_core_kernels():
    """include/mednet_hip.h: MEDNET_ALGO_MFMA = "a matrix-core path is required"; in fp32 storage that is the split-bf16
    contraction, with MEDNET_ALGO_EXACT_BIT the fp32 matrix instruction.  Until round 4 the C side rejected both (its gate only
    knew the 16-bit kernels: ADVICE r4).  Host-only: without a device the call fails where it prepares the LAUNCH (MEDNET_E_HIP,
    naming the kernel it chose), not at the algorithm gate (MEDNET_E_UNSUPPORTED)."""
    from mednet_hip import _lib as L
    lib = L.lib()
    if lib.mednet_device_ok():
        pytest.skip("host-logic check: needs the no-device error path")
    chosen = {}
    for algo in (L.ALGO_AUTO, L.ALGO_MFMA, L.ALGO_EXACT, L.ALGO_MFMA | 4):
        rc = lib.mednet_conv3d_fwd(None, None, None, None, 1, 8, 8, 16, 32, 32, 3, L.F32, L.NDHWC, L.F32, L.NDHWC, 0, algo, None, None)
        msg = lib.mednet_last_error().decode()
        assert rc == -4 and "does not take" not in msg, (algo, rc, msg)
        chosen[algo] = msg.split(":")[0]
    assert chosen[L.ALGO_MFMA] == chosen[L.ALGO_AUTO] == "conv_x3"                    # split-bf16 contraction
    assert chosen[L.ALGO_MFMA | 4] == chosen[L.ALGO_EXACT] == "conv_f32_mfma"         # exact fp32 products
    # the 16-bit gate is unchanged: a channel count the matrix-core kernels do not take is still refused under ALGO_MFMA
    rc = lib.mednet_conv3d_fwd(None, None, None, None, 1, 8, 8, 16, 12, 20, 3, L.BF16, L.NDHWC, L.BF16, L.NDHWC, 0, L.ALGO_MFMA, None, None)
    assert rc == -5 and "does not take" in lib.mednet_last_error().decode()
    # and the weight-gradient plan is an argument: a negative workgroup count is a shape error before anything else happens
    rc = lib.mednet_conv3d_wgrad(None, None, None, None, 1, 8, 8, 16, 32, 32, 3, L.BF16, L.NDHWC, L.BF16, L.NDHWC, L.ALGO_AUTO, -1, None, 0, None)
    assert rc == -1 and "workgroups" in lib.mednet_last_error().decode()
    assert lib.mednet_get_option(b"wgrad_wgs", -7) == -7 and lib.mednet_abi_version() == 3


def test_fused_landmark_head_and_first_layer_entry_points_answer_without_a_device():
    """The round-5 entry points' host side: which shapes the matrix-core landmark head (head_mfma.hip) and the first layer's fused
    GroupNorm-backward + weight gradient take, their workspace / row counts, and argument errors that come before any launch."""
    from mednet_hip import _lib as L
    lib = L.lib()
    sp = 128 ** 3
    # landmarks.py:71-75: 16 heat maps + 2 classes on 32 features, either 16-bit type; not fp32 storage, not other widths
    assert lib.mednet_head_landmark_supported(32, 16, 2, L.BF16, sp) == 1 and lib.mednet_head_landmark_supported(32, 16, 2, L.F16, sp) == 1
    assert lib.mednet_head_landmark_supported(32, 16, 2, L.F32, sp) == 0
    assert lib.mednet_head_landmark_supported(64, 16, 2, L.BF16, sp) == 0
    assert lib.mednet_head_landmark_supported(32, 17, 2, L.BF16, sp) == 0 and lib.mednet_head_landmark_supported(32, 16, 5, L.BF16, sp) == 0
    assert lib.mednet_head_landmark_supported(32, 1, 1, L.BF16, 64) == 1 and lib.mednet_head_landmark_supported(32, 1, 1, L.BF16, 66) == 0
    rows = lib.mednet_head_landmark_gn_rows(sp)
    assert rows == (sp // 128 + 63) // 64 == 256 and lib.mednet_head_landmark_gn_rows(4) == 1
    assert lib.mednet_head_landmark_ws_bytes(4, sp, 16, 2) >= 4 * rows * 32 * 33 * 4
    rc = lib.mednet_head_landmark_fwd(None, None, None, None, 0, None, 0, None, None, None, None, None, None, 4, sp, 32, 16, 2, 0, 1e-5, 0,
                                      L.NO_IGNORE, L.BF16, None, 0, None)
    assert rc == -1 and "head_landmark_fwd" in lib.mednet_last_error().decode()
    # the head family's other entries share their checks: each answers null pointers with MEDNET_E_SHAPE under its own name (codes as
    # the library returned them before the entries were put on one implementation)
    lm_dims = (4, sp, 32, 16, 2, 0)  # n, spatial, cin, nh, ncls, kind
    lm_tail = (1e-5, 0, L.NO_IGNORE, L.BF16, None, 0, None)  # eps, sigmoid, ignore_index, dtype, ws, ws_bytes, stream
    seg_dims = (4, sp, 32, 14)
    nulls = {
        "head_landmark_bwd": lambda: lib.mednet_head_landmark_bwd(None, None, None, None, 0, None, 0, *[None] * 7, 0, None, None, None,
                                                                  *lm_dims, *lm_tail),
        "head_landmark_cls_fwd": lambda: lib.mednet_head_landmark_cls_fwd(None, None, None, None, 0, None, 0, *[None] * 7, *lm_dims,
                                                                          L.CLASS_CE, *lm_tail),
        "head_landmark_cls_bwd": lambda: lib.mednet_head_landmark_cls_bwd(None, None, None, None, 0, None, 0, *[None] * 7, 0, None, None,
                                                                          None, *lm_dims, L.CLASS_CE, *lm_tail),
        "head_seg_fwd": lambda: lib.mednet_head_seg_fwd(None, None, None, None, 0, *[None] * 4, *seg_dims, L.CLASS_DICE, *lm_tail),
        "head_seg_bwd": lambda: lib.mednet_head_seg_bwd(None, None, None, None, 0, *[None] * 5, 0, None, None, None, *seg_dims,
                                                        L.CLASS_CE, *lm_tail),
    }
    for name, call in nulls.items():
        rc = call()
        assert rc == -1 and lib.mednet_last_error().decode().startswith(name + ":"), (name, rc, lib.mednet_last_error())
    # Dice through the _cls_ entry: the same checks under the _cls_ name
    rc = lib.mednet_head_landmark_cls_fwd(None, None, None, None, 0, None, 0, *[None] * 7, *lm_dims, L.CLASS_DICE, *lm_tail)
    assert rc == -1 and lib.mednet_last_error().decode().startswith("head_landmark_cls_fwd:")
    # cross-entropy is a softmax form; dice_metric of a Dice forward takes no ignore_index: refused before the pointers are looked at
    import ctypes as C
    metric = C.c_float()
    rc = lib.mednet_head_landmark_cls_fwd(None, None, None, None, 0, None, 0, *[None] * 7, *lm_dims, L.CLASS_CE, 1e-5, 1, L.NO_IGNORE,
                                          L.BF16, None, 0, None)
    assert rc == -5 and "head_landmark_cls_fwd" in lib.mednet_last_error().decode()
    rc = lib.mednet_head_landmark_cls_fwd(None, None, None, None, 0, None, 0, *[None] * 6, C.addressof(metric), *lm_dims, L.CLASS_DICE,
                                          1e-5, 0, 1, L.BF16, None, 0, None)
    assert rc == -5 and "head_landmark_cls_fwd" in lib.mednet_last_error().decode()
    # first layer (Cin = 1): 16 / 32 / 64 output channels, 16-bit gradients, patch fp32 or the same 16-bit type
    for dt in (L.BF16, L.F16):
        assert all(lib.mednet_conv3d_wgrad_c1_gn_supported(c, L.F32, dt) == 1 for c in (16, 32, 64))
        assert lib.mednet_conv3d_wgrad_c1_gn_supported(32, dt, dt) == 1 and lib.mednet_conv3d_wgrad_c1_gn_supported(48, L.F32, dt) == 0
    assert lib.mednet_conv3d_wgrad_c1_gn_supported(32, L.F32, L.F32) == 0 and lib.mednet_conv3d_wgrad_c1_gn_supported(32, L.BF16, L.F16) == 0
    rc = lib.mednet_conv3d_wgrad_c1_gn(None, None, None, None, None, None, 1, 8, 8, 16, 32, 0, L.F32, L.BF16, None, 0, None)
    assert rc == -1 and "conv3d_wgrad_c1_gn" in lib.mednet_last_error().decode()
    rc = lib.mednet_gn_bwd_coefficients(None, None, None, 0, None, None, None, 1, 64, 32, 8, None, 0, None)
    assert rc == -1 and "gn_bwd_coefficients" in lib.mednet_last_error().decode()


def test_normalisation_entries_refuse_what_they_refused_in_the_same_order(golden_dir):
    """tools/norm_refusals.py: every extern "C" entry of csrc/norm_act.hip (and the Adam entries of csrc/optim.hip) with argument sets that trip each of its checks in turn
    (null pointers, bad dtype, C % groups, C / vec > 256, a workspace one byte short, two violations at once, the options that
    switch a fused form off) -- all refused before any launch, no device needed.  tests/golden/norm_refusals.jsonl is the table
    the library printed BEFORE the entries were put on one host path (GnPlan, launch_gn_*, gn_bwd_coefs): return code and
    message of every case are frozen, so a reordered or reworded check shows."""
    import importlib.util
    import json
    import os
    from mednet_hip import _lib as L
    spec = importlib.util.spec_from_file_location("norm_refusals", os.path.join(os.path.dirname(golden_dir), "..", "tools", "norm_refusals.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(golden_dir, "norm_refusals.jsonl")) as f:
        want = [json.loads(line) for line in f]
    got = tool.run(L.lib())
    assert len(want) == 360 and [(r["entry"], r["case"]) for r in got] == [(r["entry"], r["case"]) for r in want]
    for g, w in zip(got, want):
        assert g == w, (g, w)
    assert all(r["rc"] < 0 for r in want if r["error"])  # (a refusal each: nothing in the table reached a launch)


def test_convolution_entries_refuse_and_answer_what_they_did_before_their_host_code_was_shared(golden_dir):
    """tools/conv_routes.py: every conv-family extern "C" entry of csrc/api.hip with argument sets that trip each of its checks in
    turn (bad dtype, ksize = 2, a zero extent, null gn_* pointers, negative workgroups, a workspace one byte short for the bias
    gradient, MEDNET_ALGO_MFMA on shapes the matrix-core path does not take, an activation out of range, two at once, the options
    that switch a fused form off) -- all refused before any launch -- and every entry that answers a number (rows, chunks, plans,
    workspace and pack sizes, the *_supported predicates) at points of volumes x channel pairs x storage types x algo, with
    assume_cus = 256, no device needed.  tests/golden/conv_routes.jsonl is the table the library printed BEFORE the family's host code was put
    on one launch idiom, one variant table and shared route predicates: every code, message and number is frozen."""
    import importlib.util
    import json
    import os
    from mednet_hip import _lib as L
    spec = importlib.util.spec_from_file_location("conv_routes", os.path.join(os.path.dirname(golden_dir), "..", "tools", "conv_routes.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(golden_dir, "conv_routes.jsonl")) as f:
        want = [json.loads(line) for line in f]
    got = tool.run(L.lib())
    assert len(want) == 375 and [r["case"] for r in got] == [r["case"] for r in want]
    for g, w in zip(got, want):
        assert g == w, (g, w)
    refused = [r for r in want if "error" in r]
    assert len(refused) == 231 and all(r["rc"] in (-1, -2, -3, -5) for r in refused)  # (a check's refusal each: nothing reached a launch)
    plans = [a for r in want if r["case"].startswith("plan") for a in r["answers"].items()]
    kinds = lambda name: {p[0] for k, v in plans if k.startswith(name) for p in v if isinstance(p, list)}  # noqa: E731
    assert kinds("stats_plan") == {2, 3, 4, 5, 6, 7}  # (every kind of the forward / data-gradient family's plan occurs)
    assert kinds("wgrad_plan") == {2, 4}


def test_fused_head_nodes_step_aside_for_hooks_on_the_bypassed_calls():
    """The fused head + loss nodes (train.SegmentationStep._head_loss, LandmarkStep._head_losses) call forward_features() and never
    final_conv: a forward hook / pre-hook on the model or on final_conv would not fire, so the steps take the stock model(inputs)
    path then.  Hooks on encoder / decoder children fire either way and do not switch the fusion off."""
    from mednet_hip.train import _call_is_hooked
    m = HM.ResidualUNet3D(1, 4, False, f_maps=[16, 32])
    fc = m.final_conv
    assert not _call_is_hooked(m, fc)
    h = m.encoders[0].register_forward_hook(lambda *a: None)  # a child the fused form still calls through __call__
    assert not _call_is_hooked(m, fc)
    h.remove()
    for mod, reg in ((fc, "register_forward_hook"), (fc, "register_forward_pre_hook"), (m, "register_forward_hook"),
                     (m, "register_forward_pre_hook")):
        h = getattr(mod, reg)(lambda *a: None)
        assert _call_is_hooked(m, fc), reg
        h.remove()
        assert not _call_is_hooked(m, fc)
    g = torch.nn.modules.module.register_module_forward_hook(lambda *a: None)
    try:
        assert _call_is_hooked(m, fc)
    finally:
        g.remove()
    assert not _call_is_hooked(m, fc)


def test_loss_module_keeps_product_and_restated_reference_code_apart():
    """mednet_hip/unet/loss.py defines the fused HIP losses; the reference's unused loss zoo lives in loss_compat.py and is only
    re-exported (VERDICT r5 housekeeping), and every public name of the reference's module still resolves through the alias."""
    import midasmednet.unet.loss as ML
    from mednet_hip.unet import loss_compat as HCOMP
    for name in ("DiceLoss", "dice_metric", "CrossEntropyLoss", "HeatmapRegressionLoss", "LandmarkLoss"):
        assert getattr(HL, name).__module__ == "mednet_hip.unet.loss", name
    for name in ("flatten", "expand_as_one_hot", "compute_per_channel_dice", "CELoss", "WeightedCrossEntropyLoss", "BCELossWrapper",
                 "PixelWiseCrossEntropyLoss"):
        assert getattr(HL, name) is getattr(HCOMP, name) and getattr(ML, name) is getattr(HCOMP, name), name
        assert getattr(HCOMP, name).__module__ == "mednet_hip.unet.loss_compat", name


def test_lean_pack_bookkeeping_decisions():
    """MEDNET_PACK_HIGH_ONLY (train.BatchedRepack): which layers may run on packs whose fp32 / low images are stale, and which calls
    must re-pack first -- the host-side rules of nn._PackedWeightMixin (mednet_hip.h: only the 16-bit matrix-core path reads nothing
    else).  Decisions only; no device."""
    import mednet_hip
    from mednet_hip import nn as hnn
    conv = hnn.Conv3d(32, 64, 3, bias=False)
    assert conv._lean_layer_ok()
    assert not hnn.Conv3d(32, 64, 3, bias=True)._lean_layer_ok()              # conv_mfma_supported: no bias
    assert not hnn.Conv3d(1, 32, 3, bias=False)._lean_layer_ok()              # first layer: reads the fp32 image
    assert not hnn.Conv3d(32, 4, 1, planar_output=True)._lean_layer_ok()      # 1x1x1 head
    assert not hnn.Conv3d(24, 32, 3, bias=False)._lean_layer_ok()
    assert hnn.ConvTranspose3d(64, 32)._lean_layer_ok()
    assert not hnn.ConvTranspose3d(48, 16)._lean_layer_ok()                   # matrix-core ConvTranspose kernels: channels in 32s
    x16 = torch.empty(1, 32, 8, 8, 8, dtype=torch.bfloat16, device="meta")
    x32 = torch.empty(1, 32, 8, 8, 8, dtype=torch.float32, device="meta")
    big = torch.empty(1, 32, 400, 400, 400, dtype=torch.bfloat16, device="meta")  # 4.1 GB per sample at 32 channels
    with mednet_hip.precision("bf16"):
        assert conv._lean_call_ok(x16, False) and conv._lean_call_ok(None, False)
        assert not conv._lean_call_ok(x32, False)     # fp32 tensors in a 16-bit mode: split-bf16 kernels, low images
        assert conv._lean_call_ok(x32, True)          # ... unless the op casts its input first (ResBlockFn, ConvTranspose3d)
        assert not conv._lean_call_ok(big, False)     # conv_mfma_fits: direct kernels
        assert not conv._lean_call_ok(x16.to(torch.float16), False)
        mednet_hip.set_conv_algo("direct")
        try:
            assert not conv._lean_call_ok(x16, False)
        finally:
            mednet_hip.set_conv_algo("auto")
        mednet_hip.set_conv_algo("mfma")
        try:
            assert conv._lean_call_ok(x16, False)
        finally:
            mednet_hip.set_conv_algo("auto")
    with mednet_hip.precision("fp32"):
        assert not conv._lean_call_ok(x32, False)     # fp32 storage: every image is read
    with mednet_hip.precision("fp16x2"):
        assert conv._lean_call_ok(x16.to(torch.float16), False)
