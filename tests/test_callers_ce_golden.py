"""tests/golden/callers_ce.npz -- recorded by tools/make_golden.py from the reference's own callers (SegmentationNet(loss='CE'),
LandmarkNet(loss_class='CE' / 'DICE'): training_step, validation_step, validation_epoch_end) after they agreed bit for bit with the
oracle -- against the oracle composition recomputed here on the CPU.  No GPU needed."""
import os

import numpy as np
import torch
import torch.nn as nn

from oracle import ref_cpu as O

# (the cases of tools/make_golden.py caller_ce_cases; tests/test_gpu_ce_heads.py runs them through the HIP path)
CE_SEG = dict(ctor=(1, 2, [32, 64]), shape=(16, 16, 16), weight=[0.05, 1.0], seed=1240, val_seeds=(640, 641))
CE_LDMK = dict(ctor=(1, 5, [32, 64]), shape=(16, 16, 16), weight=[0.05, 1.0], regw=[0.015, 0.02, 0.001], seed=4330,
               val_seeds=(740, 741))
LDMK_KEYS = ["val_loss", "val_class_loss", "val_regression_loss", "val_dice0", "val_dice1"]


def ldmk_validation_step(model, loss_class, regw, batch):
    """LandmarkNet.validation_step (landmarks.py:136-162) without the sample logging: O.landmark_loss + O.dice_metric."""
    x = batch["data"].float()
    hm = batch["label"][:, :-1, ...].float()
    nh = hm.shape[1]
    y = batch["label"][:, -1, ...].long()
    with torch.no_grad():
        out = model(x)
        tot, cl, rg = O.landmark_loss(out[:, nh:], out[:, :nh], y, hm, loss_class, nn.MSELoss(), regw)
        dm = O.dice_metric(out[:, nh:], y)
    res = {"val_loss": tot, "val_class_loss": cl, "val_regression_loss": rg}
    for c in range(out.shape[1] - nh):
        res[f"val_dice{c}"] = dm[c]
    return res


def _close(a, b, what, rtol=1e-5):
    a, b = float(a), float(b)
    assert abs(a - b) <= rtol * max(1.0, abs(b)), (what, a, b)


def test_segmentation_ce_caller_fixture_against_the_oracle(golden_dir):
    """SegmentationNet(loss='CE', loss_weight=[0.05, 1.0]) (segmentation.py:43-49, 58-65, 94-118): training loss, two
    validation_steps and validation_epoch_end."""
    rec = np.load(os.path.join(golden_dir, "callers_ce.npz"))
    cin, cout, fm = CE_SEG["ctor"]
    crit = nn.CrossEntropyLoss(weight=torch.tensor(CE_SEG["weight"]))
    ora = O.keyed_init_(O.ResidualUNet3D(cin, cout, False, f_maps=fm))
    batch = O.synthetic_batch(2, 1, CE_SEG["shape"], cout, 0, seed=CE_SEG["seed"])
    _close(O.seg_training_step(ora, crit, batch), rec["seg.loss"], "seg.loss")
    ora.eval()
    outs = [O.seg_validation_step(ora, crit, O.synthetic_batch(2, 1, CE_SEG["shape"], cout, 0, seed=s)) for s in CE_SEG["val_seeds"]]
    for i, o in enumerate(outs):
        assert list(o.keys()) == ["val_loss", "val_dice0", "val_dice1"]
        for k, v in o.items():
            _close(v, rec[f"seg.val{i}.{k}"], f"seg.val{i}.{k}")
    for k, v in O.validation_epoch_end(outs).items():
        _close(v, rec["seg.val_end." + k], "seg.val_end." + k)


def test_landmark_ce_caller_fixture_against_the_oracle(golden_dir):
    """LandmarkNet(loss_class='CE') training_step's three losses with L2 and L1 regression (landmarks.py:43-56, 66-83, 125-134),
    and validation_step x 2 + validation_epoch_end (landmarks.py:136-174) for loss_class DICE and CE."""
    rec = np.load(os.path.join(golden_dir, "callers_ce.npz"))
    cin, cout, fm = CE_LDMK["ctor"]
    w = torch.tensor(CE_LDMK["weight"])
    regw = CE_LDMK["regw"]
    nh = len(regw)
    batch = O.synthetic_batch(2, 1, CE_LDMK["shape"], cout - nh, nh, seed=CE_LDMK["seed"])
    for kind, crit in (("L2", nn.MSELoss()), ("L1", nn.L1Loss())):
        ora = O.keyed_init_(O.ResidualUNet3D(cin, cout, False, f_maps=fm))
        tot, cl, rg = O.ldmk_training_step(ora, nn.CrossEntropyLoss(weight=w), crit, regw, batch)
        for name, v in (("loss", tot), ("class_loss", cl), ("regression_loss", rg)):
            _close(v, rec[f"ldmk.{kind}.{name}"], f"ldmk.{kind}.{name}")
    vb = [O.synthetic_batch(2, 1, CE_LDMK["shape"], cout - nh, nh, seed=s) for s in CE_LDMK["val_seeds"]]
    for lc in ("DICE", "CE"):
        ora = O.keyed_init_(O.ResidualUNet3D(cin, cout, False, f_maps=fm)).eval()
        crit = O.DiceLoss(weight=w) if lc == "DICE" else nn.CrossEntropyLoss(weight=w)
        outs = [ldmk_validation_step(ora, crit, regw, b) for b in vb]
        for i, o in enumerate(outs):
            assert list(o.keys()) == LDMK_KEYS
            for k, v in o.items():
                _close(v, rec[f"ldmk_val.{lc}.{i}.{k}"], f"ldmk_val.{lc}.{i}.{k}")
        end = O.validation_epoch_end(outs)
        assert list(end.keys()) == LDMK_KEYS
        for k, v in end.items():
            _close(v, rec[f"ldmk_val_end.{lc}.{k}"], f"ldmk_val_end.{lc}.{k}")
    # the two class losses are different numbers on the same network and batches (the fixture records both, not one twice)
    assert abs(float(rec["ldmk_val_end.DICE.val_class_loss"]) - float(rec["ldmk_val_end.CE.val_class_loss"])) > 1e-3
