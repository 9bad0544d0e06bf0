"""tests/golden/dice_ce.npz -- the reference's DiceLoss(weight) + torch.nn.CrossEntropyLoss(weight), captured by tools/make_golden.py
(--only dice_ce) -- against the oracle's composition O.DiceLoss + F.cross_entropy, at the bounds test_oracle_golden.py holds the two
single losses of losses.npz to.  Runs without the reference."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O
from test_oracle_golden import RTOL

CLASSES = (2, 4, 14)
N, SHAPE = 2, (6, 5, 4)


def dice_ce_weights(c):
    return torch.tensor([0.05] + [0.6 + 0.1 * (k % 7) for k in range(1, c)])


def test_fixture_holds_the_cases_of_the_issue(golden_dir):
    path = os.path.join(golden_dir, "dice_ce.npz")
    assert os.path.getsize(path) < 100 * 1024
    rec = np.load(path)
    for c in CLASSES:
        assert rec[f"c{c}.logits"].shape == (N, c) + SHAPE and rec[f"c{c}.logits"].dtype == np.float32
        assert rec[f"c{c}.labels"].shape == (N,) + SHAPE and int(rec[f"c{c}.labels"].max()) == c - 1
        np.testing.assert_array_equal(rec[f"c{c}.weight"], dice_ce_weights(c).numpy())
        for wtag in ("plain", "weight"):
            for name in ("loss", "dice", "ce"):
                assert rec[f"c{c}.{wtag}.{name}"].shape == ()
            assert rec[f"c{c}.{wtag}.dlogits"].shape == (N, c) + SHAPE
            # one rounded fp32 add of the two terms
            assert np.float32(rec[f"c{c}.{wtag}.dice"]) + np.float32(rec[f"c{c}.{wtag}.ce"]) == np.float32(rec[f"c{c}.{wtag}.loss"])


def test_oracle_composition_reproduces_the_fixture(golden_dir):
    rec = np.load(os.path.join(golden_dir, "dice_ce.npz"))
    for c in CLASSES:
        y = torch.from_numpy(rec[f"c{c}.labels"]).long()
        for wtag, w in (("plain", None), ("weight", torch.from_numpy(rec[f"c{c}.weight"]))):
            z = torch.from_numpy(rec[f"c{c}.logits"]).clone().requires_grad_(True)
            dice, ce = O.DiceLoss(weight=w)(z, y), F.cross_entropy(z, y, weight=w)
            (dice + ce).backward()
            tag = f"c{c}.{wtag}"
            for name, v in (("loss", dice + ce), ("dice", dice), ("ce", ce)):
                assert abs(float(v.detach()) - float(rec[f"{tag}.{name}"])) <= 1e-6, (tag, name)
            assert O.rel_l2(z.grad, rec[f"{tag}.dlogits"]) <= RTOL, tag
