"""tests/ds_util.py on the CPU: the fp64 restatement of the deep-supervision node passes its own checkers, and the checkers reject
each fault they are there for -- an off-by-one label pick, an averaged label, a double-rounded junction, a dropped d_pass."""
import numpy as np
import pytest
import torch

import ds_util as U
from gpu_util import half_round, rnd

KINDS = ["DICE", "CE", "DICE_CE"]
EPS = 2.0 ** -15   # (the GPU tests' allowance for the kernel's own arithmetic; the restatement itself needs none)


def _case(mode, ncls, s, lev=(4, 4, 8), cin=64, n=2):
    full = tuple(v << s for v in lev)
    tag = f"dsu{mode}{ncls}{s}"
    z = half_round(rnd(tag + "z", n, cin, *lev), mode)
    W, b = rnd(tag + "w", ncls, cin, scale=0.3), rnd(tag + "b", ncls)
    d_pass = half_round(rnd(tag + "p", n, cin, *lev, scale=0.05), mode)
    labels = U.random_labels(n, full, ncls)[:, -1]
    return z, W, b, labels, d_pass


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("s", [1, 2])
def test_the_restatement_passes_and_every_fault_is_rejected(mode, kind, s):
    z, W, b, labels, d_pass = _case(mode, 4, s)
    ref = U.head_ref(z, W, b, labels, s, kind, d_pass=d_pass, dloss=32.0, mode=mode)
    assert U.check_join(ref.stored, ref, mode, 0.0, "the restatement's own rounding") == 0.0
    U.check_loss(ref.loss, ref, 0.0, "the restatement's own loss")
    for fault in U.FAULTS:
        bad = U.head_ref(z, W, b, labels, s, kind, d_pass=d_pass, dloss=32.0, mode=mode, fault=fault)
        with pytest.raises(AssertionError):
            U.check_join(bad.stored, ref, mode, EPS, fault)
        if fault in ("pick_off_by_one", "averaged_label"):
            with pytest.raises(AssertionError):
                U.check_loss(bad.loss, ref, 1e-4, fault)


@pytest.mark.parametrize("ncls", [2, 4, 8, 16])
@pytest.mark.parametrize("s", [1, 2, 3])
def test_exact_pick_premise(ncls, s):
    """Zero features and weights, equal biases: p = 1 / ncls is dyadic, every Dice sum is a multiple of 1 / ncls far below 2^24
    steps (exact in fp32 in any order), the restatement's loss is exactly 1 - 1 / ncls, and every position a stray pick or an
    averaged label would read holds an out-of-range class."""
    lev = (4, 4, 8)
    lab = U.exact_pick_labels(2, lev, s, ncls)[:, -1]
    picked = U.pick(lab, s)
    vox = picked.numel()
    assert torch.equal(torch.bincount(picked.flatten().long(), minlength=ncls), torch.full((ncls,), vox // ncls))
    assert int((lab == U.OUTSIDE).sum()) == lab.numel() - vox
    assert bool((U.pick(lab, s, 1) == U.OUTSIDE).all()) and int(U.averaged(lab, s).min()) >= ncls
    z, W, b = torch.zeros(2, 64, *lev), torch.zeros(ncls, 64), torch.full((ncls,), 0.25)
    ref = U.head_ref(z, W, b, lab, s, "DICE", mode="bf16")
    p = torch.softmax(torch.full((ncls,), 0.25, dtype=torch.float32), 0)
    assert bool((p == 1.0 / ncls).all())
    assert 2 * vox < 2 ** 24                      # D_k = 2 V / ncls in steps of 1 / ncls
    assert ref.loss == 1.0 - 1.0 / ncls
    assert np.float32(ref.loss) == np.float32(1.0) - np.float32(1.0 / ncls)
