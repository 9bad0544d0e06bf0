"""Host logic of the Dice + cross-entropy class loss, without a GPU: the loss module, its re-export, what the training and validation
steps construct for "DICE_CE" and that "DICE" / "CE" construct what they did."""
import pytest
import torch

from mednet_hip import ops
from mednet_hip.unet import loss as HL
from mednet_hip.unet import model as HM


def test_loss_module_and_its_re_export():
    import midasmednet.unet.loss as ML
    assert HL.DiceCELoss.__module__ == "mednet_hip.unet.loss" and ML.DiceCELoss is HL.DiceCELoss
    crit = HL.DiceCELoss()
    assert crit.epsilon == 1e-5 and crit.weight is None
    w = torch.tensor([0.05, 1.0])
    crit = HL.DiceCELoss(epsilon=1e-3, weight=w)
    assert crit.epsilon == 1e-3 and torch.equal(crit.weight, w) and "weight" in dict(crit.named_buffers())
    with pytest.raises(ValueError):  # there is no sigmoid form
        HL.DiceCELoss(sigmoid_normalization=True)
    with pytest.raises(TypeError):   # ... and no ignore_index
        HL.DiceCELoss(ignore_index=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(torch.zeros(1, 2, 2, 2, 2), torch.zeros(1, 2, 2, 2, dtype=torch.int64))
    assert callable(ops.dice_ce_loss) and callable(ops.head_dice_ce) and callable(ops.head_dice_ce_supported)


def test_class_kind_names():
    from mednet_hip import _lib as L
    assert (ops._class_kind("DICE"), ops._class_kind("CE"), ops._class_kind("DICE_CE")) == (L.CLASS_DICE, L.CLASS_CE, L.CLASS_DICE_CE) == (0, 1, 2)
    with pytest.raises(ValueError):
        ops._class_kind("DICE+CE")
    assert ops._class_operands(L.CLASS_DICE_CE, 9, False, None, "t") == (19, L.NO_IGNORE)
    assert ops._class_operands(L.CLASS_DICE, 9, True, None, "t") == (18, L.NO_IGNORE)
    assert ops._class_operands(L.CLASS_CE, 9, False, None, "t") == (18, -100)
    assert ops._class_operands(L.CLASS_CE, 9, False, 3, "t") == (18, 3)
    for sigmoid, ignore in ((True, None), (False, -100), (False, 2)):
        with pytest.raises(ValueError):
            ops._class_operands(L.CLASS_DICE_CE, 9, sigmoid, ignore, "t")


def test_segmentation_steps_accept_the_new_string_and_keep_the_old_ones():
    from mednet_hip.train import SegmentationStep, SegmentationValidation
    w = [0.05, 1.0, 1.0, 1.0]
    for make in (lambda m, k: SegmentationStep(m, loss_weight=w, loss=k), lambda m, k: SegmentationValidation(m, loss_weight=w, loss=k)):
        for kind, cls in (("DICE", HL.DiceLoss), ("CE", HL.CrossEntropyLoss), ("DICE_CE", HL.DiceCELoss)):
            step = make(HM.ResidualUNet3D(1, 4, False, f_maps=[8, 16]), kind)
            assert type(step.loss) is cls, kind
            assert torch.equal(step.loss.weight, torch.tensor(w))
    dice = SegmentationStep(HM.ResidualUNet3D(1, 4, False, f_maps=[8, 16]), loss="DICE").loss
    assert (dice.epsilon, dice.weight, dice.ignore_index, dice.sigmoid_normalization, dice.skip_last_target) == (1e-5, None, None, False, False)
    ce = SegmentationStep(HM.ResidualUNet3D(1, 4, False, f_maps=[8, 16]), loss="CE").loss
    assert (ce.weight, ce.ignore_index) == (None, -100)
    both = SegmentationStep(HM.ResidualUNet3D(1, 4, False, f_maps=[8, 16])).loss  # the default is still Dice
    assert type(both) is HL.DiceLoss


def test_landmark_steps_accept_the_new_string_and_keep_the_old_ones():
    from mednet_hip.train import LandmarkStep, LandmarkValidation
    regw = [0.015, 0.02, 0.001]
    for make in (LandmarkStep, LandmarkValidation):
        for kind, cls in (("DICE", HL.DiceLoss), ("CE", HL.CrossEntropyLoss), ("DICE_CE", HL.DiceCELoss)):
            step = make(HM.ResidualUNet3D(1, 5, False, f_maps=[8, 16]), class_weight=[0.05, 1.0], regression_weight=regw, class_loss=kind)
            assert type(step.loss_class) is cls and step.class_loss == kind
            assert torch.equal(step.loss_class.weight, torch.tensor([0.05, 1.0]))
            assert step.loss_reg.kind == "L2"
        with pytest.raises(ValueError):
            make(HM.ResidualUNet3D(1, 5, False, f_maps=[8, 16]), class_weight=[0.05, 1.0], regression_weight=regw, class_loss="DICECE")
