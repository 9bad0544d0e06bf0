"""mednet_hip._volume.like_volume on the CPU: what it refuses, with the caller's words, and what it passes."""
import pytest
import torch

from mednet_hip._volume import like_volume


def test_like_volume_refuses_dtype_shape_and_layout_in_the_callers_words():
    ref = torch.zeros((3, 4, 5), dtype=torch.uint8)
    good = torch.empty((3, 4, 5), dtype=torch.float32)
    assert like_volume(good, ref, torch.float32, "who", "what") is good
    for bad in (good.double(), torch.empty((3, 4, 6)), torch.empty((3, 5, 4)).transpose(1, 2), torch.empty((3, 4, 5), device="meta")):
        with pytest.raises(ValueError) as e:
            like_volume(bad, ref, torch.float32, "edt_squared", "out must be a contiguous fp32 volume of the seed's shape on its device")
        assert str(e.value) == "edt_squared: out must be a contiguous fp32 volume of the seed's shape on its device"
