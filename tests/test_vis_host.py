"""Host-side rules of mednet_hip.vis (no GPU): the make_grid layout the reference's plots rely on, vis_logimages' slice rule, and
the argument checks / workspace query of mednet_sample_panels, which answer before anything is launched."""
import numpy as np
import pytest
import torch

from mednet_hip import _lib as L
from mednet_hip import vis


def test_grid_of_two_cells_in_one_row():
    """vis_loglabels: make_grid of [pred, label] with the default nrow=8, padding=2, pad_value=0."""
    cells = np.arange(1, 25, dtype=np.uint8).reshape(2, 3, 4)
    want = np.zeros((3 + 4, 2 * (4 + 2) + 2), dtype=np.uint8)
    want[2:5, 2:6] = cells[0]
    want[2:5, 8:12] = cells[1]
    got = vis.make_grid2d(torch.from_numpy(cells))
    assert got.dtype == torch.uint8
    np.testing.assert_array_equal(got.numpy(), want)
    assert vis.grid_shape(2, 3, 4) == (7, 14, 2, 1)


def test_grid_of_six_cells_three_per_row():
    """vis_logheatmaps: 2 * num_heatmaps cells, nrow = num_heatmaps."""
    cells = (np.arange(6 * 3 * 4, dtype=np.float32) + 1).reshape(6, 3, 4)
    want = np.zeros((2 * (3 + 2) + 2, 3 * (4 + 2) + 2), dtype=np.float32)
    for k, (r0, c0) in enumerate([(2, 2), (2, 8), (2, 14), (7, 2), (7, 8), (7, 14)]):
        want[r0:r0 + 3, c0:c0 + 4] = cells[k]
    np.testing.assert_array_equal(vis.make_grid2d(torch.from_numpy(cells), nrow=3).numpy(), want)
    # a last row that is not full stays at the pad value
    five = vis.make_grid2d(torch.from_numpy(cells[:5]), nrow=3).numpy()
    want[7:10, 14:18] = 0
    np.testing.assert_array_equal(five, want)


@pytest.mark.parametrize("h,count", [(8, 8), (12, 6), (16, 6), (128, 6)])
def test_slice_rule_is_the_literal_range(h, count):
    idx = vis.slice_indices(h, 5)
    assert idx == list(range(0, h, h // 5)) and len(idx) == count


def test_fewer_slices_than_steps_raise():
    with pytest.raises(ValueError):
        vis.slice_indices(4, 5)


def test_cpu_tensors_are_refused():
    z = torch.zeros(1, 2, 5, 5, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vis.sample_panels(z, torch.zeros(1, 1, 5, 5, 5, dtype=torch.uint8), z[:, :1])


def test_workspace_query_and_argument_checks_need_no_gpu():
    lib = L.lib()
    # config 2's volume: 3 jobs x 16 segments x 128 x 128 floats for the strided axes, nothing for the contiguous one
    assert lib.mednet_sample_panels_ws_bytes(128, 128, 128, 0, 1) == 3 * 16 * 128 * 128 * 4
    assert lib.mednet_sample_panels_ws_bytes(128, 128, 128, 3, 0) == 9 * 16 * 128 * 128 * 4
    assert lib.mednet_sample_panels_ws_bytes(128, 128, 128, 3, 2) == 0
    assert lib.mednet_sample_panels_ws_bytes(5, 7, 9, 0, 1) == 3 * 7 * 5 * 9 * 4  # never more segments than reduced elements

    def call(axis=1, mode=L.MIP_MEAN, ncls=2, label_dtype=L.U8, pred=16, ws_bytes=1 << 20, d=5):
        # (non-null dummies: every case below is refused before a pointer is used)
        return lib.mednet_sample_panels(16, 125, 0, ncls, 16, label_dtype, None, L.U8, 16, pred, 16, 16, None, None, d, 5, 5, axis,
                                        mode, 16, ws_bytes, None)
    for kw, code, text in ((dict(axis=3), -1, "mip axis 3"), (dict(mode=7), -5, "image mode 7"), (dict(ncls=0), -1, "classes"),
                           (dict(label_dtype=L.F32), -2, "uint8 or int64 labels"), (dict(d=0), -1, "bad volume"),
                           (dict(ws_bytes=64), -3, "workspace of 64 bytes")):
        assert call(**kw) == code, kw
        assert text in lib.mednet_last_error().decode(), (kw, lib.mednet_last_error())
