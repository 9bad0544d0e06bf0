"""Connected components of a uint8 class volume on the device (csrc/components.hip): the post-processing step
between inference and measurement, without the volume leaving HBM.

    comps = label_components(pred, cls=2, connectivity=26)       # pred uint8 D x H x W, e.g. GridPredictor(...)(vol)[-1]
    comps.labels, comps.count, comps.stats()                      # int32 volume, K, int64 [K, 11] table -- all on the device
    keep_largest(pred, classes=(1, 2, 3))                         # nnU-Net's default post-processing
    remove_small(pred, classes=(4,), min_volume=30.0, spacing=(3.0, 0.7, 0.7))
    fill_holes(pred, cls=1)
    pp = Postprocess(keep_largest=(1, 2), min_voxels={3: 10}, fill_holes=(1,))        # a callable for GridPredictor(postprocess=pp)

Definitions.  Foreground is `volume == cls` (`volume != cls` with invert); with cls=None every non-zero voxel is foreground and two
voxels are connected only if their values are equal, which labels every class of a multi-organ prediction at once.  connectivity 6,
18, 26 = neighbours that differ by 1 in at most 1, 2, 3 coordinates: scipy's generate_binary_structure(3, 1 | 2 | 3).  Components are
numbered 1 .. K in raster order (z, y, x; x fastest) of their first voxel -- exactly scipy.ndimage.label's numbering, so
`labels == scipy.ndimage.label(mask, structure)[0]` voxel for voxel.  Every result is an integer and a pure function of the input.

The table of `stats()` has one row per component (row id - 1): voxel count, zmin, zmax, ymin, ymax, xmin, xmax, sum z, sum y, sum x,
the component's value in the volume."""
from __future__ import annotations

import dataclasses

import torch

from . import _lib as L
from ._volume import like_volume, volume_u8

COUNT, ZMIN, ZMAX, YMIN, YMAX, XMIN, XMAX, SUM_Z, SUM_Y, SUM_X, VALUE = range(11)
COLUMNS = 11
_OUT = "out must be a contiguous uint8 volume of the input's shape on its device"


@dataclasses.dataclass
class Components:
    """A labelling: `labels` int32 D x H x W on the device (0 background, 1 .. count), `count` = K on the host, `volume` the uint8
    volume it was made from."""
    labels: torch.Tensor
    count: int
    volume: torch.Tensor
    _table: torch.Tensor = None

    def stats(self) -> torch.Tensor:
        """int64 [count, 11] on the device (module docstring gives the columns); computed once."""
        if self._table is None:
            d, h, w = self.volume.shape
            table = torch.empty((self.count, COLUMNS), dtype=torch.int64, device=self.volume.device)
            L.check(L.lib().mednet_cc_stats(self.volume.data_ptr(), self.labels.data_ptr(), d, h, w, self.count,
                                            table.data_ptr() if self.count else None, L.stream()), "cc_stats")
            self._table = table
        return self._table

    def volumes(self, spacing=(1, 1, 1)) -> torch.Tensor:
        """fp64 [count]: voxel count times the voxel's volume sz * sy * sx."""
        sz, sy, sx = (float(s) for s in spacing)
        return self.stats()[:, COUNT].double() * (sz * sy * sx)

    def centroids(self) -> torch.Tensor:
        """fp64 [count, 3]: the mean (z, y, x) voxel index of each component (scipy.ndimage.center_of_mass of its mask)."""
        t = self.stats()
        return t[:, SUM_Z:SUM_X + 1].double() / t[:, COUNT:COUNT + 1].double()

    def select(self, keep: torch.Tensor, fill: int = 0, out=None) -> torch.Tensor:
        """out[v] = fill where labels[v] > 0 and keep[labels[v]] is 0, else volume[v].  keep: uint8 / bool [count + 1] on the device,
        entry 0 is ignored.  out may be the volume itself."""
        vol = self.volume
        out = like_volume(out, vol, torch.uint8, "select", _OUT)
        if keep.dtype == torch.bool:
            keep = keep.to(torch.uint8)
        if keep.dtype != torch.uint8 or keep.numel() != self.count + 1 or keep.device != vol.device:
            raise ValueError(f"select: keep must be uint8 [{self.count + 1}] on {vol.device}")
        d, h, w = vol.shape
        L.check(L.lib().mednet_cc_select(vol.data_ptr(), self.labels.data_ptr(), keep.contiguous().data_ptr(), int(fill),
                                         out.data_ptr(), d, h, w, L.stream()), "cc_select")
        return out


def label_components(volume: torch.Tensor, cls=None, connectivity: int = 26, invert: bool = False) -> Components:
    """Label the components of `volume == cls` (`!=` with invert; cls=None: of every non-zero value, each value on its own).
    Reading K is the one host synchronisation of this module: 16 bytes, which also carry the kernels' error word (non-zero raises
    RuntimeError).  Because of it this is not for a captured step."""
    vol = volume_u8(volume, "label_components")
    d, h, w = vol.shape
    labels = torch.empty((d, h, w), dtype=torch.int32, device=vol.device)
    info = torch.empty((2,), dtype=torch.int64, device=vol.device)
    ws = L.workspace(L.lib().mednet_cc_ws_bytes(d, h, w), vol.device)
    L.check(L.lib().mednet_cc_label(vol.data_ptr(), L.CC_ALL if cls is None else int(cls), int(bool(invert)), int(connectivity), d, h, w,
                                    labels.data_ptr(), info.data_ptr(), ws.data_ptr(), ws.numel(), L.stream()), "cc_label")
    k, err = info.tolist()
    if err:
        raise RuntimeError(f"mednet_hip.cc_label: a parent walk reached its step cap (error word {err}); the labels are not valid")
    return Components(labels, int(k), vol)


def _keep_vector(keep_rows: torch.Tensor) -> torch.Tensor:
    """bool [K] per component -> uint8 [K + 1] for select (entry 0 unused)."""
    return torch.cat((torch.ones((1,), dtype=torch.uint8, device=keep_rows.device), keep_rows.to(torch.uint8)))


def _largest_keep(table: torch.Tensor, classes) -> torch.Tensor:
    """bool [K]: False for every component of a class in `classes` but its largest (ties: the smaller id)."""
    count, value = table[:, COUNT], table[:, VALUE]
    k = table.shape[0]
    keep = torch.ones((k,), dtype=torch.bool, device=table.device)
    ids = torch.arange(k, device=table.device)
    for c in classes:
        of = value == int(c)
        # the largest count wins, then the smaller id: one integer key, largest first
        key = torch.where(of, count * (k + 1) + (k - ids), torch.full_like(count, -1))
        best = torch.argmax(key) if k else None
        keep &= ~of | (ids == best)
    return keep


def _relabel(volume: torch.Tensor, who: str, cls, connectivity: int, invert: bool, keep_of, fill: int, out) -> torch.Tensor:
    """What keep_largest, remove_small and fill_holes share: ONE labelling (cls, connectivity, invert as label_components takes
    them), keep_of(comps) -> bool [K] of the components that stay, the others become `fill`.  A volume without a component is
    copied (or left, where out is the volume itself)."""
    comps = label_components(volume, cls, connectivity, invert)
    out = like_volume(out, comps.volume, torch.uint8, who, _OUT)
    if comps.count == 0:
        return out if out.data_ptr() == comps.volume.data_ptr() else out.copy_(comps.volume)
    return comps.select(_keep_vector(keep_of(comps)), fill, out)


def keep_largest(volume: torch.Tensor, classes, connectivity: int = 26, out=None) -> torch.Tensor:
    """Per class in `classes`, every component but the one with the most voxels becomes 0 (ties go to the smaller id, i.e. the
    component that starts first in raster order); a class absent from the volume is left alone.  All classes come from ONE labelling
    of the non-zero voxels by value.  out may be `volume` (in place)."""
    return _relabel(volume, "keep_largest", None, connectivity, False, lambda comps: _largest_keep(comps.stats(), classes), 0, out)


def _small_keep(table: torch.Tensor, thresholds: dict, voxel_volume=None) -> torch.Tensor:
    """bool [K]: False for components of class c with count (times voxel_volume, in fp64) < thresholds[c]."""
    count, value = table[:, COUNT], table[:, VALUE]
    keep = torch.ones((table.shape[0],), dtype=torch.bool, device=table.device)
    for c, t in thresholds.items():
        big = count >= int(t) if voxel_volume is None else count.double() * voxel_volume >= float(t)
        keep &= (value != int(c)) | big
    return keep


def remove_small(volume: torch.Tensor, classes, min_voxels=None, min_volume=None, spacing=(1, 1, 1), connectivity: int = 26,
                 out=None) -> torch.Tensor:
    """Components of the classes in `classes` below the threshold become 0.  Exactly one of min_voxels (a component is kept iff
    count >= min_voxels) and min_volume (kept iff count * sz * sy * sx >= min_volume, in fp64) is given."""
    if (min_voxels is None) == (min_volume is None):
        raise ValueError("remove_small: exactly one of min_voxels and min_volume must be given")
    sz, sy, sx = (float(s) for s in spacing)
    thresholds = {int(c): min_volume if min_voxels is None else min_voxels for c in classes}
    voxel_volume = None if min_volume is None else sz * sy * sx
    return _relabel(volume, "remove_small", None, connectivity, False, lambda c: _small_keep(c.stats(), thresholds, voxel_volume), 0, out)


def _border_keep(comps: Components) -> torch.Tensor:
    """bool [K]: True for components whose bounding box touches a face of the volume."""
    t = comps.stats()
    d, h, w = comps.volume.shape
    return (t[:, ZMIN] == 0) | (t[:, ZMAX] == d - 1) | (t[:, YMIN] == 0) | (t[:, YMAX] == h - 1) | (t[:, XMIN] == 0) | \
        (t[:, XMAX] == w - 1)


def fill_holes(volume: torch.Tensor, cls: int, out=None) -> torch.Tensor:
    """scipy.ndimage.binary_fill_holes(volume == cls) written back as `cls`: the components of `volume != cls` are labelled with
    connectivity 6 and every one whose bounding box touches no face of the volume becomes `cls`.  This OVERWRITES voxels of other
    classes that `cls` encloses."""
    return _relabel(volume, "fill_holes", int(cls), 6, True, _border_keep, int(cls), out)


class Postprocess:
    """A callable on a uint8 D x H x W volume: remove-small (min_voxels = {cls: n}: components of class cls with fewer than n voxels
    become 0), then keep-largest for the classes in keep_largest, then fill-holes for the classes in fill_holes, in that order.
    Returns a new volume; the input is left alone."""

    def __init__(self, keep_largest=(), min_voxels=None, fill_holes=(), connectivity: int = 26):
        self.keep_largest = tuple(int(c) for c in keep_largest)
        self.min_voxels = None if min_voxels is None else {int(c): int(n) for c, n in dict(min_voxels).items()}
        self.fill_holes = tuple(int(c) for c in fill_holes)
        self.connectivity = int(connectivity)

    def __call__(self, volume: torch.Tensor) -> torch.Tensor:
        out = volume_u8(volume, "Postprocess").clone()
        if self.min_voxels:
            _relabel(out, "Postprocess", None, self.connectivity, False, lambda c: _small_keep(c.stats(), self.min_voxels), 0, out)
        if self.keep_largest:
            keep_largest(out, self.keep_largest, self.connectivity, out=out)
        for c in self.fill_holes:
            fill_holes(out, c, out=out)
        return out
