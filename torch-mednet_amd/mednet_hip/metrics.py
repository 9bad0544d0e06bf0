"""Case-level evaluation of a whole-volume prediction on the device (csrc/metrics.hip): what a segmentation
model is judged by after inference, without the volumes leaving HBM.

    m = evaluate_case(pred, label, num_classes, spacing=(3.0, 0.7, 0.7))      # uint8 D x H x W each, e.g. GridPredictor(...)(vol)[-1]
    m.to_host()                                                                # one small table: the only transfer

Overlap, per class, from the confusion counts in fp64: Dice 2 TP / (|P| + |G|), IoU TP / (|P| + |G| - TP), sensitivity TP / |G|,
precision TP / |P|; a zero denominator gives NaN (a class absent from both volumes has Dice NaN, as nnU-Net reports it).

Surface distances, per class.  The surface S of a mask is `mask & ~erosion(mask)` with the 6-connected structuring element and
background outside the volume; d(a, S) is the Euclidean distance, in units of `spacing`, from voxel a to the nearest voxel of S.
With S_p, S_g the surfaces of the class in prediction and label, n_p, n_g their sizes:

    hd            = max(max_{p in S_p} d(p, S_g), max_{g in S_g} d(g, S_p))                   (MONAI compute_hausdorff_distance)
    hd_percentile = max of the two directed numpy.percentile(d, q) values, linear interpolation  (.. with percentile=q)
    assd          = (sum_p d(p, S_g) + sum_g d(g, S_p)) / (n_p + n_g)       (MONAI compute_average_surface_distance, symmetric)
    nsd           = (#{p : d(p, S_g) <= tol} + #{g : d(g, S_p) <= tol}) / (n_p + n_g)           (DeepMind's surface Dice)

If either surface is empty all four are NaN and n_pred / n_label say why.  Distances come from the exact squared Euclidean distance
transform `edt_squared`, two per class (one per direction, one after the other in ONE fp32 volume of scratch).  Neither MONAI nor
scipy is needed."""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch

from . import _lib as L
from ._volume import like_volume, volume_u8

MAX_CLASSES = 32
_PAD_LABEL, _PAD_IGNORE = 255, 254     # uint8 codes of a converted label outside 0 .. 255 / of an ignore_index outside 0 .. 255


def _label_u8(label: torch.Tensor, ignore_index, who: str):
    """-> (uint8 volume, the ignore code for the kernel).  A label of another integer type is converted: values outside 0 .. 255
    become 255 (out of range for every class count the kernel takes), an ignore_index outside 0 .. 255 becomes 254."""
    L.require_gpu(label, who)
    ign = L.NO_IGNORE if ignore_index is None else int(ignore_index)
    if label.dtype in (torch.uint8, torch.bool):
        return volume_u8(label, who), (ign if 0 <= ign <= 255 else L.NO_IGNORE)
    lab = label.long()
    out = torch.where((lab < 0) | (lab > 255), torch.full_like(lab, _PAD_LABEL), lab)
    if ignore_index is not None and not 0 <= ign <= 255:
        out = torch.where(lab == ign, torch.full_like(lab, _PAD_IGNORE), out)
        ign = _PAD_IGNORE
    return volume_u8(out.to(torch.uint8), who), ign


def _same_shape(a, b, who):
    if a.shape != b.shape or a.device != b.device:
        raise ValueError(f"{who}: prediction {tuple(a.shape)} on {a.device} and label {tuple(b.shape)} on {b.device} differ")


def _spacing(spacing):
    sz, sy, sx = (float(np.float32(s)) for s in spacing)
    return sz, sy, sx


# ------------------------------------------------------------------------------------------------------- overlap
def confusion(pred: torch.Tensor, label: torch.Tensor, num_classes: int, ignore_index=None):
    """-> (int64 [C, C] with entry [l, p] = voxels of label l predicted as p, int64 scalar = voxels left out because label or
    prediction is >= C), both on the device.  Voxels whose label equals ignore_index are counted nowhere."""
    p = volume_u8(pred, "confusion")
    lab, ign = _label_u8(label, ignore_index, "confusion")
    _same_shape(p, lab, "confusion")
    c = int(num_classes)
    d, h, w = p.shape
    out = torch.empty((max(c, 0) * max(c, 0) + 1,), dtype=torch.int64, device=p.device)
    ws = L.workspace(L.lib().mednet_confusion_ws_bytes(d, h, w, c), p.device)
    L.check(L.lib().mednet_confusion(p.data_ptr(), lab.data_ptr(), d, h, w, c, ign, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                     L.stream()), "confusion")
    return out[:c * c].view(c, c), out[c * c]


def overlap(cm: torch.Tensor):
    """cm int64 [C, C] (rows: label) -> dice, iou, sensitivity, precision, volume_pred, volume_label, each [C] on cm's device; the
    ratios in fp64 from the integer counts, NaN where the denominator is 0."""
    tp = cm.diagonal()
    vol_label, vol_pred = cm.sum(1), cm.sum(0)
    tpd, vl, vp = tp.double(), vol_label.double(), vol_pred.double()
    return 2.0 * tpd / (vp + vl), tpd / (vp + vl - tpd), tpd / vl, tpd / vp, vol_pred, vol_label


# ------------------------------------------------------------------------------------------------------- building blocks
def _surface_masks(a: torch.Tensor, b, cls: int):
    d, h, w = a.shape
    out_a = torch.empty_like(a)
    out_b = None if b is None else torch.empty_like(b)
    L.check(L.lib().mednet_surface_mask(a.data_ptr(), out_a.data_ptr(), L.ptr(b), L.ptr(out_b), int(cls), d, h, w, L.stream()),
            "surface_mask")
    return out_a, out_b


def surface_mask(volume: torch.Tensor, cls: int) -> torch.Tensor:
    """uint8 D x H x W: 1 where volume == cls and a face neighbour differs or lies outside the volume."""
    return _surface_masks(volume_u8(volume, "surface_mask"), None, cls)[0]


def edt_squared(seed: torch.Tensor, spacing=(1, 1, 1), out=None) -> torch.Tensor:
    """fp32 D x H x W: the squared Euclidean distance, in units of `spacing` = (z, y, x), to the nearest voxel with seed != 0; +inf
    everywhere without a seed.  Exact for unit and dyadic spacing (include/mednet_hip.h gives the arithmetic).  out: an fp32 volume
    to write into."""
    s = volume_u8(seed, "edt_squared")
    d, h, w = s.shape
    out = like_volume(out, s, torch.float32, "edt_squared", "out must be a contiguous fp32 volume of the seed's shape on its device")
    sz, sy, sx = _spacing(spacing)
    L.check(L.lib().mednet_edt_sq(s.data_ptr(), out.data_ptr(), d, h, w, sz, sy, sx, L.stream()), "edt_squared")
    return out


def surface_stats(surf: torch.Tensor, d2: torch.Tensor, tol_sq: float, counts=None, max_d2=None, sum_sqrt=None):
    """Over the voxels with surf != 0 -> (int64 [2] = {their number, those with d2 <= tol_sq}, fp32 scalar max d2 (-inf for none),
    fp64 scalar sum of sqrt(d2)), written into the given tensors where given."""
    s = volume_u8(surf, "surface_stats")
    d, h, w = s.shape
    like_volume(d2, s, torch.float32, "surface_stats", "d2 must be a contiguous fp32 volume of the mask's shape", same_device=False)
    counts = torch.empty((2,), dtype=torch.int64, device=s.device) if counts is None else counts
    max_d2 = torch.empty((), dtype=torch.float32, device=s.device) if max_d2 is None else max_d2
    sum_sqrt = torch.empty((), dtype=torch.float64, device=s.device) if sum_sqrt is None else sum_sqrt
    ws = L.workspace(L.lib().mednet_surface_stats_ws_bytes(d, h, w), s.device)
    L.check(L.lib().mednet_surface_stats(s.data_ptr(), d2.data_ptr(), d, h, w, float(tol_sq), counts.data_ptr(), max_d2.data_ptr(),
                                         sum_sqrt.data_ptr(), ws.data_ptr(), ws.numel(), L.stream()), "surface_stats")
    return counts, max_d2, sum_sqrt


def _root32(x: torch.Tensor) -> torch.Tensor:
    """The correctly rounded fp32 square root (an fp64 root rounded to fp32 is that: 53 >= 2 * 24 + 2 bits)."""
    return torch.sqrt(x.double()).float()


def _directed_percentile(d2: torch.Tensor, surf: torch.Tensor, q: float) -> torch.Tensor:
    """numpy.percentile(sqrt(d2[surf]), q) with linear interpolation, fp32 on the device: the two order statistics are selected on
    d2 (exact), rooted, and interpolated as a + (b - a) * t.  NaN for an empty surface."""
    v = d2[surf.bool()]
    n = v.numel()
    if n == 0:
        return torch.full((), float("nan"), dtype=torch.float32, device=d2.device)
    v = torch.sort(v).values
    pos = q / 100.0 * (n - 1)
    lo = min(int(math.floor(pos)), n - 1)
    hi = min(lo + 1, n - 1)
    a, b = _root32(v[lo]), _root32(v[hi])
    t = pos - lo
    return a if t == 0.0 else a + (b - a) * t


# ------------------------------------------------------------------------------------------------------- surface distances
def surface_distances(pred: torch.Tensor, label: torch.Tensor, classes, spacing=(1, 1, 1), percentile=95.0, tolerance=1.0):
    """-> hd (fp32), hd_percentile (fp32), assd (fp64), nsd (fp64), n_pred, n_label (int64), each [len(classes)] on the device; the
    module docstring gives the definitions.  tolerance is in units of `spacing`; a voxel counts as within it when its squared
    distance is <= fp32(tolerance)^2."""
    p = volume_u8(pred, "surface_distances")
    g, _ = _label_u8(label, None, "surface_distances")
    _same_shape(p, g, "surface_distances")
    if not (float(tolerance) >= 0.0):
        raise ValueError(f"surface_distances: tolerance {tolerance} is negative or NaN")
    if not 0.0 <= float(percentile) <= 100.0:
        raise ValueError(f"surface_distances: percentile {percentile} outside [0, 100]")
    classes = [int(c) for c in classes]
    k, dev = len(classes), p.device
    tol_sq = float(np.float32(tolerance) * np.float32(tolerance))
    counts = torch.empty((max(k, 1), 2, 2), dtype=torch.int64, device=dev)       # [class][direction][n, within]
    mx = torch.empty((max(k, 1), 2), dtype=torch.float32, device=dev)
    sm = torch.empty((max(k, 1), 2), dtype=torch.float64, device=dev)
    pct = []
    d2 = torch.empty(tuple(p.shape), dtype=torch.float32, device=dev)            # the one volume of scratch, both directions
    for i, cls in enumerate(classes):
        sp, sg = _surface_masks(p, g, cls)
        row = []
        for j, (seed, surf) in enumerate(((sg, sp), (sp, sg))):                  # prediction -> label surface, then label -> prediction
            edt_squared(seed, spacing, out=d2)
            surface_stats(surf, d2, tol_sq, counts[i, j], mx[i, j], sm[i, j])
            row.append(_directed_percentile(d2, surf, float(percentile)))
        pct.append(torch.maximum(row[0], row[1]))
    counts, mx, sm = counts[:k], mx[:k], sm[:k]
    n_pred, n_label = counts[:, 0, 0], counts[:, 1, 0]
    valid = (n_pred > 0) & (n_label > 0)
    total = (n_pred + n_label).double()
    nan32 = torch.full((k,), float("nan"), dtype=torch.float32, device=dev)
    nan64 = nan32.double()
    hd = torch.where(valid, _root32(torch.maximum(mx[:, 0], mx[:, 1])), nan32)
    hdp = torch.where(valid, torch.stack(pct) if k else nan32, nan32)
    assd = torch.where(valid, (sm[:, 0] + sm[:, 1]) / total, nan64)
    nsd = torch.where(valid, (counts[:, 0, 1] + counts[:, 1, 1]).double() / total, nan64)
    return hd, hdp, assd, nsd, n_pred, n_label


_PER_CLASS = ("dice", "iou", "sensitivity", "precision", "volume_pred", "volume_label")
_PER_SURFACE = ("hd", "hd_percentile", "assd", "nsd", "n_pred", "n_label")
_COUNTS = ("volume_pred", "volume_label", "n_pred", "n_label")


@dataclasses.dataclass
class CaseMetrics:
    """Everything evaluate_case measured, on the device.  confusion [C, C] (rows: label) and out_of_range; the overlap fields [C];
    the surface fields [len(classes)], in the order of `classes`."""
    confusion: torch.Tensor
    out_of_range: torch.Tensor
    dice: torch.Tensor
    iou: torch.Tensor
    sensitivity: torch.Tensor
    precision: torch.Tensor
    volume_pred: torch.Tensor
    volume_label: torch.Tensor
    classes: tuple
    hd: torch.Tensor
    hd_percentile: torch.Tensor
    assd: torch.Tensor
    nsd: torch.Tensor
    n_pred: torch.Tensor
    n_label: torch.Tensor
    spacing: tuple
    percentile: float
    tolerance: float

    def to_host(self) -> dict:
        """One transfer: every field packed into one fp64 vector (the counts are exact in it, the fp32 fields widen exactly) -> a
        dict of numpy arrays, counts as int64, plus `classes`, `spacing`, `percentile`, `tolerance`."""
        names = ("confusion", "out_of_range") + _PER_CLASS + _PER_SURFACE
        parts = [getattr(self, n).reshape(-1).double() for n in names]
        flat = torch.cat(parts).cpu().numpy()
        out, at = {}, 0
        for n, part in zip(names, parts):
            a = flat[at:at + part.numel()]
            at += part.numel()
            out[n] = a.astype(np.int64) if n in _COUNTS or n in ("confusion", "out_of_range") else a.copy()
        c = self.confusion.shape[0]
        out["confusion"] = out["confusion"].reshape(c, c)
        out["out_of_range"] = int(out["out_of_range"][0])
        out.update(classes=tuple(self.classes), spacing=tuple(self.spacing), percentile=self.percentile, tolerance=self.tolerance)
        return out


_LESION_COUNTS = ("n_label", "n_pred", "tp_label", "fn", "fp", "tp_pred")
_LESION_RATIOS = ("sensitivity", "precision", "f1")


@dataclasses.dataclass
class LesionDetection:
    """Lesion-wise detection counts of one class, int64 scalars on the device: n_label / n_pred components of the class in label /
    prediction; tp_label label components overlapped by some prediction component, fn = n_label - tp_label; fp prediction components
    that overlap no label component, tp_pred = n_pred - fp.  In fp64: sensitivity tp_label / n_label, precision tp_pred / n_pred and
    f1, their harmonic mean; a zero denominator gives NaN."""
    n_label: torch.Tensor
    n_pred: torch.Tensor
    tp_label: torch.Tensor
    fn: torch.Tensor
    fp: torch.Tensor
    tp_pred: torch.Tensor
    sensitivity: torch.Tensor
    precision: torch.Tensor
    f1: torch.Tensor

    def to_host(self) -> dict:
        """One transfer: the nine fields in one fp64 vector (the counts are exact in it) -> counts as int, ratios as float."""
        flat = torch.stack([getattr(self, n).double() for n in _LESION_COUNTS + _LESION_RATIOS]).cpu().numpy()
        out = {n: int(flat[i]) for i, n in enumerate(_LESION_COUNTS)}
        out.update({n: float(flat[len(_LESION_COUNTS) + i]) for i, n in enumerate(_LESION_RATIOS)})
        return out


def lesion_detection(pred: torch.Tensor, label: torch.Tensor, cls: int, connectivity: int = 26, min_overlap: int = 1) -> LesionDetection:
    """Component-wise detection of class `cls`: the components of pred == cls and of label == cls are labelled on the device
    (mednet_hip.components); a prediction component and a label component overlap if they share >= min_overlap voxels.  The pairs
    are counted with torch.unique on the key pid * (K_label + 1) + gid over the voxels where both are labelled.  Synchronises with
    the host (the two component counts and the unique); not for a captured step."""
    from .components import label_components
    p = volume_u8(pred, "lesion_detection")
    g, _ = _label_u8(label, None, "lesion_detection")
    _same_shape(p, g, "lesion_detection")
    if int(min_overlap) < 1:
        raise ValueError(f"lesion_detection: min_overlap {min_overlap} must be at least 1")
    cp, cg = label_components(p, int(cls), connectivity), label_components(g, int(cls), connectivity)
    kp, kg, dev = cp.count, cg.count, p.device
    both = (cp.labels > 0) & (cg.labels > 0)
    key, shared = torch.unique(cp.labels[both].long() * (kg + 1) + cg.labels[both].long(), return_counts=True)
    key = key[shared >= int(min_overlap)]
    hit_p = torch.zeros((kp + 1,), dtype=torch.bool, device=dev)
    hit_g = torch.zeros((kg + 1,), dtype=torch.bool, device=dev)
    hit_p[torch.div(key, kg + 1, rounding_mode="floor")] = True
    hit_g[key % (kg + 1)] = True
    n_label, n_pred = torch.tensor(kg, dtype=torch.int64, device=dev), torch.tensor(kp, dtype=torch.int64, device=dev)
    tp_label, tp_pred = hit_g.sum(), hit_p.sum()
    sens, prec = tp_label.double() / n_label.double(), tp_pred.double() / n_pred.double()
    return LesionDetection(n_label, n_pred, tp_label, n_label - tp_label, n_pred - tp_pred, tp_pred, sens, prec,
                           2.0 * sens * prec / (sens + prec))


@dataclasses.dataclass
class CaseMetricsWithLesions(CaseMetrics):
    """CaseMetrics plus `lesions`: {cls: LesionDetection} for the lesion_classes evaluate_case was asked for; to_host() adds
    `lesion_classes` and one `lesion_<field>` array per field of LesionDetection, in the order of lesion_classes."""
    lesions: dict = None

    def to_host(self) -> dict:
        out = super().to_host()
        rows = [self.lesions[c].to_host() for c in self.lesions]
        out["lesion_classes"] = tuple(self.lesions)
        for n in _LESION_COUNTS:
            out["lesion_" + n] = np.asarray([r[n] for r in rows], dtype=np.int64)
        for n in _LESION_RATIOS:
            out["lesion_" + n] = np.asarray([r[n] for r in rows], dtype=np.float64)
        return out


def evaluate_case(pred: torch.Tensor, label: torch.Tensor, num_classes: int, spacing=(1, 1, 1), classes=None, percentile=95.0,
                  tolerance=1.0, ignore_index=None, lesion_classes=None, lesion_connectivity=26, lesion_min_overlap=1) -> CaseMetrics:
    """Overlap for every class and surface distances for `classes` (default 1 .. C - 1) of one case.  pred, label: D x H x W on the
    device (uint8; a label of another integer type is converted).  ignore_index applies to the confusion counts.  Synchronises with
    the host (the percentile selects the surface voxels); not for a captured step.  lesion_classes: classes to count lesion-wise as
    well (lesion_detection); the result is then a CaseMetricsWithLesions, whose to_host() has the additional `lesion_*` keys."""
    cm, oor = confusion(pred, label, num_classes, ignore_index)
    dice, iou, sens, prec, vp, vl = overlap(cm)
    classes = tuple(range(1, int(num_classes))) if classes is None else tuple(int(c) for c in classes)
    hd, hdp, assd, nsd, n_pred, n_label = surface_distances(pred, label, classes, spacing, percentile, tolerance)
    fields = (cm, oor, dice, iou, sens, prec, vp, vl, classes, hd, hdp, assd, nsd, n_pred, n_label,
              tuple(float(s) for s in spacing), float(percentile), float(tolerance))
    if lesion_classes is None:
        return CaseMetrics(*fields)
    lesions = {int(c): lesion_detection(pred, label, int(c), lesion_connectivity, lesion_min_overlap) for c in lesion_classes}
    return CaseMetricsWithLesions(*fields, lesions)


def landmark_errors(positions: torch.Tensor, targets, spacing=(1, 1, 1)) -> torch.Tensor:
    """Euclidean error per landmark in units of `spacing`: positions H x 3 as (z, y, x) voxel indices (what peaks() returns),
    targets likewise (a tensor or anything torch.as_tensor takes) -> fp64 [H] on positions' device."""
    pos = positions.double()
    tgt = torch.as_tensor(targets, dtype=torch.float64, device=pos.device)
    sp = torch.as_tensor([float(s) for s in spacing], dtype=torch.float64, device=pos.device)
    return torch.linalg.vector_norm((pos - tgt) * sp, dim=-1)
