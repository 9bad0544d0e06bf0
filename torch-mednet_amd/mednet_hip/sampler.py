"""Class-balanced random patch sampler on device-resident volumes: MedDataset of
midasmednet/dataset.py:208-346 without the per-patch numpy crop, pickling and host-to-device copy.

The volumes (images float16, labels / heat maps uint8 -- the dtypes the reference preloads, dataset.py:254-257) are
uploaded once.  WHERE to crop is decided on the host by the reference's own procedure -- get_labeled_position (:18-52) and
get_random_patch_indices (:55-88), drawing from numpy's global generator in the reference's order, so a seeded run visits
the same patches as the reference -- and the crop + cast (:313-331) of a whole batch is a few launches of
mednet_crop_patches writing straight into the batch tensors the training step consumes
({'data': fp32 B x C x pD x pH x pW, 'label': uint8 B x (heat maps + 1) x ...}, segmentation.py:58-61).
The optional `transform` of the reference -- the batchgenerators Compose of examples/train_seg.py:82-86 (additive brightness,
gamma, contrast on `data`), applied per sample at dataset.py:340-341 -- is `augment=True`: its random numbers are drawn on
the host right after the sample's position (the reference's order of calls into numpy's global generator), the arithmetic
runs on the device (mednet_augment_patches).  batchgenerators itself is not available here: see oracle/ref_augment.py
("parity unpinned").

Spatial transforms -- what a batchgenerators Compose usually opens with: random rotation, scaling, mirroring, elastic deformation --
are `spatial=SpatialAugmentation(...)`: the sample's parameters are drawn on the host after its position and before the intensity
draws (spatial first, batchgenerators' usual order), and mednet_warp_patches does crop + transform in one pass in place of
mednet_crop_patches (images trilinear, heat maps trilinear and rounded once, labels nearest).  Parity with batchgenerators is
unpinned here as well, and the elastic model is NOT batchgenerators' (Gaussian-filtered full-resolution noise) but this library's
own: normal displacements on a coarse control lattice, interpolated trilinearly.  As with batchgenerators, a rotated or deformed
patch may lose the labelled voxel the class-balanced position was drawn for.  `spatial=None` is the path without any of this: the
same launches and the same generator calls as before.

Gaussian noise, Gaussian blur and simulated low resolution -- the transforms nnU-Net's pipeline runs between the spatial transform
and the brightness / contrast / gamma group -- are `degrade=ImageDegradation(...)`: drawn per sample after the spatial draws and
before the intensity ones, run on the device (csrc/degrade.hip) between the crop or warp and `augment_`.  The noise is the library's
own counter-based generator (philox4x32-10, a pure function of the batch's seed, the row and the voxel); blur and low resolution
are separable table passes over the whole batch with one table per (sample, channel) row.  `degrade=None` changes nothing."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L


def get_labeled_position(label, class_value, label_any=None):
    """dataset.py:18-52 (host, numpy).  The reference keeps only the first matching index along axis 2."""
    if label_any is None:
        label_any = np.any(label == class_value, axis=2)
    valid_idx = np.argwhere(label_any == True)  # noqa: E712
    if valid_idx.size:
        rnd = np.random.randint(0, valid_idx.shape[0])
        idx = valid_idx[rnd]
        first = np.argwhere(label[idx[0], idx[1], :] == class_value)[0]
        return [idx[0], idx[1], np.random.choice(first)]
    return None


def get_random_patch_indices(patch_size, img_shape, pos=None):
    """dataset.py:55-88 (host, numpy)."""
    if pos:
        pos = np.array(pos, dtype=int)
        min_index = np.maximum(pos - patch_size + 1, 0)
        max_index = np.minimum(img_shape - patch_size + 1, pos + 1)
    else:
        min_index = np.array([0, 0, 0])
        max_index = img_shape - patch_size + 1
    index_ini = np.random.randint(low=min_index, high=max_index)
    return index_ini, index_ini + patch_size


# examples/train_seg.py:84-86
AUG_BRIGHTNESS = (0.0, 0.3)      # BrightnessTransform(mu, sigma)
AUG_GAMMA_RANGE = (0.7, 1.3)     # GammaTransform(gamma_range)
AUG_CONTRAST_RANGE = (0.3, 1.7)  # ContrastAugmentationTransform(contrast_range)


def _range_draw(lo_hi):
    if np.random.random() < 0.5 and lo_hi[0] < 1:
        return np.random.uniform(lo_hi[0], 1)
    return np.random.uniform(max(lo_hi[0], 1), lo_hi[1])


def draw_augmentation(channels):
    """The draws of one Compose call on ONE sample, in batchgenerators' order (per-sample and per-channel probability
    draws included, all probabilities 1) -> (C, 3) float32: additive brightness, gamma (one per sample), contrast factor."""
    out = np.zeros((channels, 3), dtype=np.float32)
    np.random.uniform()
    for c in range(channels):
        np.random.uniform()
        out[c, 0] = np.random.normal(*AUG_BRIGHTNESS)
    np.random.uniform()
    out[:, 1] = _range_draw(AUG_GAMMA_RANGE)
    np.random.uniform()
    for c in range(channels):
        out[c, 2] = _range_draw(AUG_CONTRAST_RANGE)
    return out


def augment_(data, params):
    """In place on a B x C x ... fp32 device tensor; params: (B, C, 3) array / tensor as from draw_augmentation."""
    L.require_gpu(data, "augment")
    assert data.dtype == torch.float32 and data.is_contiguous()
    b, c = data.shape[:2]
    spatial = data[0, 0].numel()
    prm = torch.as_tensor(np.asarray(params, dtype=np.float32)).reshape(b, c, 3).to(data.device).contiguous()
    lib = L.lib()
    ws = L.workspace(lib.mednet_augment_ws_bytes(b, c, spatial), data.device)
    L.check(lib.mednet_augment_patches(data.data_ptr(), prm.data_ptr(), b, c, spatial, ws.data_ptr(), ws.numel(), L.stream()),
            "augment_patches")
    return data


_DT = {torch.float16: L.F16, torch.float32: L.F32, torch.uint8: L.U8}
_BORDER = {"constant": L.BORDER_CONSTANT, "edge": L.BORDER_EDGE}
_INTERP = {"linear": L.INTERP_LINEAR, "nearest": L.INTERP_NEAREST}


def _rotation(ax, ay, az):
    """R_z . R_y . R_x in fp64 on (z, y, x) coordinates: R_x turns the (z, y) plane about the x axis, R_y the (z, x) plane, R_z the
    (y, x) plane; angles in radians."""
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = np.array([[cx, -sx, 0.0], [sx, cx, 0.0], [0.0, 0.0, 1.0]])
    ry = np.array([[cy, 0.0, -sy], [0.0, 1.0, 0.0], [sy, 0.0, cy]])
    rz = np.array([[1.0, 0.0, 0.0], [0.0, cz, -sz], [0.0, sz, cz]])
    return rz @ ry @ rx


class SpatialAugmentation:
    """Random rotation, scaling, mirroring and elastic deformation of one training patch, as parameters of mednet_warp_patches.

    rotation     ((lo, hi),) * 3 in radians about the x, y and z axes, or None
    scale        (lo, hi): one isotropic factor on the SOURCE step (> 1 zooms out: the patch covers more of the volume), or None
    mirror_axes  patch axes (0 = z, 1 = y, 2 = x) that are reversed with probability 1/2 each
    elastic      (spacing_voxels, sigma_voxels): normal(0, sigma) displacements in patch voxels on a control lattice of
                 ceil(p / spacing) + 1 points per axis whose corners sit on the patch's corner voxels, or None
    p_*          probability that the drawn rotation / scale / lattice is applied
    border_*     "constant" (taps outside read the cval) or "edge" (indices are clamped); the defaults are those of batchgenerators'
                 SpatialTransform (border_mode_data 'nearest', border_mode_seg 'constant' with 0).  Heat maps take the label rule.

    draw() makes these calls into numpy's global generator, in this order, whatever the outcome of a probability test -- a sample
    always consumes calls_per_sample() of them:
      rotation: uniform() [p_rotation], uniform(lo, hi) for the x, y and z angle      4 calls
      scale:    uniform() [p_scale], uniform(lo, hi)                                  2 calls
      mirror:   uniform() per listed axis, in the order given                         len(mirror_axes) calls
      elastic:  uniform() [p_elastic], normal(0, sigma, (3, gd, gh, gw))              2 calls
    An option that is None makes none.  The matrix is R_z . R_y . R_x . scale . mirror signs in fp64, rounded once to fp32; the
    translation is the drawn patch position plus the patch-centre offset (p - 1) / 2."""

    def __init__(self, rotation=None, scale=None, mirror_axes=(), elastic=None, p_rotation=1.0, p_scale=1.0, p_elastic=1.0,
                 border_data="edge", data_cval=0.0, border_label="constant", label_cval=0):
        if rotation is not None:
            rotation = tuple((float(lo), float(hi)) for lo, hi in rotation)
            assert len(rotation) == 3
        self.rotation = rotation
        self.scale = None if scale is None else (float(scale[0]), float(scale[1]))
        self.mirror_axes = tuple(int(a) for a in mirror_axes)
        assert all(a in (0, 1, 2) for a in self.mirror_axes)
        self.elastic = None if elastic is None else (float(elastic[0]), float(elastic[1]))
        assert self.elastic is None or self.elastic[0] > 0
        self.p_rotation, self.p_scale, self.p_elastic = float(p_rotation), float(p_scale), float(p_elastic)
        assert border_data in _BORDER and border_label in _BORDER
        assert 0 <= int(label_cval) <= 255
        self.border_data, self.data_cval, self.border_label, self.label_cval = border_data, float(data_cval), border_label, int(label_cval)

    def calls_per_sample(self):
        return 4 * (self.rotation is not None) + 2 * (self.scale is not None) + len(self.mirror_axes) + 2 * (self.elastic is not None)

    def lattice_shape(self, patch_size):
        if self.elastic is None:
            return None
        return tuple(int(np.ceil(int(p) / self.elastic[0])) + 1 for p in patch_size)

    def draw(self, position, patch_size):
        """One sample: (affine (12,) float32 = row-major [A | t], lattice (3, gd, gh, gw) float32 or None)."""
        m = np.eye(3)
        if self.rotation is not None:
            take = np.random.uniform() < self.p_rotation
            ax, ay, az = (np.random.uniform(lo, hi) for lo, hi in self.rotation)
            if take:
                m = _rotation(ax, ay, az)
        if self.scale is not None:
            take = np.random.uniform() < self.p_scale
            f = np.random.uniform(*self.scale)
            if take:
                m = m * f
        for a in self.mirror_axes:
            if np.random.uniform() < 0.5:
                m[:, a] = -m[:, a]
        lattice = None
        if self.elastic is not None:
            take = np.random.uniform() < self.p_elastic
            lattice = np.random.normal(0.0, self.elastic[1], (3,) + self.lattice_shape(patch_size)).astype(np.float32)
            if not take:
                lattice[...] = 0
        p = np.asarray(patch_size, dtype=np.float64)
        t = np.asarray(position, dtype=np.float64) + (p - 1) / 2
        affine = np.concatenate([m + 0.0, t[:, None]], axis=1).astype(np.float32)  # (+ 0.0: no negative zeros)
        return affine.reshape(12), lattice


def warp_patches(volume, affine, slot, out, c_off=0, interp="linear", border="edge", cval=0.0, disp=None):
    """out[slot[i], c_off : c_off + C] = the warped patch of row i (mednet_warp_patches, include/mednet_hip.h): volume C x D x H x W
    (float16 / float32 -> float32 out, uint8 -> uint8 out), affine (count, 12) float32, slot (count,) int32, disp None or
    (count, 3, gd, gh, gw) float32 -- device tensors; out B x c_total x pD x pH x pW."""
    L.require_gpu(volume, "warp_patches")
    assert volume.is_contiguous() and out.is_contiguous() and affine.is_contiguous() and slot.is_contiguous()
    assert affine.dtype == torch.float32 and slot.dtype == torch.int32 and affine.numel() == 12 * slot.numel()
    gd = gh = gw = 0
    if disp is not None:
        assert disp.dtype == torch.float32 and disp.is_contiguous() and disp.shape[:2] == (slot.numel(), 3)
        gd, gh, gw = disp.shape[2:]
    c, d, h, w = volume.shape
    pd, ph, pw = out.shape[2:]
    L.check(L.lib().mednet_warp_patches(volume.data_ptr(), _DT[volume.dtype], affine.data_ptr(), L.ptr(disp), gd, gh, gw,
                                        slot.data_ptr(), slot.numel(), out.data_ptr(), _DT[out.dtype], c, d, h, w, out.shape[1], c_off,
                                        pd, ph, pw, _INTERP[interp], _BORDER[border], float(cval), L.stream()), "warp_patches")
    return out


# ---------------------------------------------------------------------------------------------- noise, blur, low resolution
# csrc/degrade.hip, DESIGN.md section 32.  Blur and simulated low resolution are separable table passes like resample.py's, per
# (sample, channel) row of the batch: a table states, per output index, `count` taps with an explicit source index and a weight.
FILTER_MAX_TAPS = 64


def _reflect(j, n):
    """scipy's mode="reflect" (d c b a | a b c d | d c b a) by the periodic formula, so any j and n >= 1 are legal."""
    j = np.mod(j, 2 * n)
    return np.where(j >= n, 2 * n - 1 - j, j)


def blur_table(n, sigma):
    """(count int32 [n], index int32 [n][taps], weight fp32 [n][taps], taps) of scipy.ndimage.gaussian_filter1d(sigma,
    mode="reflect", truncate=4.0) on an axis of extent n: radius r = int(4 sigma + 0.5), weights exp(-k^2 / 2 sigma^2) normalised in
    fp64 and rounded once to fp32, index reflect(i - r + k).  None for sigma == 0 (no table: the row is copied)."""
    n, sigma = int(n), float(sigma)
    if not (np.isfinite(sigma) and sigma >= 0):
        raise ValueError(f"blur_table: sigma {sigma!r} is not finite and non-negative")
    if sigma == 0:
        return None
    r = int(4.0 * sigma + 0.5)
    taps = 2 * r + 1
    if taps > FILTER_MAX_TAPS:
        raise ValueError(f"blur_table: sigma {sigma} needs {taps} taps (at most {FILTER_MAX_TAPS})")
    k = np.arange(-r, r + 1, dtype=np.float64)
    wt = np.exp(-0.5 * k * k / (sigma * sigma))
    wt = (wt / wt.sum()).astype(np.float32)
    index = _reflect(np.arange(n)[:, None] + np.arange(-r, r + 1)[None, :], n).astype(np.int32)
    return np.full(n, taps, dtype=np.int32), index, np.broadcast_to(wt, (n, taps)).copy(), taps


_low_resolution_tables = {}


def low_resolution_table(n, zoom):
    """The composite of nearest-neighbour down-sampling to m = max(1, round(n zoom)) and cubic up-sampling back to n, as one table:
    count and weight are those of U = axis_table(m, n, "cubic"), index[i][k] is the source index that row U.start[i] + k of
    S = axis_table(n, m, "nearest") reads.  None for zoom >= 1 or m == n.  The table depends on (n, m) alone and is kept per pair
    (read-only arrays): a training run meets at most n of them per extent."""
    from .resample import axis_table
    n, zoom = int(n), float(zoom)
    if not (np.isfinite(zoom) and zoom > 0):
        raise ValueError(f"low_resolution_table: zoom {zoom!r} is not finite and positive")
    m = max(1, int(round(n * zoom)))
    if zoom >= 1 or m == n:
        return None
    hit = _low_resolution_tables.get((n, m))
    if hit is None:
        s_start = axis_table(n, m, "nearest")[0]
        u_start, u_count, u_weight, taps = axis_table(m, n, "cubic")
        low = np.minimum(u_start[:, None].astype(np.int64) + np.arange(taps)[None, :], m - 1)   # (slots past count are never read)
        hit = (u_count.copy(), s_start[low].astype(np.int32), u_weight.copy(), taps)
        for a in hit[:3]:
            a.setflags(write=False)
        _low_resolution_tables[(n, m)] = hit
    return hit


def filter_rows(src, dst, axis, row_table, tables):
    """One axis pass over a batch (mednet_filter_rows, include/mednet_hip.h): src, dst B x C x D x H x W fp32, contiguous, distinct;
    row_table int32 [B * C]; tables = (count int32 [T][n], index int32 [T][n][taps], weight fp32 [T][n][taps]) -- device tensors."""
    L.require_gpu(src, "filter_rows")
    count, index, weight = tables
    assert src.dtype == dst.dtype == torch.float32 and src.is_contiguous() and dst.is_contiguous() and src.shape == dst.shape
    assert src.dim() == 5 and row_table.dtype == torch.int32 and row_table.numel() == src.shape[0] * src.shape[1]
    assert count.dtype == index.dtype == torch.int32 and weight.dtype == torch.float32
    assert all(t.is_contiguous() for t in (row_table, count, index, weight))
    n = src.shape[2 + axis]
    n_tables, taps = int(index.shape[0]), int(index.shape[2])
    assert tuple(count.shape) == (n_tables, n) and tuple(index.shape) == tuple(weight.shape) == (n_tables, n, taps)
    d, h, w = src.shape[2:]
    L.check(L.lib().mednet_filter_rows(src.data_ptr(), dst.data_ptr(), row_table.numel(), d, h, w, int(axis), row_table.data_ptr(),
                                       n_tables, count.data_ptr(), index.data_ptr(), weight.data_ptr(), taps, L.stream()), "filter_rows")
    return dst


def stack_tables(n, params, table_of):
    """The distinct tables of a pass: params is one value per row; -> (row_table int32 [rows], count [T][n], index [T][n][taps],
    weight [T][n][taps]) as numpy, each distinct (n, parameter) built once, padded to the longest table's taps; None if no row has
    a table."""
    built, row_table = {}, []
    for p in params:
        p = float(p)
        if p not in built:
            built[p] = table_of(n, p)
        row_table.append(p)
    keys = [p for p in built if built[p] is not None]
    if not keys:
        return None
    taps = max(built[p][3] for p in keys)
    count = np.stack([built[p][0] for p in keys]).astype(np.int32)
    index = np.zeros((len(keys), n, taps), dtype=np.int32)
    weight = np.zeros((len(keys), n, taps), dtype=np.float32)
    for t, p in enumerate(keys):
        index[t, :, :built[p][3]], weight[t, :, :built[p][3]] = built[p][1], built[p][2]
    slot = {p: t for t, p in enumerate(keys)}
    return np.array([slot.get(p, -1) for p in row_table], dtype=np.int32), count, index, weight


def _row_params(data, value):
    b, c = data.shape[:2]
    v = np.asarray(value, dtype=np.float64)
    return np.ascontiguousarray(np.broadcast_to(v if v.ndim else v.reshape(1, 1), (b, c))).reshape(b * c)


def _filter_passes(data, params, table_of, scratch, who):
    """Axis 2, then 1, then 0, ping-pong between data and ONE scratch tensor; an axis on which no row has a table launches nothing.
    -> the tensor that holds the result (data or the scratch)."""
    L.require_gpu(data, who)
    if data.dtype != torch.float32 or data.dim() != 5 or not data.is_contiguous():
        raise ValueError(f"{who}: a contiguous float32 B x C x D x H x W batch expected, got {tuple(data.shape)} {data.dtype}")
    cur, other = data, scratch
    for axis in (2, 1, 0):
        st = stack_tables(int(data.shape[2 + axis]), params, table_of)
        if st is None:
            continue
        if other is None:
            other = torch.empty_like(data)
        assert other.shape == data.shape and other.dtype == data.dtype and other.is_contiguous() and other.data_ptr() != cur.data_ptr()
        row_table, count, index, weight = (torch.from_numpy(a).to(data.device) for a in st)     # one copy per array
        filter_rows(cur, other, axis, row_table, (count, index, weight))
        cur, other = other, cur
    return cur


def gaussian_noise_(data, std, seed):
    """In place on a B x C x ... fp32 device tensor: data += std * z(seed, row, voxel) (mednet_noise_patches: philox4x32-10 and
    Box-Muller, a pure function of the seed, the row b * C + c and the voxel).  std: a scalar or a (B, C) array; rows with std 0 are
    not touched, and nothing is launched when every row's is 0."""
    L.require_gpu(data, "gaussian_noise_")
    if data.dtype != torch.float32 or data.dim() < 3 or not data.is_contiguous():
        raise ValueError(f"gaussian_noise_: a contiguous float32 B x C x ... batch expected, got {tuple(data.shape)} {data.dtype}")
    sd = _row_params(data, std).astype(np.float32)
    if not sd.any():
        return data
    rows = sd.size
    L.check(L.lib().mednet_noise_patches(data.data_ptr(), torch.from_numpy(sd).to(data.device).data_ptr(), int(seed) & (2 ** 64 - 1), rows,
                                         data.numel() // rows, L.stream()), "noise_patches")
    return data


def gaussian_blur(data, sigma, scratch=None):
    """scipy.ndimage.gaussian_filter(mode="reflect", truncate=4.0) of every (sample, channel) volume of a B x C x D x H x W fp32 device
    batch, one sigma (a scalar or a (B, C) array, 0: untouched) for all three axes.  -> the tensor that holds the result: `data`
    itself or the scratch tensor (`scratch`, or one allocated here), whichever the last pass wrote."""
    return _filter_passes(data, _row_params(data, sigma), blur_table, scratch, "gaussian_blur")


def simulate_low_resolution(data, zoom, scratch=None):
    """Every (sample, channel) volume down-sampled by `zoom` (a scalar or a (B, C) array; >= 1: untouched) with nearest neighbour and
    back up with this library's cubic kernel: bit for bit resample(resample(x, size=m, kind="nearest"), size=n, kind="cubic"),
    in three composite passes -- the low-resolution volume never exists.  -> the tensor that holds the result, as gaussian_blur."""
    return _filter_passes(data, _row_params(data, zoom), low_resolution_table, scratch, "simulate_low_resolution")


class ImageDegradation:
    """Gaussian noise, Gaussian blur and simulated low resolution with nnU-Net's default ranges and probabilities; a range that is
    None switches its transform off.

    noise           (lo, hi) of the STANDARD DEVIATION, one per sample (batchgenerators passes the number it calls a variance to
                    np.random.normal as the scale, so the two agree)
    blur            (lo, hi) of sigma in voxels, one per channel
    low_resolution  (lo, hi) of the zoom factor, one per channel
    p_*             probability that a sample takes the transform;  p_*_channel: that a channel of such a sample does

    draw(channels) makes these calls into numpy's global generator, in this order, whatever the outcome of a probability test --
    a sample always consumes calls_per_sample(channels) of them, each one uniform double:
      noise:           uniform() [p_noise], uniform(lo, hi)                                            2 calls
      blur:            uniform() [p_blur], then per channel uniform() [p_blur_channel], uniform(lo, hi)  1 + 2 C calls
      low resolution:  the same with its own probabilities                                              1 + 2 C calls
    The noise seed of a batch is drawn by the sampler, not here (DevicePatchSampler.batch)."""

    def __init__(self, noise=(0.0, 0.1), blur=(0.5, 1.0), low_resolution=(0.5, 1.0), p_noise=0.1, p_blur=0.2, p_blur_channel=0.5,
                 p_low_resolution=0.25, p_low_resolution_channel=0.5):
        pair = lambda r: None if r is None else (float(r[0]), float(r[1]))
        self.noise, self.blur, self.low_resolution = pair(noise), pair(blur), pair(low_resolution)
        assert self.noise is None or 0 <= self.noise[0] <= self.noise[1]
        assert self.blur is None or 0 <= self.blur[0] <= self.blur[1]
        assert self.low_resolution is None or 0 < self.low_resolution[0] <= self.low_resolution[1]
        if self.blur is not None:
            blur_table(1, self.blur[1])      # a sigma that needs more than 64 taps is refused here, not in the middle of an epoch
        self.p_noise, self.p_blur, self.p_blur_channel = float(p_noise), float(p_blur), float(p_blur_channel)
        self.p_low_resolution, self.p_low_resolution_channel = float(p_low_resolution), float(p_low_resolution_channel)

    def calls_per_sample(self, channels):
        return 2 * (self.noise is not None) + (1 + 2 * channels) * ((self.blur is not None) + (self.low_resolution is not None))

    def draw(self, channels):
        """One sample: (channels, 3) float64 = (std, sigma, zoom) per channel, (0, 0, 1) where a transform is off."""
        out = np.zeros((channels, 3))
        out[:, 2] = 1.0
        if self.noise is not None:
            take = np.random.uniform() < self.p_noise
            std = np.random.uniform(*self.noise)
            if take:
                out[:, 0] = std
        for col, rng, p, p_channel in ((1, self.blur, self.p_blur, self.p_blur_channel),
                                       (2, self.low_resolution, self.p_low_resolution, self.p_low_resolution_channel)):
            if rng is None:
                continue
            take = np.random.uniform() < p
            for c in range(channels):
                take_c = np.random.uniform() < p_channel
                v = np.random.uniform(*rng)
                if take and take_c:
                    out[c, col] = v
        return out


class DevicePatchSampler:
    """images[i]: C x D x H x W float16/float32, labels[i]: L x D x H x W uint8 (class map last), heatmaps[i] optional uint8
    (numpy arrays or tensors).  `batch(indices)` -> the collated batch dict on the device.

    degrade: an ImageDegradation.  Per sample the draws run position -> spatial -> degradation -> intensity; after the last sample,
    and only if some row of the batch drew noise, ONE further call np.random.randint(0, 2^64, dtype=uint64) draws the batch's noise
    seed.  Per batch the kernels run crop or warp -> noise -> blur -> low resolution -> augment_.  `last_degradation` holds what was
    drawn ({"params": (B, C, 3) = (std, sigma, zoom), "seed": int or None}); the batch dict is unchanged.  degrade=None makes no
    call into numpy's generator and no launch of its own."""

    def __init__(self, images, labels, patch_size, samples_per_subject=1, heatmaps=None, class_probabilities=None,
                 subject_keys=None, device="cuda:0", augment=False, spatial=None, degrade=None):
        self.device = torch.device(device)
        self.spatial = spatial  # a SpatialAugmentation: mednet_warp_patches takes the place of mednet_crop_patches
        self.last_spatial = None
        self.degrade = degrade  # an ImageDegradation: noise, blur, low resolution on 'data' between the crop / warp and augment_
        self.last_degradation = None
        self.augment = augment  # the reference's `transform` (train_seg.py:82-86) on 'data'
        self.last_augmentation = None
        self.patch_size = np.array(patch_size, dtype=int)
        self.samples_per_subject = samples_per_subject
        self.subject_keys = subject_keys if subject_keys is not None else [str(i) for i in range(len(images))]
        assert len(images) == len(labels)
        self._labels_host = [np.asarray(l) for l in labels]        # the position sampling reads label columns on the host
        self.images = [torch.as_tensor(np.asarray(v)).to(self.device).contiguous() for v in images]
        self.labels = [torch.as_tensor(np.asarray(v)).to(self.device).contiguous() for v in labels]
        self.heatmaps = None if heatmaps is None else [torch.as_tensor(np.asarray(v)).to(self.device).contiguous() for v in heatmaps]
        self.class_probabilities = class_probabilities
        self._label_ax2_any = []
        if class_probabilities:
            self.class_probabilities = class_probabilities / np.sum(class_probabilities)
            for lab in self._labels_host:
                self._label_ax2_any.append([np.any(lab[-1, ...] == c, axis=2) for c in range(len(class_probabilities))])

    def __len__(self):
        return len(self.images) * self.samples_per_subject

    def position(self, idx):
        """(subject, index_ini, selected_class) of dataset.py:286-310 for dataset index idx."""
        idx = idx % len(self.images)
        pos, selected_class = None, 0
        if self.class_probabilities is not None:
            selected_class = np.random.choice(range(len(self.class_probabilities)), p=self.class_probabilities)
            if selected_class > 0:
                pos = get_labeled_position(self._labels_host[idx][-1], selected_class,
                                           label_any=self._label_ax2_any[idx][selected_class])
        ini, _ = get_random_patch_indices(self.patch_size, np.array(self.images[idx].shape[1:]), pos=pos)
        return idx, ini, selected_class

    def batch(self, indices):
        L.require_gpu(self.images[0], "patch sampler")
        plan, aug, warp, deg = [], [], [], []
        for i in indices:  # per sample: position draws, then (optionally) the transform's draws -- the reference's order
            plan.append(self.position(i))
            if self.spatial is not None:  # spatial transforms first, then the intensity ones
                warp.append(self.spatial.draw(plan[-1][1], self.patch_size))
            if self.degrade is not None:
                deg.append(self.degrade.draw(self.images[0].shape[0]))
            if self.augment:
                aug.append(draw_augmentation(self.images[0].shape[0]))
        if self.degrade is not None:
            deg = np.stack(deg)
            seed = int(np.random.randint(0, 2 ** 64, dtype=np.uint64)) if deg[:, :, 0].any() else None
            self.last_degradation = {"params": deg, "seed": seed}
        b = len(plan)
        pd, ph, pw = (int(v) for v in self.patch_size)
        c_img = self.images[0].shape[0]
        n_hm = 0 if self.heatmaps is None else self.heatmaps[0].shape[0]
        n_lab = self.labels[0].shape[0]
        data = torch.empty((b, c_img, pd, ph, pw), dtype=torch.float32, device=self.device)
        label = torch.empty((b, n_hm + n_lab, pd, ph, pw), dtype=torch.uint8, device=self.device)
        if self.spatial is not None:
            self._warp_batch(plan, warp, data, label, n_hm)
        else:
            self._crop_batch(plan, data, label, n_hm, n_lab)
        if self.degrade is not None:
            data = self._degrade_batch(data)
        if self.augment:
            self.last_augmentation = np.stack(aug)
            augment_(data, self.last_augmentation)
        out = {"subject_key": [self.subject_keys[p[0]] for p in plan],
               "patch_position": np.stack([p[1] for p in plan]), "selected_class": np.array([int(p[2]) for p in plan]),
               "data": data, "label": label}
        if self.spatial is not None:
            out["spatial"] = self.last_spatial["affine"]
        return out

    def _degrade_batch(self, data):
        """noise -> blur -> low resolution with last_degradation; a transform that no row drew launches nothing."""
        prm, seed = self.last_degradation["params"], self.last_degradation["seed"]
        if seed is not None:
            gaussian_noise_(data, prm[:, :, 0], seed)
        scratch = torch.empty_like(data) if (prm[:, :, 1] != 0).any() or (prm[:, :, 2] < 1).any() else None
        for run, values in ((gaussian_blur, prm[:, :, 1]), (simulate_low_resolution, prm[:, :, 2])):
            out = run(data, values, scratch)
            if out is not data:
                data, scratch = out, data
        return data

    def _crop_batch(self, plan, data, label, n_hm, n_lab):
        lib = L.lib()
        c_img = data.shape[1]
        pd, ph, pw = data.shape[2:]
        for subj in sorted({p[0] for p in plan}):
            slots = [k for k, p in enumerate(plan) if p[0] == subj]
            pos = torch.tensor(np.stack([plan[k][1] for k in slots]).astype(np.int32), device=self.device)
            slot = torch.tensor(slots, dtype=torch.int32, device=self.device)
            jobs = [(self.images[subj], data, L.F32, c_img, 0)]
            if n_hm:
                jobs.append((self.heatmaps[subj], label, L.U8, n_hm + n_lab, 0))
            jobs.append((self.labels[subj], label, L.U8, n_hm + n_lab, n_hm))
            for vol, out, dst, c_total, c_off in jobs:
                c, d, h, w = vol.shape
                L.check(lib.mednet_crop_patches(vol.data_ptr(), _DT[vol.dtype], pos.data_ptr(), slot.data_ptr(), len(slots),
                                                out.data_ptr(), dst, c, d, h, w, c_total, c_off, pd, ph, pw, L.stream()),
                        "crop_patches")

    def _warp_batch(self, plan, warp, data, label, n_hm):
        """The crop loop of batch() with mednet_warp_patches: per subject one call for the image, the heat maps and the labels."""
        sp = self.spatial
        affine = np.stack([a for a, _ in warp])
        lattice = None if sp.elastic is None else np.stack([g for _, g in warp])
        self.last_spatial = {"affine": affine.reshape(-1, 3, 4), "lattice": lattice}
        for subj in sorted({p[0] for p in plan}):
            slots = [k for k, p in enumerate(plan) if p[0] == subj]
            slot = torch.tensor(slots, dtype=torch.int32, device=self.device)
            aff = torch.tensor(affine[slots], device=self.device)
            disp = None if lattice is None else torch.tensor(lattice[slots], device=self.device)
            warp_patches(self.images[subj], aff, slot, data, 0, "linear", sp.border_data, sp.data_cval, disp)
            if n_hm:
                warp_patches(self.heatmaps[subj], aff, slot, label, 0, "linear", sp.border_label, sp.label_cval, disp)
            warp_patches(self.labels[subj], aff, slot, label, n_hm, "nearest", sp.border_label, sp.label_cval, disp)
