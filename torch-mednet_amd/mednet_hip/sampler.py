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
same launches and the same generator calls as before."""
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


class DevicePatchSampler:
    """images[i]: C x D x H x W float16/float32, labels[i]: L x D x H x W uint8 (class map last), heatmaps[i] optional uint8
    (numpy arrays or tensors).  `batch(indices)` -> the collated batch dict on the device."""

    def __init__(self, images, labels, patch_size, samples_per_subject=1, heatmaps=None, class_probabilities=None,
                 subject_keys=None, device="cuda:0", augment=False, spatial=None):
        self.device = torch.device(device)
        self.spatial = spatial  # a SpatialAugmentation: mednet_warp_patches takes the place of mednet_crop_patches
        self.last_spatial = None
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
        plan, aug, warp = [], [], []
        for i in indices:  # per sample: position draws, then (optionally) the transform's draws -- the reference's order
            plan.append(self.position(i))
            if self.spatial is not None:  # spatial transforms first, then the intensity ones
                warp.append(self.spatial.draw(plan[-1][1], self.patch_size))
            if self.augment:
                aug.append(draw_augmentation(self.images[0].shape[0]))
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
        if self.augment:
            self.last_augmentation = np.stack(aug)
            augment_(data, self.last_augmentation)
        out = {"subject_key": [self.subject_keys[p[0]] for p in plan],
               "patch_position": np.stack([p[1] for p in plan]), "selected_class": np.array([int(p[2]) for p in plan]),
               "data": data, "label": label}
        if self.spatial is not None:
            out["spatial"] = self.last_spatial["affine"]
        return out

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
