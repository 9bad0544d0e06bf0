"""Blended sliding-window inference restated in numpy fp64, with the checkers of tests/test_gpu_blend_predict.py.

`Blend64` is what mednet_blend_accumulate computes, taken literally: the patches in row order, a patch covering the volume voxels
[pos - ov, pos - ov + patch), what lies outside the volume dropped, the weight (win0[z] * win1[y]) * win2[x] formed in fp32 (the C ABI
fixes that association; everything after it is fp64), looked up at the UNMIRRORED patch coordinate, the logits of a mirrored pass
flipped back first, one softmax per voxel per patch ("probabilities") or the raw class logits ("logits").  Next to acc and wsum it keeps
what the bounds need: norm = the sum of the absolute terms of every accumulator element, cnt = the number of terms of a voxel.
`finalize64` and `peaks64` restate the other two entries.  `Blend32` is the same composition in fp32 ATen ops on the CPU: its error
against Blend64 is the yardstick of the bounds (profiles/blend_bounds.md).

`fault=` injects the mistakes the checkers are there for (tests/test_blend_util.py shows that each is rejected):
  drop_last_row     the last row of every batch is not added
  no_flip_back      the logits of a mirrored pass are added as they come
  swap_weight_axes  the weight table is indexed with the y and x coordinates exchanged
  wsum_per_batch    the weight sum is counted once per batch instead of once per patch
  no_clip           the overhang behind the volume is not dropped: it wraps into the next line / plane through the flat index
  unnormalised      finalize does not divide by the weight sum
"""
import numpy as np
import torch

FAULTS = ("drop_last_row", "no_flip_back", "swap_weight_axes", "wsum_per_batch", "no_clip", "unnormalised")
U32 = 2.0 ** -24          # half an ulp of fp32, relative
U16 = 2.0 ** -11          # half an ulp of fp16, relative
TINY16 = 2.0 ** -25       # half the spacing of fp16's subnormals
FP32_EXACT = float(2 ** 24)

# the smallest shapes at which the kernels can still go wrong: three distinct axes, 80 patches of 1536 voxels (6 workgroups), 1-8-fold
# coverage, two grid rows on axes 0 and 1 and one on axis 2 hanging over the volume's far end
PATCH, OVERLAP, VOLUME = (8, 12, 16), (2, 3, 4), (13, 19, 37)


def grid_positions(vol, patch, ov):
    step = np.asarray(patch) - 2 * np.asarray(ov)
    n = np.ceil(np.asarray(vol) / step).astype(int)
    axes = [np.arange(n[k]) * step[k] for k in range(3)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int32)


def pow2_windows(patch):
    """2^min(i, p - 1 - i, 3) per axis: every product and partial sum of integer data stays exact in fp32."""
    return tuple((2.0 ** np.minimum(np.minimum(np.arange(p), p - 1 - np.arange(p)), 3)).astype(np.float32) for p in patch)


def gaussian_windows(patch, sigma_scale=0.125):
    out = []
    for p in patch:
        i = np.arange(p, dtype=np.float64)
        out.append(np.exp(-0.5 * ((i - (p - 1) / 2.0) / (sigma_scale * p)) ** 2).astype(np.float32))
    return tuple(out)


def flip(a, mask, first):
    """Reverse axis first + k of `a` for every bit k of mask."""
    axes = [first + k for k in range(3) if mask >> k & 1]
    return np.flip(a, axes) if axes else a


def weight32(windows, fault=None):
    """The fp32 weight of every patch voxel in the ABI's association."""
    w0, w1, w2 = (np.asarray(w, dtype=np.float32) for w in windows)
    w = (w0[:, None, None] * w1[None, :, None]) * w2[None, None, :]
    assert w.dtype == np.float32
    if fault == "swap_weight_axes":
        w = np.ascontiguousarray(w.transpose(0, 2, 1)).reshape(w.shape)
    return w


def softmax64(x, axis=0):
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def _window(start, patch, vol):
    """Per axis: the slice of the patch that lies inside the volume, and the slice of the volume it covers."""
    ps, vs = [], []
    for k in range(3):
        lo, hi = max(0, -int(start[k])), min(int(patch[k]), int(vol[k]) - int(start[k]))
        ps.append(slice(lo, max(lo, hi)))
        vs.append(slice(int(start[k]) + lo, int(start[k]) + max(lo, hi)))
    return tuple(ps), tuple(vs)


class Blend64:
    def __init__(self, channels, num_heatmaps, vol, patch, ov, windows, blend_of="probabilities", fault=None):
        self.nh, self.vol, self.patch, self.ov = num_heatmaps, tuple(vol), tuple(patch), tuple(ov)
        self.blend_of, self.fault = blend_of, fault
        self.w = weight32(windows, fault).astype(np.float64)
        self.acc = np.zeros((channels,) + self.vol)
        self.norm = np.zeros((channels,) + self.vol)
        self.wsum = np.zeros(self.vol)
        self.cnt = np.zeros(self.vol, dtype=np.int64)

    def values(self, lg, mirror):
        """What a patch contributes per voxel before weighting, in the volume's orientation."""
        lg = np.asarray(lg, dtype=np.float64)
        if self.fault != "no_flip_back":
            lg = flip(lg, mirror, 1)
        cls = lg[self.nh:] if self.blend_of == "logits" else softmax64(lg[self.nh:])
        return np.concatenate((lg[:self.nh], cls))

    def add(self, logits, pos, mirror=0, batch=None):
        """logits [rows, channels, pd, ph, pw] as the model returns them for patches gathered with `mirror`; the rows in order.
        `batch` only matters to the per-batch faults."""
        n = len(pos)
        batch = n if batch is None else batch
        for b in range(n):
            last = (b + 1) % batch == 0 or b == n - 1
            if self.fault == "drop_last_row" and last:
                continue
            count_w = self.fault != "wsum_per_batch" or b % batch == 0
            t = self.w[None] * self.values(logits[b], mirror)
            start = np.asarray(pos[b]) - np.asarray(self.ov)
            if self.fault == "no_clip":
                self._add_unclipped(t, start, count_w)
                continue
            ps, vs = _window(start, self.patch, self.vol)
            self.acc[(slice(None),) + vs] += t[(slice(None),) + ps]
            self.norm[(slice(None),) + vs] += np.abs(t[(slice(None),) + ps])
            self.cnt[vs] += 1
            if count_w:
                self.wsum[vs] += self.w[ps]
        return self

    def _add_unclipped(self, t, start, count_w):
        d, h, w = self.vol
        g = [start[k] + np.arange(self.patch[k]) for k in range(3)]
        gz, gy, gx = np.meshgrid(*g, indexing="ij")
        flat = (gz * h + gy) * w + gx
        ok = (gz >= 0) & (gy >= 0) & (gx >= 0) & (flat < d * h * w)
        for c in range(self.acc.shape[0]):
            np.add.at(self.acc[c].reshape(-1), flat[ok], t[c][ok])
            np.add.at(self.norm[c].reshape(-1), flat[ok], np.abs(t[c][ok]))
        np.add.at(self.cnt.reshape(-1), flat[ok], 1)
        if count_w:
            np.add.at(self.wsum.reshape(-1), flat[ok], self.w[ok])


def finalize64(acc, wsum, num_heatmaps, blend_of="probabilities", fault=None):
    """-> heat [nh, ..], prob [classes, ..] (fp64), result uint8 [(nh + 1), ..] in the crop-stitch predictor's layout."""
    acc, wsum = np.asarray(acc, dtype=np.float64), np.asarray(wsum, dtype=np.float64)
    live = wsum != 0
    mean = acc if fault == "unnormalised" else np.where(live, acc / np.where(live, wsum, 1.0), 0.0)
    heat, cls = mean[:num_heatmaps], mean[num_heatmaps:]
    prob = np.where(live, softmax64(cls), 0.0) if blend_of == "logits" else cls
    result = np.concatenate((np.clip(heat, 0, 255).astype(np.uint8), np.where(live, acc[num_heatmaps:].argmax(0), 0)[None].astype(np.uint8)))
    return heat, prob, result


def peaks64(heat):
    """Per channel the flat index of the maximum (the first on ties, NaN never wins; -1 and -inf for a channel of NaNs) and its value."""
    h = np.asarray(heat).reshape(len(heat), -1)
    idx, val = [], []
    for row in h:
        seen = np.where(np.isnan(row), -np.inf, row)
        if np.isnan(row).all():
            idx.append(-1)
            val.append(-np.inf)
        else:
            idx.append(int(seen.argmax()))
            val.append(row[idx[-1]])
    return np.asarray(idx, dtype=np.int64), np.asarray(val)


# ---------------------------------------------------------------------------------------------- ATen's fp32 composition
class Blend32:
    """Blend64's loop in fp32 torch ops on the CPU: the weight product, torch.softmax, w * value and the additions all round to fp32."""

    def __init__(self, channels, num_heatmaps, vol, patch, ov, windows, blend_of="probabilities"):
        self.nh, self.vol, self.patch, self.ov, self.blend_of = num_heatmaps, tuple(vol), tuple(patch), tuple(ov), blend_of
        w0, w1, w2 = (torch.from_numpy(np.asarray(w, dtype=np.float32)) for w in windows)
        self.w = (w0[:, None, None] * w1[None, :, None]) * w2[None, None, :]
        self.acc = torch.zeros((channels,) + self.vol, dtype=torch.float32)
        self.wsum = torch.zeros(self.vol, dtype=torch.float32)

    def add(self, logits, pos, mirror=0):
        for b in range(len(pos)):
            lg = torch.from_numpy(np.ascontiguousarray(flip(np.asarray(logits[b], dtype=np.float32), mirror, 1)))
            cls = lg[self.nh:] if self.blend_of == "logits" else torch.softmax(lg[self.nh:], 0)
            t = self.w[None] * torch.cat((lg[:self.nh], cls))
            ps, vs = _window(np.asarray(pos[b]) - np.asarray(self.ov), self.patch, self.vol)
            self.acc[(slice(None),) + vs] += t[(slice(None),) + ps]
            self.wsum[vs] += self.w[ps]
        return self


# ---------------------------------------------------------------------------------------------- bounds and checkers
def r32_of(x32, x64, norm):
    """ATen's fp32 error in the norm of the bound: max |x32 - x64| / norm (an element without terms must be 0 in both)."""
    x32, x64, norm = np.asarray(x32, dtype=np.float64), np.asarray(x64, dtype=np.float64), np.asarray(norm, dtype=np.float64)
    dead = norm == 0
    assert not (np.abs(x32 - x64)[dead] != 0).any(), "the fp32 and fp64 references differ where the bound's norm is 0"
    return float((np.abs(x32 - x64)[~dead] / norm[~dead]).max()) if (~dead).any() else 0.0


def eps_of(r32, cnt):
    """The relative error (in the sum of absolute terms) admitted to a sum of cnt terms: four times ATen's fp32 error plus half an
    ulp for each of the cnt additions."""
    return 4.0 * r32 + np.asarray(cnt, dtype=np.float64) * U32


def quotient_bound(ref, norm, wsum, eps_a, eps_w, half=False):
    """|got - ref| for got = fl(acc / wsum): acc within eps_a * norm, wsum within eps_w * wsum, the division rounds once (fp32);
    half=True: and once more to fp16."""
    ref, wsum = np.abs(np.asarray(ref, dtype=np.float64)), np.asarray(wsum, dtype=np.float64)
    live = wsum != 0
    safe = np.where(live, wsum, 1.0)
    b = np.where(live, (eps_a * norm / safe + ref * eps_w) / (1.0 - eps_w), 0.0)
    b = b + U32 * (ref + b)
    if half:
        b = b + U16 * (ref + b) + TINY16
    return b


def softmax_bound(prob, delta, r32_sm, half=False):
    """|got - prob| for got = softmax32(m), every m_k within delta_k of the fp64 mean logit: a softmax moves by at most
    p (e^(2 max delta) - 1); its own evaluation is held to four times ATen's fp32 softmax error plus four roundings."""
    prob = np.asarray(prob, dtype=np.float64)
    b = prob * np.expm1(2.0 * np.asarray(delta).max(axis=0)) + (4.0 * r32_sm + 4.0 * U32) * prob
    if half:
        b = b + U16 * (prob + b) + TINY16
    return b


def assert_exact_premise(norm, unit, what):
    """Every term is a multiple of `unit` and the sum of the absolute terms of every element stays below 2^24 units: each fp32
    product and partial sum is exact in any order."""
    steps = np.asarray(norm, dtype=np.float64) / unit
    assert (steps == np.round(steps)).all(), f"{what}: terms are no multiples of {unit}"
    assert steps.max() < FP32_EXACT, f"{what}: the sum of |terms| reaches {steps.max():.4g} steps >= 2^24"


def _first(bad, got, ref, extra=None, first=6):
    out = []
    for i in np.argwhere(bad)[:first]:
        i = tuple(i.tolist())
        out.append(f"{i}: got {got[i]!r} want {ref[i]!r}" + ("" if extra is None else f" bound {extra[i]:.3e}"))
    return " | ".join(out)


def check_exact(got, ref, what):
    """Every element equals the fp64 restatement (a NaN or an unwritten element counts as a difference)."""
    got, ref = np.asarray(got).astype(np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    bad = ~(got == ref)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {got.size} elements differ; first at " + _first(bad, got, ref)
    return got.size


def check_values(got, ref, bound, what):
    """Every element, none left out: |got - ref| <= bound, no NaN.  -> the worst observed |got - ref| / bound."""
    got, ref, bound = np.asarray(got).astype(np.float64), np.asarray(ref, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    bound = np.broadcast_to(bound, ref.shape)
    nan = int(np.isnan(got).sum())
    assert nan == 0, f"{what}: {nan} of {got.size} elements are NaN (not written)"
    diff = np.abs(got - ref)
    bad = diff > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} of {got.size} elements outside the bound; first at " + _first(bad, got, ref, bound)
    live = bound > 0
    return float((diff[live] / bound[live]).max()) if live.any() else 0.0


def check_one_ulp(got32, q64, what):
    """fp32 `got` within one ulp (the spacing of fp32 at |q|) of the fp64 quotient q."""
    got32, q64 = np.asarray(got32, dtype=np.float32), np.asarray(q64, dtype=np.float64)
    ulp = np.spacing(np.abs(q64).astype(np.float32)).astype(np.float64)
    return check_values(got32, q64, ulp, what)


# ---------------------------------------------------------------------------------------------- inputs
def exact_logits(rows, num_heatmaps, ncls, patch, blend_of, seed=0):
    """Heat maps: small integers encoding (row, z) and (y, x); class logits: all equal (softmax is exactly 1 / ncls for ncls in
    1, 2, 4) or, for blend_of="logits", integers in [-8, 8]."""
    pd, ph, pw = patch
    z, y, x = np.meshgrid(np.arange(pd), np.arange(ph), np.arange(pw), indexing="ij")
    lg = np.zeros((rows, num_heatmaps + ncls, pd, ph, pw), dtype=np.float32)
    for b in range(rows):
        planes = (b * pd + z, y * pw + x)
        for k in range(num_heatmaps):
            lg[b, k] = planes[k % 2] + k // 2
    if blend_of == "logits":
        lg[:, num_heatmaps:] = np.random.Generator(np.random.PCG64(seed)).integers(-8, 9, size=lg[:, num_heatmaps:].shape)
    else:
        lg[:, num_heatmaps:] = 3.0
    return lg


def random_logits(rows, channels, patch, seed, scale=3.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return (g.standard_normal((rows, channels) + tuple(patch)) * scale).astype(np.float32)


# the pointwise stub model of the end-to-end test: logits_c = a_c x + b_c, heat map k = (k + 1) x
STUB_A = (1.0, -1.0, 0.5, -0.5, 0.25)
STUB_B = (0.0, 1 / 16, 1 / 32, -3 / 32, 1 / 64)


def lattice_volume(vol, seed):
    """One channel, a random draw from the multiples of 1/8 in [-2, 2] (exact in fp16)."""
    g = np.random.Generator(np.random.PCG64(seed))
    return (g.integers(-16, 17, size=(1,) + tuple(vol)) / 8.0).astype(np.float16)


def stub_logits64(x, num_heatmaps):
    """x [..] -> [num_heatmaps + 5, ..] fp64: what the stub returns for a voxel of value x."""
    x = np.asarray(x, dtype=np.float64)
    return np.stack([(k + 1) * x for k in range(num_heatmaps)] + [a * x + b for a, b in zip(STUB_A, STUB_B)])
