"""mednet_warp_patches without a GPU: the arithmetic of include/mednet_hip.h restated in numpy, the test cases, and the checkers.

`warp_model(..., prec="f64")` is the fp64 restatement (tests/test_warp_util.py holds it against scipy.ndimage.map_coordinates);
`prec="f32"` follows the header's fp32 association operation by operation (fmaf = one rounding of the exact product-sum, made in
fp64: a double rounding is possible once in about 2^29 operations and only matters to the bit comparisons, whose operands are dyadic
and therefore exact either way).  `fault=` injects one of FAULTS into the model.

A case is a dict (see `make_case`); `run(case)` returns the whole batch tensor B x c_total x pD x pH x pW, prefilled with the canary.
`model_run(fault)` gives such a runner on the CPU model, tests/test_gpu_warp.py has the one that calls the library.  `check_case`
is what both go through:
  * canary: everything outside rows `slots`, channels [c_off, c_off + C) is untouched;
  * kind "exact": the written part equals the fp64 restatement rounded once (to fp32; bytes: rint, nearest-even), bit for bit;
  * kind "bound": profiles/spatial_augment_bounds.md -- linear: every element within eps * norm; nearest: equal wherever the fp64
    coordinate is farther than 2^-12 from a half-integer on every axis, the left-out share at most 1 %; bytes (heat maps): within one
    grey level everywhere and equal wherever the fp64 value is farther than the linear bound from a tie.
"""
import itertools

import numpy as np

U = 2.0 ** -24
EPS_FLOOR = 2.0 ** -20      # sixteen fp32 roundings (derivation: profiles/spatial_augment_bounds.md)
HALF_MARGIN = 2.0 ** -12    # nearest: coordinates this close to a half-integer are left out
LEFT_OUT_CAP = 0.01
CANARY = {np.dtype(np.float32): np.float32(12345.0), np.dtype(np.uint8): np.uint8(0xA5)}
BRICKS = ((4, 8, 8), (4, 4, 16), (2, 4, 32), (1, 1, 256))   # (z, y, x) of the workgroup mappings, option warp_brick 0..3
BRICK = BRICKS[1]           # the default
FAULTS = ("trunc", "centre", "swap_rows", "swap_cols", "swap_w", "no_cval", "edge_coord", "no_lattice", "lattice_after", "hm_trunc",
          "drop_brick")


class WarpCheckError(AssertionError):
    pass


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ------------------------------------------------------------------------------------------------------------ the model
def _fma(prec):
    if prec == "f64":
        return lambda a, b, c: a * b + c
    return lambda a, b, c: (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _clamp(s, n, T):
    s = np.where(s >= T(-2), s, T(-2))          # NaN and everything below
    return np.where(s > T(n + 1), T(n + 1), s)


def _gather(vol, iz, iy, ix, border, cval, T):
    """vol[:, iz, iy, ix] with the border rule -> (C, ...) in T"""
    _, d, h, w = vol.shape
    inside = (iz >= 0) & (iz < d) & (iy >= 0) & (iy < h) & (ix >= 0) & (ix < w)
    v = vol[:, np.clip(iz, 0, d - 1), np.clip(iy, 0, h - 1), np.clip(ix, 0, w - 1)].astype(T)
    return v if border == "edge" else np.where(inside[None], v, T(cval))


def source_coordinates(affine, patch, disp=None, prec="f64", fault=None):
    """(3, pD, pH, pW) source coordinates of one row in T (steps 1-3 of the header)."""
    T = np.float64 if prec == "f64" else np.float32
    fma = _fma(prec)
    lerp = lambda q, a, b: fma(q, b - a, a)
    idx = np.meshgrid(*(np.arange(p) for p in patch), indexing="ij")
    half = [T(p / 2) if fault == "centre" else T((p - 1) * 0.5) for p in patch]
    u = [idx[k].astype(T) - half[k] for k in range(3)]
    A = np.asarray(affine, dtype=T).reshape(3, 4).copy()
    if fault == "swap_rows":
        A[[0, 1]] = A[[1, 0]]
    if fault == "swap_cols":
        A[:, [1, 2]] = A[:, [2, 1]]
    D = None
    if disp is not None and fault != "no_lattice":
        disp = np.asarray(disp, dtype=T)
        cell, q = [], []
        for k in range(3):
            G, p = disp.shape[1 + k], patch[k]
            r = T(G - 1) / T(p - 1) if p > 1 else T(0)
            g = (idx[k].astype(T) * T(r)).astype(T)
            c = np.minimum(np.floor(g).astype(np.int64), G - 2)
            cell.append(c)
            q.append((g - c.astype(T)).astype(T))
        cz, cy, cx = cell
        D = []
        for j in range(3):
            lat = disp[j]
            a = [[lerp(q[2], lat[cz + dz, cy + dy, cx], lat[cz + dz, cy + dy, cx + 1]) for dy in (0, 1)] for dz in (0, 1)]
            D.append(lerp(q[0], lerp(q[1], a[0][0], a[0][1]), lerp(q[1], a[1][0], a[1][1])))
        if fault != "lattice_after":
            u = [(u[j] + D[j]).astype(T) for j in range(3)]
    s = [fma(A[k, 0], u[0], fma(A[k, 1], u[1], fma(A[k, 2], u[2], A[k, 3]))) for k in range(3)]
    if D is not None and fault == "lattice_after":
        s = [(s[k] + D[k]).astype(T) for k in range(3)]
    return np.stack(s).astype(T)


def sample(vol, s, interp, border, cval, prec="f64", fault=None):
    """Steps 4-5: (C, pD, pH, pW) values in T (not yet converted to the output type) from coordinates s (3, ...)."""
    T = np.float64 if prec == "f64" else np.float32
    fma = _fma(prec)
    lerp = lambda q, a, b: fma(q, b - a, a)
    dims = vol.shape[1:]
    if fault == "no_cval":
        cval = 0
    sc = [_clamp(s[k].astype(T), dims[k], T) for k in range(3)]
    if fault == "edge_coord" and border == "constant":
        sc = [np.clip(sc[k], T(0), T(dims[k] - 1)) for k in range(3)]
    if interp == "nearest":
        i = [np.floor((sc[k] + T(0.5)).astype(T)).astype(np.int64) for k in range(3)]
        return _gather(vol, i[0], i[1], i[2], border, cval, T)
    f = [np.trunc(sc[k]) if fault == "trunc" else np.floor(sc[k]) for k in range(3)]
    w = [(sc[k] - f[k]).astype(T) for k in range(3)]
    i = [f[k].astype(np.int64) for k in range(3)]
    if fault == "swap_w":
        w = [w[2], w[1], w[0]]
    tap = lambda dz, dy, dx: _gather(vol, i[0] + dz, i[1] + dy, i[2] + dx, border, cval, T)
    a = [[lerp(w[2][None], tap(dz, dy, 0), tap(dz, dy, 1)) for dy in (0, 1)] for dz in (0, 1)]
    return lerp(w[0][None], lerp(w[1][None], a[0][0], a[0][1]), lerp(w[1][None], a[1][0], a[1][1]))


def to_output(values, out_dtype, interp, fault=None):
    if np.dtype(out_dtype) == np.uint8:
        v = np.floor(values) if (fault == "hm_trunc" and interp == "linear") else np.rint(values)   # np.rint: nearest-even
        return v.astype(np.int64).astype(np.uint8)
    return values.astype(np.float32)


def warp_model(vol, affine, patch, interp, border, cval, disp=None, prec="f32", fault=None):
    """One row: (C, pD, pH, pW) in the output type (prec f32) or the unrounded fp64 values (prec f64)."""
    s = source_coordinates(affine, patch, disp, prec, fault)
    v = sample(vol, s, interp, border, cval, prec, fault)
    if prec == "f64":
        return v
    return to_output(v, np.uint8 if vol.dtype == np.uint8 else np.float32, interp, fault)


def out_dtype(case):
    return np.dtype(np.uint8 if case["vol"].dtype == np.uint8 else np.float32)


def blank_output(case):
    C = case["vol"].shape[0]
    dt = out_dtype(case)
    return np.full((case["batch"], C + 2) + tuple(case["patch"]), CANARY[dt], dtype=dt)


def model_run(fault=None, brick=BRICK):
    def run(case):
        out = blank_output(case)
        C = case["vol"].shape[0]
        for i, slot in enumerate(case["slots"]):
            disp = None if case["disp"] is None else case["disp"][i]
            got = warp_model(case["vol"], case["affine"][i], case["patch"], case["interp"], case["border"], case["cval"], disp, "f32", fault)
            if fault == "drop_brick":
                keep = np.ones(case["patch"], dtype=bool)
                for k, (p, b) in enumerate(zip(case["patch"], brick)):
                    if p % b:
                        sl = [slice(None)] * 3
                        sl[k] = slice(p // b * b, None)
                        keep[tuple(sl)] = False
                got = np.where(keep[None], got, out[slot, 1:1 + C])
            out[slot, 1:1 + C] = got
        return out
    return run


# ------------------------------------------------------------------------------------------------------------ the bound
def coordinate_budget(case, i):
    """C_k (3, pD, pH, pW): the magnitude whose 16 u covers the rounding of source coordinate k (derivation in the profile):
    |t_k| + sum_j |A_kj| (|u_j| + Dmax (2 + gmax)), with Dmax the largest displacement and gmax the largest lattice coordinate."""
    A = np.asarray(case["affine"][i], np.float64).reshape(3, 4)
    patch = case["patch"]
    idx = np.meshgrid(*(np.arange(p) for p in patch), indexing="ij")
    u = [np.abs(idx[k] - (patch[k] - 1) / 2) for k in range(3)]
    extra = 0.0
    if case["disp"] is not None:
        d = np.asarray(case["disp"][i], np.float64)
        extra = np.abs(d).max() * (2 + max(d.shape[1:]) - 1)
    return np.stack([abs(A[k, 3]) + sum(abs(A[k, j]) * (u[j] + extra) for j in range(3)) for k in range(3)])


def cell_differences(vol, s64, border, cval):
    """G_k (3, C, pD, pH, pW): the largest |finite difference along axis k| over the cell of s64 and its face neighbours, in the volume
    extended by the border rule."""
    P = 4
    dims = vol.shape[1:]
    v = vol.astype(np.float64)
    pad = [(0, 0)] + [(P, P)] * 3
    v = np.pad(v, pad, mode="edge") if border == "edge" else np.pad(v, pad, mode="constant", constant_values=float(cval))
    f = [np.floor(_clamp(s64[k], dims[k], np.float64)).astype(np.int64) + P for k in range(3)]
    out = []
    for k in range(3):
        dk = np.abs(np.diff(v, axis=1 + k))
        best = np.zeros((vol.shape[0],) + s64.shape[1:])
        rng = [(-1, 0, 1, 2)] * 3
        rng[k] = (-1, 0, 1)
        for off in itertools.product(*rng):
            best = np.maximum(best, dk[:, f[0] + off[0], f[1] + off[1], f[2] + off[2]])
        out.append(best)
    return np.stack(out)


def reference(case):
    """Per row: (s64 (3, ...), ref64 (C, ...)); cached on the case and never modified."""
    if "_ref" not in case:
        rows = []
        for i in range(len(case["slots"])):
            disp = None if case["disp"] is None else case["disp"][i]
            s = source_coordinates(case["affine"][i], case["patch"], disp, "f64")
            rows.append((s, sample(case["vol"], s, case["interp"], case["border"], case["cval"], "f64")))
        case["_ref"] = rows
    return case["_ref"]


def norms(case):
    if "_norm" not in case:
        out = []
        for i, (s, ref) in enumerate(reference(case)):
            G = cell_differences(case["vol"], s, case["border"], case["cval"])
            Ck = coordinate_budget(case, i)
            out.append(((Ck[:, None] + 1.0) * G).sum(axis=0) + np.abs(ref))
        case["_norm"] = out
    return case["_norm"]


def worst_ratio(case, out):
    """max |got - ref64| / norm over every element of a linear float case (0 / 0 counts as 0)."""
    C = case["vol"].shape[0]
    worst = 0.0
    for i, slot in enumerate(case["slots"]):
        err = np.abs(out[slot, 1:1 + C].astype(np.float64) - reference(case)[i][1])
        n = norms(case)[i]
        if not np.all(np.isfinite(err)):
            return np.inf
        bad = (n == 0) & (err > 0)
        if bad.any():
            return np.inf
        worst = max(worst, float(np.max(np.where(n > 0, err / np.where(n > 0, n, 1), 0))))
    return worst


def model_r32(case):
    if "_r32" not in case:
        case["_r32"] = worst_ratio(case, model_run()(case)) if (case["interp"] == "linear" and out_dtype(case) == np.float32) else 0.0
    return case["_r32"]


def eps_of(case):
    return max(EPS_FLOOR, 8 * model_r32(case))


def left_out(case):
    """nearest: per row the mask of voxels whose fp64 coordinate is within HALF_MARGIN of a half-integer on some axis"""
    masks = []
    for s, _ in reference(case):
        t = s + 0.5
        masks.append((np.abs(t - np.rint(t)) < HALF_MARGIN).any(axis=0))
    return masks


# ------------------------------------------------------------------------------------------------------------ the checks
def check_case(case, out, report=None):
    """Raises WarpCheckError if `out` (the whole batch tensor) is not what the case demands."""
    C = case["vol"].shape[0]
    dt = out_dtype(case)
    if out.dtype != dt or out.shape != blank_output(case).shape:
        raise WarpCheckError(f"{case['name']}: output {out.dtype} {out.shape}")
    untouched = np.ones(out.shape, dtype=bool)
    for slot in case["slots"]:
        untouched[slot, 1:1 + C] = False
    if not np.array_equal(bits(out[untouched]), bits(np.full(int(untouched.sum()), CANARY[dt], dtype=dt))):
        raise WarpCheckError(f"{case['name']}: a voxel outside the rows / channels of the call was written")
    for i, slot in enumerate(case["slots"]):
        got = out[slot, 1:1 + C]
        s64, ref = reference(case)[i]
        if case["kind"] == "exact":
            want = to_output(ref, dt, case["interp"])
            if not np.array_equal(bits(got), bits(want)):
                bad = np.argwhere(got != want)
                raise WarpCheckError(f"{case['name']} row {i}: {len(bad)} voxels differ, first {tuple(bad[0])}: got {got[tuple(bad[0])]}, "
                                     f"want {want[tuple(bad[0])]}")
        elif case["interp"] == "nearest":
            skip = left_out(case)[i]
            share = float(skip.mean())
            if share > LEFT_OUT_CAP:
                raise WarpCheckError(f"{case['name']} row {i}: {share:.4f} of the voxels lie within 2^-12 of a half-integer (cap 1 %)")
            want = to_output(ref, dt, "nearest")
            diff = (got != want) & ~skip[None]
            if diff.any():
                raise WarpCheckError(f"{case['name']} row {i}: {int(diff.sum())} voxels away from every half-integer differ")
            if report is not None:
                report.append(dict(case=case["name"], row=i, left_out=share))
        else:
            err = np.abs(got.astype(np.float64) - ref)
            bound = eps_of(case) * norms(case)[i]
            if dt == np.uint8:     # heat maps
                if np.any(np.abs(got.astype(np.float64) - np.rint(ref)) > 1):
                    raise WarpCheckError(f"{case['name']} row {i}: a heat-map voxel is more than one grey level off")
                tie = np.abs(ref - np.floor(ref) - 0.5)
                clear = tie > bound
                if np.any((got != np.rint(ref).astype(np.uint8)) & clear):
                    raise WarpCheckError(f"{case['name']} row {i}: a heat-map voxel away from a tie is not the rounded fp64 value")
                if report is not None:
                    report.append(dict(case=case["name"], row=i, near_tie=float(1 - clear.mean())))
            else:
                if not np.all(np.isfinite(got)) or np.any(err > bound):
                    k = np.unravel_index(np.argmax(np.where(np.isfinite(err), err - bound, np.inf)), err.shape)
                    raise WarpCheckError(f"{case['name']} row {i}: voxel {k}: |got - ref64| = {err[k]:.3e} > {bound[k]:.3e}")
    if report is not None and case["kind"] == "bound" and case["interp"] == "linear" and dt == np.float32:
        seen = worst_ratio(case, out)
        report.append(dict(case=case["name"], r32=model_r32(case), bound=eps_of(case), seen=seen, ratio=seen / eps_of(case)))


def rejected(case, out):
    try:
        check_case(case, out)
    except WarpCheckError:
        return True
    return False


# ------------------------------------------------------------------------------------------------------------ the cases
VOLUMES = {"v3": (3, 9, 11, 13), "v1": (1, 24, 20, 28), "small": (1, 5, 7, 9)}
PATCHES = {"p1": (4, 5, 7), "p8": (8, 8, 8), "ragged": (5, 9, 19)}
SLOTS, BATCH = [4, 0, 2], 6


def coded_volume(shape, dtype):
    """Every voxel holds its own address (as far as the type can): a wrong voxel names itself."""
    c, d, h, w = shape
    code = np.arange(d * h * w, dtype=np.int64).reshape(d, h, w)
    if np.dtype(dtype) == np.float32:
        return np.stack([code + 100000 * k for k in range(c)]).astype(np.float32)
    if np.dtype(dtype) == np.float16:
        return np.stack([code % 1021 + 256 * k for k in range(c)]).astype(np.float16)
    return np.stack([(code % 251 + 2 * k) % 256 for k in range(c)]).astype(np.uint8)


def random_volume(shape, dtype, rng, what="image"):
    if np.dtype(dtype) == np.uint8:
        return (rng.integers(0, 4, shape) if what == "label" else rng.integers(0, 256, shape)).astype(np.uint8)
    return (rng.standard_normal(shape) * 40 + 100).astype(dtype)


def affine_rows(mats, positions, patch):
    rows = []
    for m, pos in zip(mats, positions):
        t = np.asarray(pos, np.float64) + (np.asarray(patch, np.float64) - 1) / 2
        rows.append(np.concatenate([np.asarray(m, np.float64), t[:, None]], axis=1).astype(np.float32).reshape(12))
    return np.stack(rows)


def make_case(name, kind, vol, patch, affine, interp, border, cval=0.0, disp=None):
    n = len(affine)
    return dict(name=name, kind=kind, vol=vol, patch=tuple(patch), affine=np.asarray(affine, np.float32).reshape(n, 12), interp=interp,
                border=border, cval=cval, disp=None if disp is None else np.asarray(disp, np.float32), slots=SLOTS[:n], batch=BATCH)


def cube_symmetries():
    """The 48 signed axis permutations as 3 x 3 integer matrices."""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            m = np.zeros((3, 3))
            for k in range(3):
                m[k, perm[k]] = signs[k]
            out.append(m)
    return out


def rotation(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = np.array([[cx, -sx, 0], [sx, cx, 0], [0, 0, 1.0]])
    ry = np.array([[cy, 0, -sy], [0, 1.0, 0], [sy, 0, cy]])
    rz = np.array([[1.0, 0, 0], [0, cz, -sz], [0, sz, cz]])
    return rz @ ry @ rx


DT = {"f32": np.float32, "f16": np.float16, "u8": np.uint8}


def identity_cases():
    """Identity affine at integer positions, flush with every face of the volume: the crop."""
    shape, patch = VOLUMES["v3"], PATCHES["p1"]
    hi = [n - p for n, p in zip(shape[1:], patch)]
    positions = [(0, 0, 0), tuple(hi), (0, hi[1], 0), (hi[0], 0, hi[2]), (2, 3, 1), (hi[0], hi[1], 0)]
    out = []
    for dt, interp, border in itertools.product(DT, ("linear", "nearest"), ("constant", "edge")):
        vol = coded_volume(shape, DT[dt])
        for half in (0, 1):
            pos = positions[3 * half:3 * half + 3]
            c = make_case(f"identity-{dt}-{interp}-{border}-{half}", "exact", vol, patch, affine_rows([np.eye(3)] * 3, pos, patch), interp,
                      border, cval=7.0)
            c["positions"] = pos
            out.append(c)
    return out


def symmetry_cases():
    shape, patch = VOLUMES["v1"], PATCHES["p8"]
    mats = cube_symmetries()
    out = []
    for dt, interp, border in (("f32", "linear", "edge"), ("u8", "nearest", "constant"), ("f16", "linear", "constant")):
        vol = coded_volume(shape, DT[dt])
        for k in range(0, 48, 3):
            pos = [(k % 17, (5 * k) % 13, (3 * k) % 21), (16, 12, 20), (0, 0, 0)]
            c = make_case(f"symmetry-{dt}-{k}", "exact", vol, patch, affine_rows(mats[k:k + 3], pos, patch), interp, border, cval=3.0)
            c["positions"], c["matrices"] = pos, mats[k:k + 3]
            out.append(c)
    return out


def dyadic_lattice(shape, rng):
    return rng.integers(-6, 7, (3,) + tuple(shape)) / 4.0


def dyadic_cases():
    """Small integers in the volume, dyadic translations / scales / lattices: every fp32 partial is exact in any association."""
    rng = np.random.default_rng(5)
    out = []
    mats = [np.eye(3), np.eye(3) * 2, np.eye(3) * 0.5]
    for vname, pname, lat in (("v3", "p1", (4, 3, 7)), ("v1", "ragged", (3, 3, 19)), ("v3", "p8", None)):
        shape, patch = VOLUMES[vname], PATCHES[pname]
        pos = [(1.5, 2.25, 3.5), (0.25, 0.5, 0.75), (2.5, 1.5, 0.5)]
        disp = None if lat is None else np.stack([dyadic_lattice(lat, rng) for _ in range(3)])
        for dt, interp, border, cval in (("f32", "linear", "constant", -7.5), ("f32", "linear", "edge", 0.0), ("f16", "linear", "edge", 0.0),
                                         ("u8", "linear", "constant", 9.0), ("u8", "nearest", "edge", 0.0), ("u8", "nearest", "constant", 9.0)):
            vol = rng.integers(0, 16, shape).astype(DT[dt])
            out.append(make_case(f"dyadic-{vname}-{pname}-{dt}-{interp}-{border}", "exact", vol, patch, affine_rows(mats, pos, patch), interp,
                             border, cval, disp))
    return out


def outside_cases():
    """Partly and wholly outside, the patch larger than the volume, cval != 0, heat-map ties."""
    rng = np.random.default_rng(6)
    out = []
    shape = VOLUMES["small"]
    for pname in ("p1", "p8", "ragged"):
        patch = PATCHES[pname]
        pos = [(-2.5, 3, 4.25), (40, -50, 3), (-1, -1.5, -3)]
        mats = [np.eye(3), np.eye(3), np.eye(3) * 2]
        for dt, interp, border, cval in (("f32", "linear", "constant", -7.5), ("f32", "linear", "edge", 0.0), ("f16", "linear", "constant", 2.0),
                                         ("u8", "linear", "constant", 9.0), ("u8", "nearest", "constant", 9.0), ("u8", "nearest", "edge", 0.0)):
            vol = rng.integers(0, 16, shape).astype(DT[dt])
            out.append(make_case(f"outside-{pname}-{dt}-{interp}-{border}", "exact", vol, patch, affine_rows(mats, pos, patch), interp, border, cval))
    # ties: neighbours along x differ by an odd number, a translation of 1/2 along x lands on k + 1/2
    vol = (np.arange(9)[None, None, None, :] * 3 + np.arange(7)[None, None, :, None] * 2 + np.arange(5)[None, :, None, None]).astype(np.uint8)
    out.append(make_case("outside-ties-u8", "exact", vol, PATCHES["p1"], affine_rows([np.eye(3)] * 3, [(0, 0, 0.5), (1, 2, 1.5), (-1, 1, -0.5)], PATCHES["p1"]),
                     "linear", "constant", 4.0))
    return out


def random_affines(rng, n, patch, shape, zoom=(0.8, 1.25), spread=1.0):
    mats, pos = [], []
    for _ in range(n):
        m = rotation(*rng.uniform(-0.6, 0.6, 3)) * rng.uniform(*zoom)
        if rng.uniform() < 0.5:
            m[:, rng.integers(0, 3)] *= -1
        mats.append(m)
        room = np.asarray(shape[1:]) - np.asarray(patch)
        pos.append(rng.uniform(-2 * spread, room + 2 * spread))
    return affine_rows(mats, pos, patch)


def bound_cases():
    """Random rotations, scales and lattices, held to fp64.  The seeds of the nearest cases were chosen on the CPU so that the share
    of voxels near a half-integer is under the cap (check_case asserts it)."""
    out = []
    plan = [("v3", "p1", False, 11), ("v1", "ragged", True, 12), ("v1", "p8", True, 13), ("small", "p8", False, 14)]
    for vname, pname, lattice, seed in plan:
        shape, patch = VOLUMES[vname], PATCHES[pname]
        for dt, interp, border, cval, what in (("f32", "linear", "edge", 0.0, "image"), ("f32", "linear", "constant", -3.0, "image"),
                                               ("f16", "linear", "edge", 0.0, "image"), ("u8", "linear", "constant", 0.0, "heat"),
                                               ("u8", "nearest", "constant", 2.0, "label")):
            rng = np.random.default_rng(seed)
            vol = random_volume(shape, DT[dt], rng, "label" if what == "label" else "image")
            aff = random_affines(rng, 3, patch, shape)
            disp = None
            if lattice:
                g = tuple(int(np.ceil(p / 4)) + 1 for p in patch)
                disp = rng.normal(0, 1.5, (3, 3) + g)
            out.append(make_case(f"random-{vname}-{pname}-{dt}-{interp}-{border}", "bound", vol, patch, aff, interp, border, cval, disp))
    return out


def footprint_cases():
    """Rotations that reach every face, a 2x zoom-out (most taps outside), both borders."""
    rng = np.random.default_rng(21)
    out = []
    shape, patch = VOLUMES["v3"], PATCHES["ragged"]
    centre = (np.asarray(shape[1:]) - np.asarray(patch)) / 2
    for border in ("constant", "edge"):
        mats = [rotation(0.7, -0.5, 0.9), rotation(-0.4, 0.8, -0.6), np.eye(3) * 2.0]
        g = tuple(int(np.ceil(p / 4)) + 1 for p in patch)
        disp = rng.normal(0, 1.5, (3, 3) + g)
        for dt, interp in (("f32", "linear"), ("u8", "nearest")):
            vol = random_volume(shape, DT[dt], rng, "label" if dt == "u8" else "image")
            out.append(make_case(f"footprint-{dt}-{border}", "bound", vol, patch, affine_rows(mats, [centre] * 3, patch), interp, border, 1.0, disp))
    return out


def nonfinite_case(border):
    """Matrices holding 2^30 and a NaN: cval under the constant border, a defined volume voxel under the edge border."""
    shape, patch = VOLUMES["v3"], PATCHES["p1"]
    rows = affine_rows([np.eye(3) * 2.0 ** 30, np.eye(3), np.eye(3)], [(1, 1, 1)] * 3, patch)
    rows[1, 5] = np.nan          # A[1][1]: every y coordinate of row 1 is NaN
    rows[2, 3] = -np.inf         # t[0] of row 2
    return make_case(f"nonfinite-{border}", "exact", coded_volume(shape, np.float32), patch, rows, "linear", border, cval=-2.0)


_ALL = None


def all_cases():
    """Every case that runs on the GPU with the shared checker (built once; the references are cached on the cases)."""
    global _ALL
    if _ALL is None:
        _ALL = identity_cases() + symmetry_cases() + dyadic_cases() + outside_cases() + bound_cases() + footprint_cases()
    return _ALL
