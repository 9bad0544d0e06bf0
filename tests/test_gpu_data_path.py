"""The kernels on either side of the training step and of the network at inference time, at operator level (-m gpu):
csrc/augment.hip (aug_minmax / aug_finalize1 / aug_sum / aug_finalize2 / aug_apply) and csrc/predict.hip (crop_patches, grid_gather,
predict_assemble), through the C ABI and through sampler.augment_, predict.gather_patches, predict.assemble.

A. Augmentation on a two-valued lattice (gpu_util.aug_lattice_case): the statistics are read through the output, bit for bit --
   contrast factor 0 writes the channel mean f32(S / count) into every voxel, factor 2^40 sends every voxel to its channel's lo or hi;
   the identity parameters, a constant channel and a sample whose range comes from two channels likewise.
B. Augmentation on random data against gpu_util.augment_ref64, every element: |got - ref64| <= eps_case * norm, eps_case =
   max(2^-20, 8 * r32), r32 from oracle/ref_augment.apply (numpy fp32) on the same case (profiles/data_path_bounds.md).
C. The refusals of mednet_augment_patches; 64 channels with a workspace of exactly mednet_augment_ws_bytes, NaN-filled.
D. mednet_crop_patches, all three dtype pairs, into a canary-filled batch tensor; its refusals.
E. mednet_grid_gather against np.pad + slicing, both pad modes, bit for bit.
F. mednet_predict_assemble against oracle/ref_predict.postprocess + add_processed_batch on a canary-filled result, including windows
   of ONE launch that overlap (o0 > o1: the later row wins, in grid order and reversed) and GridPredictor at two batch sizes.
Every augmentation case prints one `[exact] item=data_path ...` line.  tests/test_data_path_util.py is the CPU side."""
import functools

import numpy as np
import pytest
import torch

from mednet_hip import _lib as L
from mednet_hip import predict as HP
from mednet_hip import sampler as HS
from oracle import ref_predict as P

import gpu_util as U
from gpu_util import DEV

pytestmark = pytest.mark.gpu
E_SHAPE, E_DTYPE, E_WORKSPACE = -1, -2, -3
SHAPES = {"tiny": (3, 7, 11),       # 231 voxels: fewer than one workgroup's threads
          "block": (8, 16, 16),     # 2048: exactly one block
          "plus1": (1, 3, 683),     # 2049: a second block holding one voxel
          "three": (5, 21, 41),     # 4305: three blocks, the last ragged
          "trip2": (1, 3, 43691)}   # 131 073: 65 partials -- the second trip of both finalize loops, the last block one voxel
# key, batch, channels of the lattice cases (A) -- 64 channels once, at the smallest shape
LATTICE_CASES = [("tiny", 3, 3), ("tiny", 1, 64), ("block", 2, 1), ("plus1", 1, 2), ("three", 3, 2), ("trip2", 2, 3)]
GAMMAS = (0.7, 1.0, 1.3)
CORNERS = [(0.9, 0.7, 0.3), (-0.9, 1.3, 1.7), (0.9, 1.3, 0.3), (-0.9, 0.7, 1.7)]    # shift, gamma, factor
# key, batch, channels, kind, params of the random cases (B)
RANDOM_CASES = [("tiny", 3, 2, "positive", "drawn"), ("tiny", 2, 3, "negative", "drawn"), ("tiny", 2, 2, "scaled", "drawn"),
                ("tiny", 1, 64, "positive", "drawn")] + [("tiny", 1, 2, "positive", k) for k in range(4)] + [
                ("block", 1, 1, "positive", "drawn"), ("block", 2, 2, "scaled", 1), ("plus1", 2, 2, "negative", 0),
                ("plus1", 1, 3, "positive", "drawn"), ("three", 3, 3, "positive", "drawn"), ("three", 2, 2, "scaled", 2),
                ("three", 2, 2, "negative", 3), ("trip2", 2, 3, "positive", "drawn"), ("trip2", 1, 2, "scaled", 1),
                ("trip2", 1, 2, "negative", "drawn")]


def random_case(key, b, c, kind, prm):
    return U.aug_random_case(f"dp:{key}:{b}:{c}:{kind}:{prm}", b, c, SHAPES[key], kind, prm if isinstance(prm, str) else CORNERS[prm])


@functools.lru_cache(maxsize=None)
def lattice_case(key, b, c):
    return U.aug_lattice_case(f"dp:{key}:{b}:{c}", b, c, SHAPES[key])


def test_shapes_sit_where_the_plan_says():
    v = {k: int(np.prod(s)) for k, s in SHAPES.items()}
    B = U.AUG_BLOCK_VOX
    assert v["tiny"] < 256 and v["block"] == B and v["plus1"] == B + 1
    assert 2 * B < v["three"] < 3 * B and (v["three"] - 2 * B) % 256 != 0
    assert U.aug_blocks(v["trip2"]) == U.AUG_FINALIZE_STRIDE + 1 and v["trip2"] == U.AUG_FINALIZE_STRIDE * B + 1
    assert max(b * c * v[k] * 4 for k, b, c in LATTICE_CASES) < 4 << 20
    for b, c, s in ((1, 1, v["tiny"]), (2, 3, v["trip2"]), (1, 64, v["tiny"])):
        assert L.lib().mednet_augment_ws_bytes(b, c, s) == (b * c * U.aug_blocks(s) * 2 + b * c * 8 + 64) * 4


# ------------------------------------------------------------------------------------------------ device side
def last_error():
    return L.lib().mednet_last_error().decode(errors="replace")


def augment_abi(x, prm, b, c, spatial, ws_bytes=None):
    """mednet_augment_patches on device tensors with a test-owned workspace of exactly mednet_augment_ws_bytes (or ws_bytes), every
    byte 0xFF (fp32 NaN): a partial or a statistic that is read but not written shows.  -> the return code."""
    lib = L.lib()
    need = lib.mednet_augment_ws_bytes(max(b, 1), max(c, 1), max(spatial, 1)) if ws_bytes is None else ws_bytes
    ws = torch.full((max(int(need), 1),), 255, dtype=torch.uint8, device=DEV)
    rc = lib.mednet_augment_patches(x.data_ptr(), prm.data_ptr(), b, c, spatial, ws.data_ptr(), int(need), L.stream())
    torch.cuda.synchronize()
    return rc


def augment(case_x, params, through="abi"):
    """[b, c, S] numpy fp32 -> the augmented copy [b, c, S]; "abi": the C ABI with the exact NaN workspace, "py": sampler.augment_."""
    b, c, S = case_x.shape
    x = torch.from_numpy(np.ascontiguousarray(case_x)).to(DEV)
    if through == "py":
        return HS.augment_(x.reshape(b, c, 1, 1, S), params).reshape(b, c, S).cpu().numpy()
    prm = torch.from_numpy(np.ascontiguousarray(params, dtype=np.float32)).to(DEV)
    rc = augment_abi(x, prm, b, c, S)
    assert rc == 0, last_error()
    return x.cpu().numpy()


# ------------------------------------------------------------------------------------------------ A. exact
@pytest.mark.parametrize("key,b,c", LATTICE_CASES, ids=[f"{k}-{b}x{c}" for k, b, c in LATTICE_CASES])
def test_augment_statistics_on_the_lattice_bit_for_bit(key, b, c):
    case = lattice_case(key, b, c)
    n = 0
    for i, gamma in enumerate(GAMMAS):
        through = "py" if i == 1 else "abi"
        n += U.check_aug_lattice_mean(augment(case.x, U.aug_lattice_params(case, gamma, 0.0), through), case, f"{key} gamma {gamma}")
        n += U.check_aug_lattice_extremes(augment(case.x, U.aug_lattice_params(case, gamma, 2.0 ** 40), through), case, f"{key} gamma {gamma}")
    U.report("data_path", f"A lattice {key} b={b} c={c} gammas={GAMMAS} factor 0 -> mean, 2^40 -> L/H: equal", "augment", n)


@pytest.mark.parametrize("key,b,c", LATTICE_CASES, ids=[f"{k}-{b}x{c}" for k, b, c in LATTICE_CASES])
def test_augment_few_bit_factors_on_the_lattice(key, b, c):
    case = lattice_case(key, b, c)
    for factor in (0.5, 1.5):
        got = augment(case.x, U.aug_lattice_params(case, 1.3, factor))
        off = U.check_aug_lattice_factor(got, case, factor, key)
        U.report("data_path", f"A lattice {key} b={b} c={c} factor={factor} bound=2^-24(|f||g-mean|+|out|) not_bit_equal={off}", "augment", got.size)


@pytest.mark.parametrize("key", list(SHAPES))
def test_augment_identity_parameters_return_the_patch_bit_for_bit(key):
    """Shift 0, gamma 1, factor 1 on {0, 2^k}: fl(fl(0 - mean) + mean) = 0, and fl(fl(H - mean) + mean) is within half a spacing below
    H = 2^k of H, so it rounds to H (profiles/data_path_bounds.md)."""
    case = U.aug_lattice_case(f"dp:ident:{key}", 3, 2, SHAPES[key], lh=[(0, 2), (0, 64), (0, 4096)], shifted=False)
    got = augment(case.x, U.aug_lattice_params(case, 1.0, 1.0, shift=False))
    n = U.assert_exact(torch.from_numpy(got), torch.from_numpy(case.x), f"identity {key}")
    U.report("data_path", f"A identity {key}: equal", "augment", n)


@pytest.mark.parametrize("key", list(SHAPES))
def test_augment_constant_channel_comes_back_unchanged(key):
    """One-channel samples of one value: grange = 0, t = 0 / 1e-7 = 0, g = gmin, mean = g (integers: the sums are exact), lo = hi = g."""
    S = int(np.prod(SHAPES[key]))
    x = np.empty((3, 1, S), dtype=np.float32)
    x[0], x[1], x[2] = -5.0, 0.0, 4096.0
    for gamma in (0.7, 1.3):
        for factor in (0.0, 0.3, 1.7, 2.0 ** 40):
            prm = np.zeros((3, 1, 3), dtype=np.float32)
            prm[:, :, 1], prm[:, :, 2] = gamma, factor
            U.assert_exact(torch.from_numpy(augment(x, prm)), torch.from_numpy(x), f"constant channel {key} gamma {gamma} factor {factor}")


@pytest.mark.parametrize("key", list(SHAPES))
def test_augment_clips_to_the_channel_and_maps_on_the_sample_range(key):
    case = U.aug_two_channel_case(f"dp:two:{key}", 2, SHAPES[key])
    worst = 0.0
    for gamma in (0.7, 1.3):
        prm = np.zeros((2, 2, 3), dtype=np.float32)
        prm[:, :, 0], prm[:, :, 1], prm[:, :, 2] = case.add, gamma, 2.0 ** 40
        ref = U.augment_ref64(case.x, prm)
        r32, eps = U.aug_eps(case.x, prm, ref, "two-channel")
        seen = U.check_aug_two_channel(augment(case.x, prm), case, ref, eps, f"two-channel {key} gamma {gamma}")
        worst = max(worst, seen / eps)
        U.report("data_path", f"A two-channel {key} gamma={gamma} r32={r32:.3e} bound={eps:.3e} seen={seen:.3e}", "augment", case.x.size)
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ B. random data against fp64
@pytest.mark.parametrize("key,b,c,kind,prm", RANDOM_CASES, ids=[f"{k}-{b}x{c}-{kind}-{p}" for k, b, c, kind, p in RANDOM_CASES])
def test_augment_random_data_against_fp64_per_element(key, b, c, kind, prm):
    case = random_case(key, b, c, kind, prm)
    ref = U.augment_ref64(case.x, case.params)
    r32, eps = U.aug_eps(case.x, case.params, ref, f"{key} {kind}")
    got = augment(case.x, case.params, "py" if b == 2 else "abi")
    print(f"[measure] {key} b={b} c={c} {kind} {prm}: r32 {r32:.3e} eps_case {eps:.3e} worst "
          f"{float(np.max(np.abs(got.astype(np.float64) - ref.out) / ref.norm)):.3e}")
    seen = U.check_augment(got, ref, eps, f"augment {key} b={b} c={c} {kind} {prm}")
    U.report("data_path", f"B random {key} b={b} c={c} {kind} params={prm} r32={r32:.3e} bound={eps:.3e} seen={seen:.3e}", "augment", got.size)


# ------------------------------------------------------------------------------------------------ C. refusals
def test_augment_refusals_leave_the_data_alone():
    lib = L.lib()
    S = 231
    x0 = torch.from_numpy(U.aug_random_case("dp:refuse", 1, 65, SHAPES["tiny"]).x).to(DEV)
    prm = torch.ones(65 * 3, dtype=torch.float32, device=DEV)
    need = lib.mednet_augment_ws_bytes(1, 64, S)
    for what, (b, c, s, ws_bytes), code in (("65 channels", (1, 65, S, lib.mednet_augment_ws_bytes(1, 65, S)), E_SHAPE),
                                            ("batch 0", (0, 2, S, need), E_SHAPE), ("spatial 0", (1, 2, 0, need), E_SHAPE),
                                            ("workspace one byte short", (1, 64, S, need - 1), E_WORKSPACE)):
        x = x0.clone()
        rc = augment_abi(x, prm, b, c, s, ws_bytes=ws_bytes)
        assert rc == code, (what, rc)
        assert "augment_patches" in last_error(), (what, last_error())
        assert torch.equal(x, x0), what + ": data was written"
    x = x0.clone()
    assert augment_abi(x, prm, 1, 64, S) == 0, last_error()          # 64 channels, exactly mednet_augment_ws_bytes
    assert not torch.equal(x[:, :64], x0[:, :64]) and torch.equal(x[:, 64], x0[:, 64]) and not bool(torch.isnan(x).any())


# ------------------------------------------------------------------------------------------------ D. crop
CROP_DTYPES = {"f32": (np.float32, torch.float32, L.F32, L.F32), "f16": (np.float16, torch.float32, L.F16, L.F32),
               "u8": (np.uint8, torch.uint8, L.U8, L.U8)}
CROP_CASES = [("ragged", (3, 9, 11, 13), (4, 5, 7)), ("small", (1, 5, 7, 9), (2, 3, 5)), ("whole", (2, 3, 5, 7), (3, 5, 7))]


def coordinate_volume(dims, kind):
    flat = np.arange(int(np.prod(dims)), dtype=np.int64).reshape(dims)
    if kind == "f32":
        return flat.astype(np.float32)                  # the flat index
    if kind == "f16":
        return (flat % 2039).astype(np.float16)         # integers below 2048: fp16 numbers
    return (flat % 251).astype(np.uint8)


def crop_abi(vol, src_code, pos, slot, count, out, dst_code, c, dims, c_total, c_off, patch):
    rc = L.lib().mednet_crop_patches(vol.data_ptr(), src_code, pos.data_ptr(), slot.data_ptr(), count, out.data_ptr(), dst_code, c,
                                     dims[0], dims[1], dims[2], c_total, c_off, patch[0], patch[1], patch[2], L.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("kind", list(CROP_DTYPES))
@pytest.mark.parametrize("tag,dims,patch", CROP_CASES, ids=[c[0] for c in CROP_CASES])
def test_crop_patches_against_numpy_slicing(tag, dims, patch, kind):
    np_src, t_dst, src_code, dst_code = CROP_DTYPES[kind]
    c, sp = dims[0], dims[1:]
    assert len(set(sp)) == 3 and all(v % 2 for v in sp)
    vol = coordinate_volume(dims, kind)
    canary = 201 if kind == "u8" else -7777.0
    slots, c_total, c_off = 6, c + 2, 1
    far = [sp[k] - patch[k] for k in range(3)]
    positions = np.asarray([[0, 0, 0], far, [far[0] // 2, far[1], 0]], dtype=np.int32)
    slot = [4, 0, 2]
    out = torch.full((slots, c_total) + tuple(patch), canary, dtype=t_dst, device=DEV)
    rc = crop_abi(torch.from_numpy(vol).to(DEV), src_code, torch.from_numpy(positions).to(DEV),
                  torch.tensor(slot, dtype=torch.int32, device=DEV), 3, out, dst_code, c, sp, c_total, c_off, patch)
    assert rc == 0, last_error()
    want = np.full((slots, c_total) + tuple(patch), canary, dtype=np.uint8 if kind == "u8" else np.float32)
    for s, p in zip(slot, positions):
        want[s, c_off:c_off + c] = vol[:, p[0]:p[0] + patch[0], p[1]:p[1] + patch[1], p[2]:p[2] + patch[2]]
    got = out.cpu().numpy()
    assert got.dtype == want.dtype and np.array_equal(got, want), f"{tag} {kind}: {int((got != want).sum())} elements differ"


def test_crop_patches_refusals_leave_the_canary():
    dims, patch = (3, 9, 11, 13), (4, 5, 7)
    pos = torch.zeros((1, 3), dtype=torch.int32, device=DEV)
    slot = torch.zeros(1, dtype=torch.int32, device=DEV)
    u8 = torch.from_numpy(coordinate_volume(dims, "u8")).to(DEV)
    f32 = torch.from_numpy(coordinate_volume(dims, "f32")).to(DEV)
    out = torch.full((2, 5) + patch, -7777.0, dtype=torch.float32, device=DEV)
    for what, args, code in (("uint8 -> float", (u8, L.U8, pos, slot, 1, out, L.F32, 3, dims[1:], 5, 1, patch), E_DTYPE),
                             ("patch larger than the volume", (f32, L.F32, pos, slot, 1, out, L.F32, 3, dims[1:], 5, 1, (4, 12, 7)), E_SHAPE),
                             ("c_off + c > c_total", (f32, L.F32, pos, slot, 1, out, L.F32, 3, dims[1:], 5, 3, patch), E_SHAPE),
                             ("count 0", (f32, L.F32, pos, slot, 0, out, L.F32, 3, dims[1:], 5, 1, patch), E_SHAPE)):
        assert crop_abi(*args) == code, what
        assert "crop_patches" in last_error(), (what, last_error())
        assert bool((out == -7777.0).all()), what + ": the batch tensor was written"


# ------------------------------------------------------------------------------------------------ E. gather
# tag, volume (C, D, H, W), patch, overlap
GATHER_CASES = [("three_channels", (3, 5, 6, 7), (6, 6, 8), (1, 2, 2)),
                ("extent_1", (2, 1, 5, 4), (4, 5, 4), (1, 2, 1)),
                ("extent_2_overlap_5", (1, 2, 7, 3), (12, 5, 5), (5, 1, 1)),      # pad of 5 on an axis of 2: more than two periods
                ("overlap_0", (2, 4, 5, 6), (2, 4, 4), (0, 1, 1)),
                ("multiple", (1, 8, 6, 4), (6, 5, 4), (1, 1, 1))]                 # size = 2 x cropped patch: the far pad is a full patch


@pytest.mark.parametrize("mode", ["constant", "symmetric"])
@pytest.mark.parametrize("tag,dims,patch,ov", GATHER_CASES, ids=[c[0] for c in GATHER_CASES])
def test_grid_gather_against_np_pad(tag, dims, patch, ov, mode):
    img = coordinate_volume(dims, "f32") + 1.0            # (no voxel is 0: a constant-mode zero is padding)
    ora = list(P.grid_patch_generator(img, list(patch), list(ov), mode=mode))
    pos = HP.grid_positions(dims[1:], patch, ov)
    assert len(ora) == len(pos) and all(np.array_equal(o[1], p) for o, p in zip(ora, pos))
    if tag == "multiple":
        assert all(dims[1 + k] % (patch[k] - 2 * ov[k]) == 0 for k in range(3))
    got = HP.gather_patches(torch.from_numpy(img).to(DEV), torch.from_numpy(pos).to(DEV), patch, ov, mode).cpu().numpy()
    for i, (p, _, _) in enumerate(ora):
        assert np.array_equal(got[i], p), (tag, mode, i)


@pytest.mark.parametrize("mode", ["constant", "symmetric"])
def test_grid_gather_of_a_patch_wholly_in_the_padding(mode):
    """Positions behind the volume's far end (the kernel maps any padded index: nothing is read out of bounds): np.pad with a far
    pad of three patches; constant mode gives all zeros."""
    dims, patch, ov = (3, 5, 6, 7), (6, 6, 8), (1, 2, 2)
    img = coordinate_volume(dims, "f32") + 1.0
    padded = np.pad(img, [[0, 0]] + [[ov[k], 3 * patch[k]] for k in range(3)], mode=mode)
    pos = np.asarray([[ov[0] + dims[1], 0, 0], [0, ov[1] + dims[2], ov[2] + dims[3]], [ov[0] + dims[1] + 3, ov[1] + dims[2] + 1, ov[2] + dims[3]],
                      [0, 0, 0]], dtype=np.int32)
    got = HP.gather_patches(torch.from_numpy(img).to(DEV), torch.from_numpy(pos).to(DEV), patch, ov, mode).cpu().numpy()
    for i, p in enumerate(pos):
        want = padded[:, p[0]:p[0] + patch[0], p[1]:p[1] + patch[1], p[2]:p[2] + patch[2]]
        assert want.shape == got[i].shape and np.array_equal(got[i], want), (mode, i)
        if mode == "constant" and i < 3:
            assert not got[i].any()


# ------------------------------------------------------------------------------------------------ F. stitch
CANARY = 201
HM_EDGES = np.asarray([-0.0, 0.0, 0.999, 1.0, 254.999, 255.0, 255.999, 256.0, 1e9, -1e9], dtype=np.float32)


def stitch_logits(tag, n, nh, ncls, patch):
    """Heat maps: the clip / truncation edges, cycling, among random values in [-20, 280); class logits: integers in {-1, 0, 1}, so
    two- and three-way ties of the maximum are everywhere (the first maximum wins)."""
    g = U._np_rng("dp:stitch:" + tag)
    lg = np.empty((n, nh + ncls) + tuple(patch), dtype=np.float32)
    hm = (g.random((n, nh) + tuple(patch)) * 300 - 20).astype(np.float32)
    flat = hm.reshape(-1)
    flat[::3] = HM_EDGES[np.arange(len(flat[::3])) % len(HM_EDGES)]
    lg[:, :nh] = hm
    lg[:, nh:] = g.integers(-1, 2, size=(n, ncls) + tuple(patch)).astype(np.float32)
    return lg


def stitch_both(lg, pos, dims, nh, ov):
    """-> (device result, oracle result), both from a result volume filled with CANARY."""
    want = np.full((nh + 1,) + tuple(dims), CANARY, dtype=np.uint8)
    P.add_processed_batch(want, P.postprocess(lg, nh), pos, list(ov))
    got = torch.full((nh + 1,) + tuple(dims), CANARY, dtype=torch.uint8, device=DEV)
    HP.assemble(torch.from_numpy(lg).to(DEV), torch.from_numpy(np.ascontiguousarray(pos, dtype=np.int32)).to(DEV), got, nh, list(ov))
    return got.cpu().numpy(), want


@pytest.mark.parametrize("ncls", [1, 2, 5, 32])
@pytest.mark.parametrize("nh", [0, 3])
def test_stitch_values_ties_and_edges(nh, ncls):
    """A window of 7 x 7 x 10 = 490 voxels (two workgroups, the second ragged); o0 < o1: one plane per patch along axis 0 is written by
    nobody and keeps the canary, as in the reference; the last row lies entirely behind the volume (position = extent on axis 0)."""
    dims, patch, ov = (13, 9, 11), (10, 11, 12), (1, 2, 1)
    start, shape = HP.crop_window(patch, ov)
    assert int(np.prod(shape)) == 490 and shape[0] < patch[0] - 2 * ov[0]
    pos = np.concatenate([HP.grid_positions(dims, patch, ov), np.asarray([[dims[0], 0, 0]], dtype=np.int32)])
    lg = stitch_logits(f"values:{nh}:{ncls}", len(pos), nh, ncls, patch)
    if ncls >= 3:
        lg[:, nh:, 2, 4, 3] = 0.0
        lg[:, nh + 1:nh + 3, 2, 4, 3] = 1.0       # a tie of classes 1 and 2 above class 0 ...
        lg[:, nh:nh + 3, 3, 4, 3] = 1.0           # ... and a three-way tie of the maximum: class 0
    got, want = stitch_both(lg, pos, dims, nh, ov)
    assert (want == CANARY).any() and np.array_equal(got, want), f"{int((got != want).sum())} voxels differ"
    if nh:
        assert {0, 1, 254, 255} <= set(np.unique(want[:nh]).tolist())


def test_stitch_with_an_overlap_of_zero_writes_nothing():
    dims, patch, ov = (6, 6, 6), (4, 4, 4), (1, 1, 0)
    assert HP.crop_window(patch, ov)[1][2] == 0
    pos = HP.grid_positions(dims, patch, ov)[:4]
    got, want = stitch_both(stitch_logits("empty", 4, 1, 2, patch), pos, dims, 1, ov)
    assert bool((want == CANARY).all()) and np.array_equal(got, want)


# o0 > o1: the step along axis 0 is pd - 2 o0, the window pd - o0 - o1 long -- neighbours share o0 - o1 planes of at least 32 x 32
OVERLAP_CASES = [("4_3_2", (9, 36, 40), (12, 12, 12), (4, 3, 2)), ("3_1_1", (7, 32, 32), (8, 18, 18), (3, 1, 1))]


@pytest.mark.parametrize("order", ["grid", "reversed"])
@pytest.mark.parametrize("tag,dims,patch,ov", OVERLAP_CASES, ids=[c[0] for c in OVERLAP_CASES])
def test_stitch_overlapping_windows_in_one_launch_the_later_row_wins(tag, dims, patch, ov, order):
    pos = HP.grid_positions(dims, patch, ov)
    lg = stitch_logits("overlap:" + tag, len(pos), 1, 3, patch)
    if order == "reversed":
        pos, lg = pos[::-1].copy(), lg[::-1].copy()
    got, want = stitch_both(lg, pos, dims, 1, ov)               # ALL patches of the volume in one call
    first = np.full_like(want, CANARY)                          # the other rule -- the earlier row wins -- for the message
    P.add_processed_batch(first, P.postprocess(lg[::-1], 1), pos[::-1], list(ov))
    shared = int((first != want).sum())
    assert dims[1] * dims[2] >= 32 * 32 and shared >= 1024, shared
    bad = got != want
    assert not bad.any(), f"{tag} {order}: {int(bad.sum())} voxels differ ({int((bad & (got == first)).sum())} hold the earlier row's value)"


class ElementwiseNet(torch.nn.Module):
    """Logits that are the same bits on the CPU and on the device: exact sums, products and negations of the input's first channel
    (multiples of 1/4) and the voxel's plane index INSIDE the patch -- two patches that cover a voxel give it different logits."""

    def __init__(self, patch):
        super().__init__()
        self.dummy = torch.nn.Parameter(torch.zeros(1))
        self.register_buffer("plane", torch.arange(patch[0], dtype=torch.float32).reshape(-1, 1, 1).expand(*patch).contiguous())

    def forward(self, x):
        x = x[:, 0] + self.plane
        return torch.stack([3.0 * x, -x, x * x], dim=1)


def test_grid_predictor_is_independent_of_the_batch_size():
    patch, ov, nh = [8, 10, 10], [3, 1, 1], 1
    img = U._np_rng("dp:predictor").integers(-8, 9, size=(1, 5, 16, 16)).astype(np.float32) / 4.0
    n = len(HP.grid_positions(img.shape[1:], patch, ov))
    assert n == 12
    net = ElementwiseNet(patch)

    def fwd(x):
        with torch.no_grad():
            return net(torch.from_numpy(x)).numpy()

    want = P.predict_volume(fwd, img, patch, ov, nh, batch_size=1, pad_kwargs={"mode": "symmetric"})
    assert np.array_equal(want, P.predict_volume(fwd, img, patch, ov, nh, batch_size=n, pad_kwargs={"mode": "symmetric"}))
    net = net.to(DEV)
    got = {bs: HP.GridPredictor(net, patch, ov, num_heatmaps=nh, pad_mode="symmetric", batch_size=bs)(img).cpu().numpy() for bs in (1, n, 4)}
    for bs, r in got.items():
        assert np.array_equal(r, want), f"batch_size {bs}: {int((r != want).sum())} voxels differ from the oracle loop"
    assert np.array_equal(got[1], got[n])
