"""SHA-256 digests of what the inference and evaluation passes compute -- the crop-stitch and the blended predictor's kernels
(mednet_hip.predict), the patch crop of the sampler, the case metrics (mednet_hip.metrics) and the connected components
(mednet_hip.components) -- on inputs seeded on the CPU by a tag: two commits whose kernels compute the same values print the same
lines.  Only the package's Python surface is used (plus metrics._surface_masks for the two-volume launch, which the tests use too),
so the tool runs against any commit's package and library:
HD_PKG=<directory that holds that commit's mednet_hip/> MEDNET_LIB_PATH=<its libmednet_hip.so> python tools/volume_digest.py
(as tools/head_digest.py); without them it takes this tree's.  One process per package; compare the outputs with diff.

One JSON line per case: its name and ONE SHA-256 over the digests of all its tensors (DIGEST_FULL=1 lists every tensor's digest).
Shapes: (1, 1, 1); (1, 17, 241) = 4097 voxels, two rows of the row plan, the second a single voxel; (17, 9, 70) = 10710 voxels, three
rows, x beyond one wavefront; (129, 256, 256), once per row-planned entry: more than 2048 x 4096 voxels, so the row cap holds and a
row is longer than 4096 voxels; (5, 7, 500) and (3, 300, 70) for the distance transform's bundles of 16 and 32 lines.  The stitch
geometries are tests/blend_util.py's and oracle/ref_predict.py's.
Families (argument: a comma-separated list, default all): metrics, components, predict, blend, peaks.

    python tools/volume_digest.py --time      # instead of digests: evaluate_case on tools/components_timing.py's synthetic case at
                                              # 256^3 and heatmap_peaks at 3 x 256^3, device events, one JSON line each"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("HD_PKG") or os.path.join(ROOT, "torch-mednet_amd")
for p in (os.path.join(ROOT, "tests"), ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mednet_hip  # noqa: E402,F401
from mednet_hip import components as C  # noqa: E402
from mednet_hip import metrics as H  # noqa: E402
from mednet_hip import predict as HP  # noqa: E402
from mednet_hip.sampler import DevicePatchSampler  # noqa: E402

import blend_util as B  # noqa: E402  (tests/)
import components_util as U  # noqa: E402  (tests/)
from oracle import ref_predict as RP  # noqa: E402

DEV = "cuda:0"
FULL = os.environ.get("DIGEST_FULL", "0") == "1"
SHAPES = [(1, 1, 1), (1, 17, 241), (17, 9, 70)]
BIG = (129, 256, 256)


def sh(shape):
    return "x".join(map(str, shape))


def seed_of(tag):
    return int.from_bytes(hashlib.sha256(tag.encode()).digest()[:6], "little")


def gen(tag):
    return torch.Generator().manual_seed(seed_of(tag))


def u8(tag, hi, shape):
    """uint8 values in [0, hi), seeded by the tag."""
    return torch.randint(0, hi, tuple(shape), generator=gen(tag), dtype=torch.uint8)


def f32(tag, shape, scale=1.0):
    return torch.randn(*shape, generator=gen(tag), dtype=torch.float32) * scale


def digest(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().contiguous().cpu()
        t = (t.view(torch.int16) if t.dtype == torch.float16 else t).numpy()
    if isinstance(t, np.ndarray):
        return hashlib.sha256(np.ascontiguousarray(t).tobytes()).hexdigest()
    return hashlib.sha256(repr(t).encode()).hexdigest()


def emit(name, tensors):
    torch.cuda.synchronize()
    res = {k: digest(v) for k, v in tensors.items()}
    line = {"case": name, "sha256": hashlib.sha256("".join(f"{k}={v};" for k, v in res.items()).encode()).hexdigest()}
    print(json.dumps({**line, **res} if FULL else line), flush=True)
    torch.cuda.empty_cache()


def blobs(shape, seed):
    return torch.from_numpy(U.blobs(shape, seed=seed, classes=3, count=20))


# ---------------------------------------------------------------------------------------------- metrics
def metrics_cases():
    for shape in SHAPES + [BIG]:
        for ncls in (1, 3, 32) if shape != BIG else (3,):
            pred, lab = u8(f"p{ncls}", ncls + 1, shape).to(DEV), u8(f"l{ncls}", ncls + 1, shape).to(DEV)  # (the value ncls: out of range)
            for ign in (None, 1):
                cm, oor = H.confusion(pred, lab, ncls, ign)
                emit(f"confusion {sh(shape)} C={ncls} ign={ign}", {"cm": cm, "oor": oor})
        pred, lab = u8("p3", 4, shape).to(DEV), u8("l3", 5, shape).to(DEV).long() - 1  # labels -1 (ignored) .. 3 (out of range)
        cm, oor = H.confusion(pred, lab, 3, -1)
        emit(f"confusion {sh(shape)} C=3 int64 ign=-1", {"cm": cm, "oor": oor})
        surf, d2 = u8("surf", 2, shape).to(DEV), f32("d2", shape, 3.0).square().to(DEV)
        emit(f"surface_stats {sh(shape)}", dict(zip(("counts", "max", "sum"), H.surface_stats(surf, d2, 4.0))))
    for shape in SHAPES:
        a, b = u8("ma", 3, shape).to(DEV), u8("mb", 3, shape).to(DEV)
        emit(f"surface_mask {sh(shape)} one", {"a": H.surface_mask(a, 1)})
        emit(f"surface_mask {sh(shape)} two", dict(zip("ab", H._surface_masks(a, b, 2))))
    for shape in SHAPES + [(5, 7, 500), (3, 300, 70)]:
        seed = (f32("seed", shape) > 1.6).to(torch.uint8).to(DEV)
        for name, spacing in (("unit", (1, 1, 1)), ("dyadic", (2.0, 0.5, 0.25)), ("general", (3.0, 0.7, 0.7))):
            emit(f"edt_squared {sh(shape)} {name}", {"d2": H.edt_squared(seed, spacing)})
    for shape in SHAPES:
        pred, lab = blobs(shape, 3).to(DEV), blobs(shape, 4).to(DEV)
        m = H.evaluate_case(pred, lab, 4, spacing=(3.0, 0.7, 0.7), ignore_index=3, lesion_classes=(1, 2)).to_host()
        emit(f"evaluate_case {sh(shape)}", {k: (np.asarray(v) if isinstance(v, np.ndarray) else v) for k, v in sorted(m.items())})
        for cls in (1, 2):
            emit(f"lesion_detection {sh(shape)} cls={cls}", H.lesion_detection(pred, lab, cls, 18, 2).to_host())


# ---------------------------------------------------------------------------------------------- components
def at_offset(vol, off):
    """The same volume `off` bytes behind an aligned address."""
    buf = torch.zeros(vol.numel() + 4, dtype=torch.uint8, device=DEV)
    buf[off:off + vol.numel()] = vol.flatten().to(DEV)
    return buf[off:off + vol.numel()].view(vol.shape)


def label_case(name, vol, cls, conn, invert):
    comps = C.label_components(vol, cls, conn, invert)
    keep = (torch.arange(comps.count + 1, device=DEV) % 2).to(torch.uint8)
    emit(name, {"labels": comps.labels, "count": comps.count, "stats": comps.stats(), "select": comps.select(keep, 7)})


def components_cases():
    for shape in SHAPES:
        volumes = {"random": torch.from_numpy(U.random_volume(shape, 0.31, seed=31, classes=3)), "blobs": blobs(shape, 5)}
        for kind, vol in volumes.items():
            for cname, cls, inv in (("all", None, False), ("2", 2, False), ("not2", 2, True)):
                for conn in (6, 18, 26):
                    for off in range(4) if (kind == "random" and conn == 26) else (0,):
                        label_case(f"label_components {sh(shape)} {kind} cls={cname} conn={conn} off={off}", at_offset(vol, off), cls, conn, inv)
        vol = volumes["blobs"].to(DEV)
        emit(f"postprocess {sh(shape)}", {
            "keep_largest": C.keep_largest(vol, (1, 2, 3)), "keep_largest_18": C.keep_largest(vol, (2,), 18),
            "remove_small_voxels": C.remove_small(vol, (1, 3), min_voxels=30),
            "remove_small_volume": C.remove_small(vol, (2,), min_volume=40.0, spacing=(3.0, 0.7, 0.7), connectivity=6),
            "fill_holes": C.fill_holes(vol, 1), "empty": C.keep_largest(torch.zeros_like(vol), (1,)),
            "Postprocess": C.Postprocess(keep_largest=(1, 2), min_voxels={3: 10}, fill_holes=(1,))(vol)})
    label_case(f"label_components {sh(BIG)} random cls=all conn=26 off=0", torch.from_numpy(U.random_volume(BIG, 0.31, seed=31, classes=3)).to(DEV),
               None, 26, False)


# ---------------------------------------------------------------------------------------------- crop-stitch predictor, sampler
def predict_cases():
    for tag, shape, patch, ov, _, nh, ncls, _ in RP.PREDICT_CASES:
        img, logits_for = RP.predict_inputs(tag, shape, patch, nh, ncls)
        vol = torch.from_numpy(img).to(DEV).float().contiguous()
        pos_all = torch.from_numpy(HP.grid_positions(shape[1:], patch, ov)).to(DEV)
        for mode in ("constant", "symmetric"):
            emit(f"gather_patches {tag} {mode}", {f"mirror{m}": HP.gather_patches(vol, pos_all, patch, ov, mode, mirror=m) for m in range(8)})
        logits = torch.from_numpy(np.stack([logits_for(k) for k in range(pos_all.shape[0])])).to(DEV)
        for batch in (1, 3):
            result = torch.zeros((nh + 1,) + tuple(shape[1:]), dtype=torch.uint8, device=DEV)
            for b0 in range(0, pos_all.shape[0], batch):
                HP.assemble(logits[b0:b0 + batch], pos_all[b0:b0 + batch].contiguous(), result, nh, ov)
            emit(f"assemble {tag} overlap={ov} batch={batch}", {"result": result})
    for name, dtype in (("f16", np.float16), ("f32", np.float32)):  # image f16 -> f32 / f32 -> f32, heat maps and labels u8 -> u8
        images = [f32(f"img{i}", (2, 19, 23, 70)).numpy().astype(dtype) for i in range(2)]
        labels = [u8(f"lab{i}", 4, (1, 19, 23, 70)).numpy() for i in range(2)]
        heat = [u8(f"hm{i}", 256, (3, 19, 23, 70)).numpy() for i in range(2)]
        np.random.seed(7)
        b = DevicePatchSampler(images, labels, (8, 12, 33), heatmaps=heat, device=DEV).batch([0, 1, 2, 3, 1])
        emit(f"crop_patches image={name}", {"data": b["data"], "label": b["label"], "pos": b["patch_position"]})


# ---------------------------------------------------------------------------------------------- blended predictor
def finalize_all(acc, wsum, nh, blend_of):
    out = {"result": HP.finalize(acc, wsum, nh, blend_of, result=True)[0], "heat": HP.finalize(acc, wsum, nh, blend_of, heatmaps=True)[2]}
    for name, dt in (("prob32", torch.float32), ("prob16", torch.float16)):
        out[name] = HP.finalize(acc, wsum, nh, blend_of, probabilities=dt)[1]
    res, prob, heat = HP.finalize(acc, wsum, nh, blend_of, result=True, probabilities=torch.float16, heatmaps=True)
    out.update(all_result=res, all_prob=prob, all_heat=heat)
    return out


def blend_cases():
    nh, ncls = 2, 3
    pos_all = B.grid_positions(B.VOLUME, B.PATCH, B.OVERLAP)
    logits = torch.from_numpy(B.random_logits(len(pos_all), nh + ncls, B.PATCH, seed=11)).to(DEV)
    pos_dev = torch.from_numpy(pos_all).to(DEV)
    win = tuple(torch.from_numpy(v).to(DEV) for v in B.gaussian_windows(B.PATCH))
    for blend_of in ("probabilities", "logits"):
        for batch in (1, 4):
            acc = torch.zeros((nh + ncls,) + B.VOLUME, dtype=torch.float32, device=DEV)
            wsum = torch.zeros(B.VOLUME, dtype=torch.float32, device=DEV)
            for m in (0, 5, 7):
                for b0 in range(0, len(pos_all), batch):
                    HP.accumulate(logits[b0:b0 + batch], pos_dev[b0:b0 + batch].contiguous(), acc, wsum, win, nh, B.OVERLAP, m, blend_of)
                emit(f"accumulate {blend_of} batch={batch} mirror<={m}", {"acc": acc, "wsum": wsum})
        emit(f"finalize {blend_of}", finalize_all(acc, wsum, nh, blend_of))
        wsum[0, 0, 0] = 0.0
        wsum[-1, -1, -1] = 0.0
        emit(f"finalize {blend_of} uncovered", finalize_all(acc, wsum, nh, blend_of))
        # ties between the class accumulators and heat maps on and around the clip edges, under a weight sum of 1 and of 0.5
        edges = torch.tensor([-1.0, -0.0, 0.0, 0.5, 0.99999994, 1.0, 254.5, 254.99998, 255.0, 255.00002, 300.0, 1e30])
        heat = edges[torch.randint(0, len(edges), (nh,) + B.VOLUME, generator=gen("edges"))]
        cls = torch.randint(-1, 2, (ncls,) + B.VOLUME, generator=gen("ties")).float()
        wsum = (1.0 - 0.5 * u8("half", 2, B.VOLUME).float()).to(DEV)
        emit(f"finalize {blend_of} ties and clip edges", finalize_all((torch.cat((heat, cls)).to(DEV) * wsum).contiguous(), wsum, nh, blend_of))


def peaks_cases():
    for shape in ((1, 1, 1), (1, 16, 256), (1, 17, 241), (17, 9, 70)):
        vox = shape[0] * shape[1] * shape[2]
        for nh in (1, 3):
            heat = f32(f"heat{nh}", (nh,) + shape)
            flat = heat.view(nh, -1)
            variants = {"random": heat.clone(), "tie": heat.clone(), "nan": heat.clone(), "negative": -heat.abs() - 1.0, "all_nan": heat.clone()}
            for k in range(nh):  # the maximum twice, the later copy first in memory order of the planting; a NaN next to / after the maximum
                top = flat[k].max() + 1.0
                variants["tie"].view(nh, -1)[k, [(vox * 3) // 4, vox // 3, vox - 1]] = top
                variants["nan"].view(nh, -1)[k, [0, vox // 2, vox - 1]] = float("nan")
            variants["all_nan"].view(nh, -1)[nh - 1, :] = float("nan")
            for name, t in variants.items():
                emit(f"heatmap_peaks {sh(shape)} H={nh} {name}", dict(zip(("zyx", "value"), HP.heatmap_peaks(t.to(DEV)))))


# ---------------------------------------------------------------------------------------------- --time
def timed(fn, repeat=7):
    fn()
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def time_cases():
    from components_timing import synthetic_case  # tools/
    shape = (256, 256, 256)
    pred, lab = synthetic_case(shape, seed=0), synthetic_case(shape, seed=1)
    rec = timed(lambda: H.evaluate_case(pred, lab, 4, spacing=(3.0, 0.7, 0.7), lesion_classes=(1, 2, 3)), repeat=5)
    print(json.dumps({"case": "evaluate_case", "shape": shape, "package": os.path.dirname(mednet_hip.__file__), **rec}), flush=True)
    heat = f32("heat", (3,) + shape).to(DEV)
    rec = timed(lambda: HP.heatmap_peaks(heat), repeat=21)
    print(json.dumps({"case": "heatmap_peaks", "shape": (3,) + shape, **rec}), flush=True)


RUN = {"metrics": metrics_cases, "components": components_cases, "predict": predict_cases, "blend": blend_cases, "peaks": peaks_cases}
if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--time":
        time_cases()
    else:
        for family in (args[0].split(",") if args else list(RUN)):
            RUN[family]()
