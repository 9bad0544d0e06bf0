"""Cost of the image-degradation transforms (csrc/degrade.hip, mednet_hip/sampler.py) on one MI355X; profiles/degrade.md holds the
numbers.  Prints one JSON line (and writes it to `--out FILE`).

  transforms   gaussian_noise_, gaussian_blur (sigma 0.75) and simulate_low_resolution (zoom 0.6) alone at 4 x 1 x 128^3 and
               4 x 4 x 128^3 with all rows active: whole calls (tables built and uploaded, one to three launches).
  passes       mednet_filter_rows per axis at 13 taps on 16 x 128^3, against mednet_resample_axis with the equivalent contiguous
               table (index = start + k) on the same shape, as a rate at 8 bytes per voxel and as a share of the 6.3 TB/s the HBM
               achieves (8 TB/s peak).
  sampler      a batch of 4 x 1 x 128^3 with nnU-Net's default probabilities over 200 batches and with every probability 1,
               against degrade=None.

Rule followed: versions are compared in one process and ALTERNATED over several rounds, every shape is warmed up, each window is
bracketed by device events (kernels) or closed by a device synchronise (sampler batches), and the spread (min, max over the rounds)
is reported next to the median."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "torch-mednet_amd")]
import numpy as np
import torch
from mednet_hip import resample as HR
from mednet_hip import sampler as HS

dev = torch.device("cuda", 0)
assert torch.cuda.is_available(), "run_degrade.py measures on the GPU only"
HBM_ACHIEVABLE, HBM_PEAK = 6.3e12, 8.0e12
stat = lambda v: {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(variants, rounds=7, reps=10):
    """{name: fn} -> {name: [ms per call, one per round]}, the variants taking turns inside every round."""
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            out[k].append(timed(fn, reps))
    return out


def transforms_leg():
    res = {}
    for c in (1, 4):
        data = torch.randn((4, c, 128, 128, 128), device=dev)
        scratch = torch.empty_like(data)
        t = alternate({"noise": lambda: HS.gaussian_noise_(data, 0.1, 7),
                       "blur_sigma_0.75": lambda: HS.gaussian_blur(data, 0.75, scratch),
                       "low_resolution_zoom_0.6": lambda: HS.simulate_low_resolution(data, 0.6, scratch)})
        res[f"4x{c}x128^3"] = {k: dict(stat(v), unit="ms per call") for k, v in t.items()}
    return res


def passes_leg():
    rows, n, sigma = 16, 128, 1.5
    src = torch.randn((rows, 1, n, n, n), device=dev)
    dst = torch.empty_like(src)
    count, index, weight, taps = HS.blur_table(n, sigma)
    assert taps == 13
    start = np.clip(np.arange(n) - 6, 0, n - taps).astype(np.int32)
    contiguous = np.minimum(start[:, None] + np.arange(taps)[None, :], n - 1).astype(np.int32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    row_table = torch.zeros(rows, dtype=torch.int32, device=dev)
    identity = torch.full((rows,), -1, dtype=torch.int32, device=dev)
    reflecting = (up(count[None]), up(index[None]), up(weight[None]))
    straight = (up(count[None]), up(contiguous[None]), up(weight[None]))
    table = (up(start), up(count), up(weight), taps)
    vol = src.view(rows, n, n, n)
    res = {}
    nbytes = 8.0 * src.numel()
    for axis in (0, 1, 2):
        t = alternate({"filter_rows_reflect": lambda: HS.filter_rows(src, dst, axis, row_table, reflecting),
                       "filter_rows_contiguous": lambda: HS.filter_rows(src, dst, axis, row_table, straight),
                       "filter_rows_identity": lambda: HS.filter_rows(src, dst, axis, identity, straight),
                       "resample_axis": lambda: HR.resample_axis(vol, axis, table)})
        res[f"axis{axis}"] = {k: dict(stat(v), TB_per_s=round(nbytes / (float(np.median(v)) * 1e-3) / 1e12, 3),
                                      share_of_achievable_hbm=round(nbytes / (float(np.median(v)) * 1e-3) / HBM_ACHIEVABLE, 3),
                                      share_of_peak_hbm=round(nbytes / (float(np.median(v)) * 1e-3) / HBM_PEAK, 3)) for k, v in t.items()}
    return {"shape": "16 x 128^3, 13 taps", "bytes_counted": "8 per voxel", "ms_per_pass": res}


def sampler_leg():
    rng = np.random.default_rng(0)
    size, patch, B = 192, [128] * 3, 4
    images = [rng.standard_normal((1, size, size, size), dtype=np.float32).astype(np.float16) for _ in range(4)]
    labels = [rng.integers(0, 3, (1, size, size, size)).astype(np.uint8) for _ in range(4)]
    mk = lambda **kw: HS.DevicePatchSampler(images, labels, patch, samples_per_subject=64, device=dev, **kw)
    one = dict(p_noise=1, p_blur=1, p_blur_channel=1, p_low_resolution=1, p_low_resolution_channel=1)
    legs = {"degrade_none": mk(), "nnunet_defaults": mk(degrade=HS.ImageDegradation()), "all_probabilities_1": mk(degrade=HS.ImageDegradation(**one))}
    np.random.seed(1)
    for s in legs.values():
        for _ in range(3):
            s.batch(range(B))
    torch.cuda.synchronize()
    rounds, per = 5, 40       # 200 batches per leg
    times = {k: [] for k in legs}
    for r in range(rounds):
        for k, s in legs.items():
            t0 = time.perf_counter()
            for i in range(per):
                s.batch(range(i * B, i * B + B))
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / per * 1e3)
    return {"shape": "4 x 1 x 128^3 from 192^3 volumes", "batches_per_leg": rounds * per,
            "ms_per_batch": {k: stat(v) for k, v in times.items()}}


line = json.dumps({"metric": "image degradation on the device: ms per call / pass / batch", "transforms": transforms_leg(),
                   "passes": passes_leg(), "sampler": sampler_leg()})
print(line)
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write(line + "\n")
