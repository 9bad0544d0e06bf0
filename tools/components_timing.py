"""Times of the component post-processing on synthetic cases (profiles/components.md).

    python tools/components_timing.py [--shapes 256,256,256 512,512,256] [--scipy] [--once]

Per shape: a four-class volume of random ellipsoid "organs" plus small satellite blobs (a few percent foreground, as
profiles/case_metrics.md uses); label (26-connectivity, all classes) + statistics + keep-largest, timed with device events after
warm-up, median of --repeat runs; with --scipy the same post-processing through scipy.ndimage.label on the host, the two copies
included.  --once runs the device path one single time after warm-up, for a kernel trace taken around this script.  Prints one JSON
line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "torch-mednet_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from mednet_hip import components as C  # noqa: E402

CLASSES = (1, 2, 3)


def synthetic_case(shape, seed=0):
    rng = np.random.default_rng(seed)
    d, h, w = shape
    vol = torch.zeros(shape, dtype=torch.uint8, device="cuda:0")
    z, y, x = torch.meshgrid(*(torch.arange(s, device="cuda:0", dtype=torch.float32) for s in shape), indexing="ij")
    for cls in CLASSES:
        for k in range(1 + 12):           # one organ, twelve satellites
            c = [rng.uniform(0.15, 0.85) * s for s in shape]
            r = [(rng.uniform(0.08, 0.14) if k == 0 else rng.uniform(0.005, 0.02)) * s + 1 for s in shape]
            inside = ((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 <= 1.0
            vol[inside] = cls
    return vol


def device_path(vol):
    comps = C.label_components(vol, None, 26)
    table = comps.stats()
    out = comps.select(C._keep_vector(C._largest_keep(table, CLASSES)), 0)
    return comps, out


def scipy_path(vol):
    from scipy import ndimage as ndi
    st = ndi.generate_binary_structure(3, 3)
    a = vol.cpu().numpy()
    out = a.copy()
    for cls in CLASSES:
        lab, k = ndi.label(a == cls, st)
        if k > 1:
            sizes = np.bincount(lab.reshape(-1))
            sizes[0] = 0
            out[(lab > 0) & (lab != sizes.argmax())] = 0
    res = torch.from_numpy(out).to(vol.device)
    torch.cuda.synchronize()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["256,256,256", "512,512,256"])
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--scipy", action="store_true")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    for text in args.shapes:
        shape = tuple(int(s) for s in text.split(","))
        vol = synthetic_case(shape)
        comps, out = device_path(vol)
        torch.cuda.synchronize()
        rec = dict(shape=shape, foreground=float((vol != 0).float().mean()), components=comps.count,
                   kept_voxels=int((out != 0).sum()))
        if args.once:
            device_path(vol)
            torch.cuda.synchronize()
            print(json.dumps(rec))
            continue
        ms = []
        for _ in range(args.repeat):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            device_path(vol)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        rec.update(device_ms_median=float(np.median(ms)), device_ms_min=float(min(ms)), device_ms_max=float(max(ms)))
        if args.scipy:
            t = time.perf_counter()
            ref = scipy_path(vol)
            rec.update(scipy_s=time.perf_counter() - t, equal=bool(torch.equal(ref, out)))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
