"""Times of the resampling kernels (profiles/resample.md).

    python tools/resample_timing.py [--repeat 20] [--skip-axis]

The way back: fp32 probabilities of 4 and 14 classes at 160 x 160 x 96 to 320 x 320 x 192 and to 512 x 512 x 60 (thick slices),
`resample_argmax` against F.interpolate(p[None], size, mode="trilinear", align_corners=False).argmax(1).to(torch.uint8) through
stock PyTorch.  Both are timed with device events after warm-up, alternating, median / min / max of --repeat runs; the peak extra
memory of each is the allocator's peak over one call minus what was allocated before it.  The share of voxels on which the two
disagree is reported too (ATen takes its interpolation weights in fp32 and associates differently: near-ties may go either way;
where an axis shrinks, the anti-aliased default is a different filter from stock trilinear, so that case is also run with
antialias=False, which is stock's rule).

The axis pass: 256^3 fp32 to 2x along each axis in turn, and to 1/2 anti-aliased, bytes read + written over the kernel's time, beside
a plain device copy (Tensor.copy_) of as many bytes.  Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "torch-mednet_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from mednet_hip import resample as M  # noqa: E402

DEV = "cuda:0"


def timed(fn, repeat):
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def stats(ms, prefix):
    return {prefix + "_ms_median": float(np.median(ms)), prefix + "_ms_min": float(min(ms)), prefix + "_ms_max": float(max(ms))}


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return int(peak)


def way_back(ncls, shape, size, repeat, antialias=True):
    g = torch.Generator(device=DEV).manual_seed(ncls)
    prob = torch.softmax(2.0 * torch.randn((ncls,) + shape, device=DEV, generator=g), 0)
    fused = lambda: M.resample_argmax(prob, size=size, antialias=antialias)
    stock = lambda: F.interpolate(prob[None], size=size, mode="trilinear", align_corners=False).argmax(1).to(torch.uint8)
    for _ in range(3):
        a, b = fused(), stock()
    torch.cuda.synchronize()
    differ = float((a != b[0]).float().mean())
    del a, b
    f_ms, s_ms = [], []
    for _ in range(repeat):              # alternating
        f_ms += timed(fused, 1)
        s_ms += timed(stock, 1)
    vox = int(np.prod(size))
    rec = dict(what="way_back", classes=ncls, shape=shape, size=size, antialias=antialias, out_bytes=vox, voxels_that_differ=differ,
               fused_peak_extra_bytes=peak_extra(fused), stock_peak_extra_bytes=peak_extra(stock))
    rec.update(stats(f_ms, "fused"))
    rec.update(stats(s_ms, "stock"))
    rec["speedup_median"] = rec["stock_ms_median"] / rec["fused_ms_median"]
    return rec


def axis_pass(axis, n_out, antialias, repeat, n=256):
    vol = torch.randn((1, n, n, n), device=DEV)
    table = M.device_table(n, n_out, "linear", antialias, vol.device)
    run = lambda: M.resample_axis(vol, axis, table)
    out = run()
    nbytes = (vol.numel() + out.numel()) * 4
    a = torch.empty(nbytes // 8, dtype=torch.float32, device=DEV)
    b = torch.empty_like(a)
    copy = lambda: b.copy_(a)
    for _ in range(3):
        run(), copy()
    r_ms, c_ms = [], []
    for _ in range(repeat):
        r_ms += timed(run, 1)
        c_ms += timed(copy, 1)
    rec = dict(what="axis_pass", axis=axis, n_in=n, n_out=n_out, antialias=antialias, taps=table[3], bytes=nbytes)
    rec.update(stats(r_ms, "pass"))
    rec.update(stats(c_ms, "copy"))
    rec["pass_GBps"] = nbytes / (rec["pass_ms_median"] * 1e-3) / 1e9
    rec["copy_GBps"] = nbytes / (rec["copy_ms_median"] * 1e-3) / 1e9
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--skip-axis", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_timing.py: no GPU (times are taken on the device or not at all)")
    for ncls in (4, 14):
        # the sizes as D x H x W, and with the short axis first (slices along z)
        for shape, size in (((160, 160, 96), (320, 320, 192)), ((160, 160, 96), (512, 512, 60)), ((96, 160, 160), (192, 320, 320)),
                            ((96, 160, 160), (60, 512, 512))):
            print(json.dumps(way_back(ncls, shape, size, args.repeat)), flush=True)
            if any(m < n for n, m in zip(shape, size)):   # stock trilinear point-samples a shrinking axis: the same rule, for the time
                print(json.dumps(way_back(ncls, shape, size, args.repeat, antialias=False)), flush=True)
    if not args.skip_axis:
        for axis in (0, 1, 2):
            for n_out, aa in ((512, True), (128, True)):
                print(json.dumps(axis_pass(axis, n_out, aa, args.repeat)), flush=True)


if __name__ == "__main__":
    main()
