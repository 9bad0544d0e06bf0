"""Times of the intensity kernels (profiles/intensity.md).

    python tools/intensity_timing.py [--repeat 10] [--host-repeat 2] [--small]

Two synthetic cases: "ct", int16 512 x 512 x 256 with 55 % of the voxels at -1024 and a label mask (about 12 % of the voxels), and
"mri", fp32 4 x 240 x 240 x 155 whose background (about 40 %) is zero, with its non-zero mask.  For each: every stage (moments, select
with the four ranks of two percentiles, apply, non-zero mask) and the whole (`intensity_stats` with two percentiles, ZScore and
CTWindow end to end), beside the stock-PyTorch composition on the device (boolean indexing, torch.sort, .mean() / .std(), the
element-wise expression) and numpy on the host including the two copies.  Device times are taken with device events after warm-up,
alternating ours and stock, median / min / max of --repeat runs.  The algorithmic bytes of a stage (what it must read and write once,
from the shapes) over its time is printed as GB/s.  The select is also timed on a constant volume and on a uniformly random one of
the "ct" shape: heavy duplication is the worst case for LDS atomics.  Prints one JSON line per measurement."""
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

from mednet_hip import _lib as L  # noqa: E402
from mednet_hip import intensity as M  # noqa: E402

DEV = "cuda:0"
QS = (0.5, 99.5)


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


def emit(case, what, repeat, ours, stock=None, nbytes=None, **extra):
    for _ in range(2):
        ours()
        if stock is not None:
            stock()
    torch.cuda.synchronize()
    o_ms, s_ms = [], []
    for _ in range(repeat):
        o_ms += timed(ours, 1)
        if stock is not None:
            s_ms += timed(stock, 1)
    rec = dict(case=case, what=what, **extra)
    rec.update(stats(o_ms, "ours"))
    if stock is not None:
        rec.update(stats(s_ms, "stock"))
        rec["speedup_median"] = rec["stock_ms_median"] / rec["ours_ms_median"]
    if nbytes is not None:
        rec["algorithmic_bytes"] = int(nbytes)
        rec["ours_GBps"] = nbytes / (rec["ours_ms_median"] * 1e-3) / 1e9
    print(json.dumps(rec), flush=True)
    return rec


def make_ct(shape, g):
    noise = (torch.randn(shape, device=DEV, generator=g) * 250 + 40).clamp_(-1000, 3000)
    air = torch.rand(shape, device=DEV, generator=g) < 0.55
    vol = torch.where(air, torch.full_like(noise, -1024.0), noise).to(torch.int16)[None].contiguous()
    label = ((torch.rand(shape, device=DEV, generator=g) < 0.12) & ~air).to(torch.uint8)
    return vol, label


def make_mri(shape, g):
    vol = torch.rand((4,) + shape, device=DEV, generator=g) * 800 + 50
    z, y, x = torch.meshgrid(*(torch.linspace(-1, 1, n, device=DEV) for n in shape), indexing="ij")
    head = (z * z + y * y + x * x) < 1.15          # about 60 % of the box
    return (vol * head).contiguous(), head.to(torch.uint8)


# ---------------------------------------------------------------------------------------------- the stock compositions
def stock_stats(vol, mask):
    """Per channel: members by boolean indexing, sort, the two interpolated percentiles, mean and std."""
    out = []
    keep = mask.bool()
    for c in range(vol.shape[0]):
        m = vol[c][keep].float()
        s = torch.sort(m).values
        n = s.numel()
        ps = []
        for q in QS:
            pos = q / 100.0 * (n - 1)
            lo = int(np.floor(pos))
            hi = min(lo + 1, n - 1)
            ps.append(s[lo].double() + (s[hi].double() - s[lo].double()) * (pos - lo))
        out.append((m.double().mean(), m.double().std(unbiased=False), ps[0], ps[1]))
    return out


def stock_zscore(vol, mask):
    keep = mask.bool()
    out = torch.zeros(vol.shape, dtype=torch.float16, device=vol.device)
    for c in range(vol.shape[0]):
        m = vol[c][keep].float()
        out[c] = torch.where(keep, (vol[c].float() - m.mean()) / m.std(unbiased=False).clamp_min(1e-8), 0.0).half()
    return out


def stock_ct(vol, lo, hi, mean, std):
    return ((vol.float().clamp(lo, hi) - mean) / std).half()


def host_stats_and_zscore(vol, mask):
    """numpy on the host, with the copy down and the copy back up"""
    v, m = vol.cpu().numpy(), mask.cpu().numpy().astype(bool)
    out = np.zeros(v.shape, np.float16)
    for c in range(v.shape[0]):
        mem = v[c][m].astype(np.float32)
        np.percentile(mem, QS)
        mean, std = mem.mean(dtype=np.float64), mem.std(dtype=np.float64)
        out[c] = np.where(m, (v[c].astype(np.float32) - np.float32(mean)) / np.float32(max(std, 1e-8)), 0).astype(np.float16)
    return torch.from_numpy(out).to(DEV)


# ---------------------------------------------------------------------------------------------- one case
def run_case(case, vol, mask, repeat, host_repeat):
    c, vox = vol.shape[0], vol[0].numel()
    item = vol.element_size()
    src, msk = c * vox * item, c * vox            # the mask is read once per channel
    cases = M._cases(vol, mask, "timing")
    table = M._moments(cases)
    ranks, frac = M._ranks(table, QS)
    params = M._params(L.INTENSITY_ZSCORE, table, None, None, 0, c, 1e-8, DEV)[0]
    shape = dict(shape=list(vol.shape), dtype=str(vol.dtype), members=int(mask.sum()) * 1)

    emit(case, "moments (pass A + pass B)", repeat, lambda: M._moments(cases), nbytes=2 * (src + msk), **shape)
    emit(case, "select (3 levels, 4 ranks)", repeat, lambda: M._select(cases, ranks), nbytes=3 * (src + msk))
    emit(case, "apply -> f16", repeat, lambda: M.apply_table(vol, params, mask, 0.0, torch.float16), nbytes=src + msk + c * vox * 2)
    emit(case, "nonzero_mask + box", repeat, lambda: M.nonzero_mask(vol, return_box=True), nbytes=src + vox)
    emit(case, "intensity_stats (2 percentiles) | stock: index, sort, mean, std", repeat, lambda: M.intensity_stats(vol, mask, QS),
         lambda: stock_stats(vol, mask), nbytes=5 * (src + msk))
    z = M.ZScore(mask=mask)
    emit(case, "ZScore(mask) end to end | stock: index, mean, std, where", repeat, lambda: z(vol), lambda: stock_zscore(vol, mask),
         nbytes=3 * (src + msk) + c * vox * 2)
    ct = M.CTWindow([-950.0] * c, [400.0] * c, [60.0] * c, [180.0] * c)
    emit(case, "CTWindow end to end | stock: clamp, sub, div, half", repeat, lambda: ct(vol), lambda: stock_ct(vol, -950.0, 400.0, 60.0, 180.0),
         nbytes=src + c * vox * 2)
    # numpy on the host with both copies (a host clock around work that ends in a synchronise)
    ts = []
    for _ in range(host_repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_stats_and_zscore(vol, mask)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(case=case, what="numpy on the host: copy down, percentiles, mean, std, z-score, copy up", **stats(ts, "host"))), flush=True)
    # agreement with stock (not bit for bit: stock sums in another order and divides where we multiply)
    ours, ref = M.intensity_stats(vol, mask, QS).to_host(), stock_stats(vol, mask)
    for k in range(c):
        mean, std, p0, p1 = (float(v) for v in ref[k])
        print(json.dumps(dict(case=case, what="agreement", channel=k, n=int(ours.n[k]), mean_rel=abs(float(ours.mean[k]) - mean) / abs(mean),
                              std_rel=abs(float(ours.std[k]) - std) / std, p_lo_equal=float(ours.percentiles[k, 0]) == p0,
                              p_hi_equal=float(ours.percentiles[k, 1]) == p1)), flush=True)


def duplication(shape, repeat):
    """The select on a constant volume beside a uniformly random one (int16, no mask)."""
    g = torch.Generator(device=DEV).manual_seed(3)
    vox = int(np.prod(shape))
    const = torch.full((1,) + shape, -1024, dtype=torch.int16, device=DEV)
    rand = torch.randint(-32768, 32768, (1,) + shape, device=DEV, generator=g, dtype=torch.int32).to(torch.int16)
    ranks = torch.tensor([[vox // 200, vox // 200 + 1, vox - vox // 200 - 1, vox - vox // 200]], dtype=torch.int64, device=DEV)
    a = emit("duplication", "select on a constant volume", repeat, lambda: M._select([(const, None)], ranks), nbytes=3 * vox * 2, shape=list(shape))
    b = emit("duplication", "select on a random volume", repeat, lambda: M._select([(rand, None)], ranks), nbytes=3 * vox * 2, shape=list(shape))
    print(json.dumps(dict(case="duplication", what="constant over random", ratio=a["ours_ms_median"] / b["ours_ms_median"])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--host-repeat", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="a quarter of each extent (a rehearsal, not a measurement)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("intensity_timing.py: no GPU (times are taken on the device or not at all)")
    div = 4 if args.small else 1
    g = torch.Generator(device=DEV).manual_seed(1)
    ct_shape, mri_shape = (256 // div, 512 // div, 512 // div), (155 // div, 240 // div, 240 // div)
    vol, label = make_ct(ct_shape, g)
    run_case("ct", vol, label, args.repeat, args.host_repeat)
    del vol, label
    vol, head = make_mri(mri_shape, g)
    run_case("mri", vol, M.nonzero_mask(vol), args.repeat, args.host_repeat)
    del vol, head
    duplication(ct_shape, args.repeat)


if __name__ == "__main__":
    main()
