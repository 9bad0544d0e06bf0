"""Same-box A/B of the predictors (profiles/blend_predict.md): BASELINE config-2 network (ResidualUNet3D(1, 4, f_maps 32..256)), bf16
storage, a synthetic 256^3 volume, 128^3 patches with a 32-voxel overlap (step 64: 64 patches, up to 8-fold coverage), batch 4.

    python tools/blend_predict_timing.py                    # crop-stitch and blend="gaussian" alternating (BP_ROUNDS rounds), then
                                                            # blend="gaussian" with three mirror axes once; one JSON line each
    BP_CASES=gaussian BP_ROUNDS=1 rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/blend_predict_timing.py
                                                            # per-launch times of blend_accumulate_kernel / blend_finalize_kernel

The last line holds the bytes a blend_accumulate launch moves, counted from the shapes (per patch voxel inside the volume: 4 B of logits
per channel read, 8 B per channel and 8 B of weight sum read and written), and the time of such launches measured with device events
on a fixed batch of logits (no model in between)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "torch-mednet_amd")]
import numpy as np
import torch

import mednet_hip
from mednet_hip import predict as HP
from mednet_hip.synth import keyed_init_
from mednet_hip.unet.model import ResidualUNet3D

SIZE, PATCH, OV, BATCH = int(os.environ.get("BP_SIZE", 256)), [128] * 3, [32] * 3, int(os.environ.get("BP_BATCH", 4))
CASES = os.environ.get("BP_CASES", "crop,gaussian,mirror3").split(",")
ROUNDS = int(os.environ.get("BP_ROUNDS", 3))

assert torch.cuda.is_available(), "needs the GPU: there is nothing to time without it"
dev = torch.device("cuda", 0)
mednet_hip.set_precision("bf16")
net = keyed_init_(ResidualUNet3D(1, 4, False, f_maps=[32, 64, 128, 256])).to(dev)
vol = torch.from_numpy(np.random.default_rng(0).standard_normal((1, SIZE, SIZE, SIZE)).astype(np.float16)).to(dev)
pos_all = HP.grid_positions(vol.shape[1:], PATCH, OV)
make = {"crop": lambda: HP.GridPredictor(net, PATCH, OV, pad_mode="constant", batch_size=BATCH),
        "gaussian": lambda: HP.GridPredictor(net, PATCH, OV, pad_mode="constant", batch_size=BATCH, blend="gaussian"),
        "mirror3": lambda: HP.GridPredictor(net, PATCH, OV, pad_mode="constant", batch_size=BATCH, blend="gaussian", mirror_axes=(0, 1, 2))}


def timed(pred):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = pred(vol)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


preds = {k: make[k]() for k in CASES}
for k in CASES:
    if k != "mirror3" or len(CASES) == 1:
        timed(preds[k])  # warm-up (the mirrored passes launch the same kernels as "gaussian")
times = {k: [] for k in CASES}
hist = {}
for r in range(ROUNDS):
    for k in CASES:
        if k == "mirror3" and r > 0:
            continue  # eight forward passes per patch: once
        dt, res = timed(preds[k])
        times[k].append(dt)
        hist[k] = torch.bincount(res[-1].flatten().int(), minlength=4).tolist()
for k in CASES:
    passes = 8 if k == "mirror3" else 1
    best = min(times[k])
    print(json.dumps({"case": k, "volume": [SIZE] * 3, "patches": len(pos_all), "forward_passes": passes * len(pos_all), "batch": BATCH,
                      "s_per_volume": [round(t, 4) for t in times[k]], "patches_per_s": round(len(pos_all) / best, 2),
                      "forward_passes_per_s": round(passes * len(pos_all) / best, 2), "labels_hist": hist[k]}))

if "gaussian" in CASES:
    # blend_accumulate / blend_finalize alone: a fixed batch of logits at the volume's first positions
    ch = 4
    pos = torch.from_numpy(pos_all[:BATCH]).to(dev)
    lg = torch.randn((BATCH, ch) + tuple(PATCH), device=dev)
    win = tuple(torch.from_numpy(v).to(dev) for v in HP.blend_window(PATCH))
    acc = torch.zeros((ch,) + tuple(vol.shape[1:]), device=dev)
    wsum = torch.zeros(tuple(vol.shape[1:]), device=dev)
    inside = 0
    for p in pos_all[:BATCH]:
        lo, hi = np.maximum(p - OV, 0), np.minimum(p - OV + PATCH, SIZE)
        inside += int(np.prod(hi - lo))
    nbytes = inside * (4 * ch + 8 * ch + 8)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    reps = 20
    for _ in range(3):
        HP.accumulate(lg, pos, acc, wsum, win, 0, OV)
    ev[0].record()
    for _ in range(reps):
        HP.accumulate(lg, pos, acc, wsum, win, 0, OV)
    ev[1].record()
    HP.finalize(acc, wsum, 0, result=True)
    ev[2].record()
    for _ in range(reps):
        HP.finalize(acc, wsum, 0, result=True)
    ev[3].record()
    torch.cuda.synchronize()
    t_acc, t_fin = ev[0].elapsed_time(ev[1]) / reps * 1e-3, ev[2].elapsed_time(ev[3]) / reps * 1e-3
    fin_bytes = SIZE ** 3 * (4 * ch + 4 + 1)
    print(json.dumps({"case": "kernels", "accumulate_launch_rows": BATCH, "accumulate_voxels_inside": inside, "accumulate_bytes": nbytes,
                      "accumulate_s_per_launch": round(t_acc, 7), "accumulate_bytes_per_s": round(nbytes / t_acc, 1),
                      "finalize_bytes": fin_bytes, "finalize_s": round(t_fin, 7), "finalize_bytes_per_s": round(fin_bytes / t_fin, 1),
                      "timing": "device events around 20 back-to-back launches"}))
