"""Throughput of the training-patch sampler on one MI355X: 8 subjects of 256^3 (fp16 image, uint8
3-class label map), 128^3 patches, class probabilities [0.2, 0.4, 0.4], batches of 4.  Prints one JSON line with the
device sampler's rate, the CPU oracle's (numpy crop, the reference's procedure) and the rate of sampler + training step.
`--spatial [--spatial-out FILE]`: only the spatial-augmentation leg (spatial_leg below; profiles/spatial_augment.md)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "torch-mednet_amd")]
import numpy as np
import torch
import mednet_hip
from mednet_hip.sampler import DevicePatchSampler
from mednet_hip.synth import keyed_init_
from mednet_hip.train import SegmentationStep
from mednet_hip.unet.model import ResidualUNet3D
from oracle import ref_sampler as S

dev = torch.device("cuda", 0)
rng = np.random.default_rng(0)
n_subj, size, patch, probs, B = 8, 256, [128] * 3, [0.2, 0.4, 0.4], 4
images, labels = [], []
for s in range(n_subj):
    images.append(rng.standard_normal((1, size, size, size), dtype=np.float32).astype(np.float16))
    lab = np.zeros((1, size, size, size), dtype=np.uint8)
    for c in (1, 2):
        for _ in range(6):
            z, y, x = rng.integers(0, size - 24, 3)
            lab[0, z:z + 24, y:y + 24, x:x + 24] = c
    labels.append(lab)
ds = DevicePatchSampler(images, labels, patch, samples_per_subject=16, class_probabilities=probs, device=dev)


def spatial_leg(out_path=None):
    """`--spatial`: the spatial augmentation (mednet_warp_patches) at the same 128^3 patches in batches of 4, in this process: crop
    only, crop + intensity, warp with the affine part, warp with affine + elastic, warp + elastic + intensity, the training step
    alone on a fixed batch, and an A/B of the workgroup mapping (tuning option warp_brick).  Rule followed: versions are compared in
    one process and ALTERNATED over several rounds, so that drift and other people's work on the host hit all of them alike; every
    shape is warmed up; each window is closed by a device synchronise (host clock) or bracketed by device events (kernel A/B); the
    spread (min, max over the rounds) is reported next to the median."""
    from mednet_hip import _lib as L
    from mednet_hip.sampler import SpatialAugmentation, warp_patches
    rot = ((-np.pi / 6, np.pi / 6),) * 3
    affine = dict(rotation=rot, scale=(0.7, 1.4), mirror_axes=(0, 1, 2))
    mk = lambda **kw: DevicePatchSampler(images, labels, patch, samples_per_subject=16, class_probabilities=probs, device=dev, **kw)
    legs = {"crop": mk(), "crop_intensity": mk(augment=True), "warp_affine": mk(spatial=SpatialAugmentation(**affine)),
            "warp_affine_elastic": mk(spatial=SpatialAugmentation(elastic=(32, 4.0), **affine)),
            "warp_affine_elastic_intensity": mk(augment=True, spatial=SpatialAugmentation(elastic=(32, 4.0), **affine))}
    np.random.seed(1)
    for s in legs.values():
        for _ in range(3):
            s.batch(range(B))
    torch.cuda.synchronize()
    rounds, per = 5, 10
    times = {k: [] for k in legs}
    for r in range(rounds):
        for k, s in legs.items():
            t0 = time.perf_counter()
            for i in range(per):
                s.batch(range(i * B, i * B + B))
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / per)
    # the training step alone (config-2 network, bf16 storage) on one fixed batch
    mednet_hip.set_precision("bf16")
    net = keyed_init_(ResidualUNet3D(1, 4, False, f_maps=[32, 64, 128, 256])).to(dev)
    step = SegmentationStep(net, loss_weight=[0.05, 1, 1, 1.0])
    fixed = legs["warp_affine_elastic_intensity"].batch(range(B))
    for _ in range(3):
        step(fixed)
    torch.cuda.synchronize()
    step_times = []
    for r in range(3):
        t0 = time.perf_counter()
        for _ in range(10):
            step(fixed)
        torch.cuda.synchronize()
        step_times.append((time.perf_counter() - t0) / 10)
    # kernel A/B of the workgroup mapping: image + label call of one batch, fixed matrices and lattice, device events
    sp = legs["warp_affine_elastic"]
    aff = torch.tensor(sp.last_spatial["affine"].reshape(-1, 12), device=dev)
    disp = torch.tensor(sp.last_spatial["lattice"], device=dev)
    slot = torch.arange(B, dtype=torch.int32, device=dev)
    data = torch.empty((B, 1, *patch), dtype=torch.float32, device=dev)
    label = torch.empty((B, 1, *patch), dtype=torch.uint8, device=dev)

    def both():
        warp_patches(sp.images[0], aff, slot, data, 0, "linear", "edge", 0.0, disp)
        warp_patches(sp.labels[0], aff, slot, label, 0, "nearest", "constant", 0, disp)

    names = {0: "brick 8x8x4 (x,y,z)", 1: "brick 16x4x4", 2: "brick 32x4x2", 3: "row 256x1x1"}
    ab = {v: [] for v in names}
    for v in names:
        L.lib().mednet_set_option(b"warp_brick", v)
        both()
    torch.cuda.synchronize()
    for r in range(7):
        for v in names:
            L.lib().mednet_set_option(b"warp_brick", v)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                both()
            e1.record()
            torch.cuda.synchronize()
            ab[v].append(e0.elapsed_time(e1) / 20)
    L.lib().mednet_set_option(b"warp_brick", 1)    # the default
    ms = lambda v: round(float(np.median(v)) * 1e3, 3)
    step_ms = ms(step_times)
    full = ms(times["warp_affine_elastic_intensity"])
    line = json.dumps({
        "metric": "128^3 training patches/sec with spatial augmentation (mednet_warp_patches), batches of 4",
        "legs": {k: {"patches_per_s": round(B / float(np.median(v)), 1), "ms_per_batch_of_4": ms(v),
                     "ms_min_max": [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)]} for k, v in times.items()},
        "training_step_ms": step_ms, "training_step_ms_min_max": [round(min(step_times) * 1e3, 2), round(max(step_times) * 1e3, 2)],
        "full_augmentation_share_of_step": round(full / step_ms, 4),
        "kernel_ab_ms_per_batch_image_plus_label": {names[v]: {"median": round(float(np.median(t)), 4), "min": round(min(t), 4),
                                                               "max": round(max(t), 4)} for v, t in ab.items()},
        "rounds": rounds, "batches_per_round": per})
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if "--spatial" in sys.argv:
    spatial_leg(sys.argv[sys.argv.index("--spatial-out") + 1] if "--spatial-out" in sys.argv else None)
    sys.exit(0)
np.random.seed(1)
for _ in range(3):
    ds.batch(range(B))
torch.cuda.synchronize()
t0 = time.perf_counter()
nb = 50
for i in range(nb):
    b = ds.batch(range(i * B, i * B + B))
torch.cuda.synchronize()
dt_dev = (time.perf_counter() - t0) / nb
# with the reference's intensity augmentation (train_seg.py:82-86) on the device
dsa = DevicePatchSampler(images, labels, patch, samples_per_subject=16, class_probabilities=probs, device=dev, augment=True)
for _ in range(3):
    dsa.batch(range(B))
torch.cuda.synchronize()
t0 = time.perf_counter()
for i in range(nb):
    b = dsa.batch(range(i * B, i * B + B))
torch.cuda.synchronize()
dt_aug = (time.perf_counter() - t0) / nb
from oracle import ref_augment as A
ora = S.PatchSampler(images, labels, patch, samples_per_subject=16, class_probabilities=probs)
np.random.seed(1)
t0 = time.perf_counter()
for i in range(2):
    items = [ora[j] for j in range(i * B, i * B + B)]
    d = np.stack([a["data"] for a in items])
    A.apply(d, A.draw_parameters(B, d.shape[1]))
dt_cpu_aug = (time.perf_counter() - t0) / 2
np.random.seed(1)
t0 = time.perf_counter()
nc = 6
for i in range(nc):
    items = [ora[j] for j in range(i * B, i * B + B)]
    batch_cpu = {"data": np.stack([a["data"] for a in items]), "label": np.stack([a["label"] for a in items])}
dt_cpu = (time.perf_counter() - t0) / nc
# sampler feeding the training step (config-2 network, bf16 storage)
mednet_hip.set_precision("bf16")
net = keyed_init_(ResidualUNet3D(1, 4, False, f_maps=[32, 64, 128, 256])).to(dev)
step = SegmentationStep(net, loss_weight=[0.05, 1, 1, 1.0])
for i in range(3):
    step(ds.batch(range(B)))
torch.cuda.synchronize()
t0 = time.perf_counter()
ns = 20
for i in range(ns):
    step(ds.batch(range(i * B, i * B + B)))
torch.cuda.synchronize()
dt_train = (time.perf_counter() - t0) / ns
print(json.dumps({"metric": "128^3 training patches/sec sampled (position + crop + cast into batch tensors)",
                  "value": round(B / dt_dev, 1), "unit": "patches/s", "ms_per_batch_of_4": round(dt_dev * 1e3, 3),
                  "cpu_baseline": {"value": round(B / dt_cpu, 2), "unit": "patches/s", "kind": "port",
                                   "sample": f"oracle PatchSampler (numpy crop + stack), {nc} batches of 4, 1 process"},
                  "with_augmentation": {"value": round(B / dt_aug, 1), "unit": "patches/s", "ms_per_batch_of_4": round(dt_aug * 1e3, 3),
                                        "what": "+ brightness / gamma / contrast of train_seg.py:82-86 (mednet_augment_patches)",
                                        "cpu_baseline": {"value": round(B / dt_cpu_aug, 2), "unit": "patches/s", "kind": "port",
                                                         "sample": "oracle sampler + oracle/ref_augment.py (numpy), 2 batches of 4, 1 process"}},
                  "sampler_plus_training_step": {"value": round(B / dt_train, 2), "unit": "patches/s",
                                                 "ms_per_step": round(dt_train * 1e3, 2)}}))
