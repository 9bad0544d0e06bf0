"""Same-box times of validation sample logging at BASELINE shapes (4 x 128^3): config 2 (4 classes) and config 4 (16 heat maps +
2 classes).  Three arms compute what `log_samples` draws, alternating in one process after a warm-up, each between two device
events and ending in a synchronise:
  (a) host      the reference's procedure without matplotlib: the `.cpu().numpy()` copies of log_samples (segmentation.py:69-72,
                landmarks.py:87-94) and the numpy projections / slices of utils/plots.py
  (b) torch     the same panels of sample 0 from torch device ops (argmax, amax, mean), copied to the host
  (c) fused     vis.sample_panels (mednet_sample_panels) + SamplePanels.to_host()
Then the fused kernels alone (bytes they read, from shapes, over their time) and a validation step with and without logging
(bf16 storage, the callback takes the panels to the host).  Prints one JSON line per measurement.
Usage: python tools/vis_panels_timing.py [warmup] [repeats] (defaults 3, 20); VIS_WHICH=cfg2,cfg4,val2,val4 selects."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "torch-mednet_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import mednet_hip  # noqa: E402
from mednet_hip import _lib as L  # noqa: E402
from mednet_hip import vis  # noqa: E402
from mednet_hip.train import LandmarkValidation, SegmentationValidation  # noqa: E402
from mednet_hip.unet import model as HM  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402

WARM = int(sys.argv[1]) if len(sys.argv) > 1 else 3
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
DEV = "cuda:0"
FM = [32, 64, 128, 256]
SHAPE = (128, 128, 128)
CONFIGS = {"cfg2": dict(ncls=4, nh=0), "cfg4": dict(ncls=2, nh=16)}
MIP_AXIS, STEPS = 1, 5


def host_arm(batch, outputs, nh):
    """log_samples + vis_logimages / vis_loglabels / vis_logheatmaps up to (not including) make_grid and imshow."""
    inputs = batch["data"].float().cpu().numpy()
    labels = batch["label"][:, -1, ...].long().cpu().numpy()
    pred = torch.argmax(F.softmax(outputs[:, nh:, ...], dim=1), dim=1).cpu().numpy()
    res = {}
    if nh:
        heatmaps = batch["label"][:, :-1, ...].float().cpu().numpy()
        out_hm = outputs[:, :nh, ...].cpu().numpy()
    x = inputs[0]
    n = x.shape[2]
    res["images"] = np.concatenate([np.stack([x[c, :, i, :] for i in range(0, n, n // STEPS)], axis=0) for c in range(x.shape[0])], axis=0)
    res["pred_mip"], res["label_mip"] = np.max(pred[0], axis=MIP_AXIS), np.max(labels[0], axis=MIP_AXIS)
    res["input_mip"] = x[0].mean(axis=MIP_AXIS)
    if nh:
        res["heatmap_mip"], res["output_heatmap_mip"] = heatmaps[0].max(axis=MIP_AXIS + 1), out_hm[0].max(axis=MIP_AXIS + 1)
    return res


def torch_arm(batch, outputs, nh):
    """What a user of this package could write without the fused kernel: device ops on sample 0, small copies to the host."""
    x = batch["data"].float()[0]
    res = {"pred_mip": outputs[0, nh:].argmax(dim=0).amax(dim=MIP_AXIS).to(torch.uint8), "label_mip": batch["label"][0, -1].amax(dim=MIP_AXIS),
           "input_mip": x[0].mean(dim=MIP_AXIS), "images": x[:, :, ::x.shape[2] // STEPS, :].permute(0, 2, 1, 3).reshape(-1, x.shape[1], x.shape[3])}
    if nh:
        res["heatmap_mip"] = batch["label"][0, :nh].amax(dim=MIP_AXIS + 1).float()
        res["output_heatmap_mip"] = outputs[0, :nh].amax(dim=MIP_AXIS + 1)
    return {k: v.cpu().numpy() for k, v in res.items()}


def fused_arm(batch, outputs, nh):
    return vis.sample_panels(outputs, batch["label"], batch["data"], nh, mip_axis=MIP_AXIS, steps=STEPS).to_host()


def event_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    out = fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1), out


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "stdev_ms": round(statistics.pstdev(ms), 4)}


def alternate(arms):
    """name -> [ms] over REPS rounds in which every arm runs once, after WARM unrecorded rounds."""
    times = {k: [] for k in arms}
    for r in range(WARM + REPS):
        for k, fn in arms.items():
            ms, _ = event_ms(fn)
            if r >= WARM:
                times[k].append(ms)
    return times


def panels_case(name, ncls, nh):
    g = torch.Generator(device="cpu").manual_seed(5)
    batch = {k: v.to(DEV) for k, v in O.synthetic_batch(4, 1, SHAPE, ncls, nh, seed=3).items()}
    outputs = torch.randn((4, nh + ncls) + SHAPE, generator=g).to(DEV)
    arms = {"host": lambda: host_arm(batch, outputs, nh), "torch": lambda: torch_arm(batch, outputs, nh),
            "fused": lambda: fused_arm(batch, outputs, nh)}
    ref, host, fused = arms["torch"](), arms["host"](), arms["fused"]()
    for key, want in ref.items():  # the three arms draw the same picture
        if key == "input_mip":
            assert np.allclose(fused[key], want, rtol=0, atol=1e-5) and np.allclose(host[key], want, rtol=0, atol=1e-5), key
        else:
            assert np.array_equal(fused[key], want), key
            if key != "pred_mip":
                assert np.array_equal(host[key], want), key
    # (the host arm takes the arg-max of the SOFT-MAXED logits, as the reference does: two logits one ulp apart can round to one
    #  probability and give the other index -- counted, not asserted)
    soft = int((host["pred_mip"] != ref["pred_mip"]).sum())
    times = alternate(arms)
    sp = SHAPE[0] * SHAPE[1] * SHAPE[2]
    host_bytes = 4 * sp * (4 + 8 + 8 + (nh * 4 * 2))  # data fp32, labels int64, arg-max int64, float heat maps, raw heat-map outputs
    for k, ms in times.items():
        print(json.dumps({"case": name, "arm": k, **spread(ms), "repeats": REPS, "warmup": WARM,
                          **({"d2h_bytes": host_bytes, "pred_mip_pixels_changed_by_softmax_rounding": soft} if k == "host" else {})}), flush=True)
    # the fused launches alone: every byte they read, from shapes (logit planes, input, class map, target heat maps)
    read_bytes = sp * ((nh + ncls) * 4 + 4 + 1 + nh)
    ws_bytes = 2 * L.lib().mednet_sample_panels_ws_bytes(*SHAPE, nh, MIP_AXIS)  # partials, written and read once
    ms = []
    for r in range(WARM + REPS):
        t, _ = event_ms(lambda: [vis.sample_panels(outputs, batch["label"], batch["data"], nh, mip_axis=MIP_AXIS) for _ in range(10)])
        if r >= WARM:
            ms.append(t / 10)
    s = spread(ms)
    print(json.dumps({"case": name, "arm": "fused launches only (10 per timing, includes the image-slice copy)", **s,
                      "source_bytes_read": read_bytes, "partial_bytes_moved": ws_bytes,
                      "source_GB_per_s": round(read_bytes / (s["median_ms"] * 1e-3) / 1e9, 1)}), flush=True)


def validation_case(name, ncls, nh):
    with mednet_hip.precision("bf16"):
        net = O.keyed_init_(HM.ResidualUNet3D(in_channels=1, out_channels=nh + ncls, final_sigmoid=False, f_maps=FM)).to(DEV)
        batch = {k: v.to(DEV) for k, v in O.synthetic_batch(4, 1, SHAPE, ncls, nh, seed=4).items()}
        log = dict(log_interval=1, on_samples=lambda panels, nb: panels.to_host())
        if nh:
            kw = dict(class_weight=[0.05] + [1.0] * (ncls - 1), regression_weight=[0.015] * nh)
            plain, logged = LandmarkValidation(net, **kw), LandmarkValidation(net, **kw, **log)
        else:
            w = [0.05] + [1.0] * (ncls - 1)
            plain, logged = SegmentationValidation(net, loss_weight=w), SegmentationValidation(net, loss_weight=w, **log)
        times = alternate({"unlogged": lambda: plain.validation_step(batch, 0), "logged": lambda: logged.validation_step(batch, 0)})
    a, b = spread(times["unlogged"]), spread(times["logged"])
    print(json.dumps({"case": name, "unlogged": a, "logged": b, "extra_ms": round(b["median_ms"] - a["median_ms"], 4),
                      "repeats": REPS, "warmup": WARM}), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "vis_panels_timing.py measures on the GPU"
    which = os.environ.get("VIS_WHICH", "cfg2,cfg4,val2,val4")
    for key, cfg in CONFIGS.items():
        if key in which:
            panels_case(f"{key} panels", **cfg)
    for key, cfg in (("val2", CONFIGS["cfg2"]), ("val4", CONFIGS["cfg4"])):
        if key in which:
            validation_case(f"config {key[-1]} validation step, bf16", **cfg)
