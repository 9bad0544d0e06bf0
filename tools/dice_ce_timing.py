"""Same-box step times of the class-loss kinds at BASELINE shapes (bf16 storage, 128^3, batch 4, graph on): SegmentationStep on
ResidualUNet3D(1, C, f_maps=[32, 64, 128, 256]) and LandmarkStep on config 4 (16 heat maps + 2 classes) with "DICE_CE", "DICE" or "CE",
the fused head + loss node on or off (off: the two-node path; for "DICE_CE" final_conv + the one-pass loss).  One JSON line per case:
the mean step time and the means of five consecutive blocks of the timed steps (their range is the spread inside the run).
Usage: python tools/dice_ce_timing.py [warmup] [steps] (defaults 10, 50); DCE_CASES picks the cases, comma separated, each
<workload>:<loss>:<fused> with workload seg<C> or ldmk, e.g. DCE_CASES=seg4:DICE_CE:1,seg4:DICE_CE:0,seg4:DICE:1,ldmk:DICE_CE:1.
DCE_GRAPH=0 times the eager step.  Per-kernel times: rocprofv3 --kernel-trace --stats --output-format csv -- python
tools/dice_ce_timing.py 4 20 with one case, no counters in that run."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "torch-mednet_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import mednet_hip  # noqa: E402
from mednet_hip import ops  # noqa: E402
from mednet_hip.train import LandmarkStep, SegmentationStep  # noqa: E402
from mednet_hip.unet import model as HM  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402

WARM = int(sys.argv[1]) if len(sys.argv) > 1 else 10
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 50
GRAPH = os.environ.get("DCE_GRAPH", "1") == "1"
BLOCKS = 5
DEV = "cuda:0"
F = [32, 64, 128, 256]
NODES = ("HeadDiceFn", "HeadCEFn", "HeadDiceCEFn", "HeadSegFn", "HeadLandmarkFn", "DiceCELossFn")


def make(workload, loss):
    if workload == "ldmk":
        net = O.keyed_init_(HM.ResidualUNet3D(in_channels=1, out_channels=18, final_sigmoid=False, f_maps=F)).to(DEV)
        step = LandmarkStep(net, class_weight=[0.05, 1.0], regression_weight=[0.015] * 16, regression="L2", lr=1e-3, class_loss=loss,
                            graph=GRAPH)
        return step, O.synthetic_batch(4, 1, (128,) * 3, 2, 16, seed=2)
    c = int(workload[3:])
    net = O.keyed_init_(HM.ResidualUNet3D(in_channels=1, out_channels=c, final_sigmoid=False, f_maps=F)).to(DEV)
    return SegmentationStep(net, loss_weight=[0.05] + [1.0] * (c - 1), lr=1e-3, loss=loss, graph=GRAPH), \
        O.synthetic_batch(4, 1, (128,) * 3, c, 0, seed=1)


def timed(workload, loss, fused):
    ops.FUSE_HEAD_LOSS = fused
    taken, reals = set(), {}
    for name in NODES:  # which autograd nodes the step takes (the eager warm-up calls and the capture go through them)
        cls = getattr(ops, name)
        reals[name] = cls.apply

        def counted(*a, _name=name):
            taken.add(_name)
            return reals[_name](*a)
        cls.apply = counted
    try:
        with mednet_hip.precision("bf16"):
            step, batch = make(workload, loss)
            batch = {k: v.to(DEV) for k, v in batch.items()}
            for _ in range(WARM):
                step(batch)
            torch.cuda.synchronize()
            per, blocks = max(1, STEPS // BLOCKS), []
            for _ in range(BLOCKS):
                t0 = time.perf_counter()
                for _ in range(per):
                    out = step(batch)
                torch.cuda.synchronize()
                blocks.append((time.perf_counter() - t0) / per * 1e3)
            ms = sum(blocks) / len(blocks)
            loss_value = float(out[0] if isinstance(out, tuple) else out)
            step.flat.release()
    finally:
        for name in NODES:
            getattr(ops, name).apply = reals[name]
    print(json.dumps({"case": f"{workload}:{loss}:{int(fused)}", "nodes": sorted(taken), "graph": GRAPH, "ms_per_step": round(ms, 3),
                      "patches_per_s": round(4e3 / ms, 2), "block_ms": [round(b, 3) for b in blocks],
                      "spread_ms": round(max(blocks) - min(blocks), 3), "warmup": WARM, "steps": per * BLOCKS, "last_loss": loss_value}),
          flush=True)
    del step, batch
    torch.cuda.empty_cache()


for case in os.environ.get("DCE_CASES", "seg4:DICE_CE:1,seg4:DICE_CE:0,seg4:DICE:1,seg14:DICE_CE:1,seg14:DICE_CE:0,seg14:DICE:1").split(","):
    w, k, f = case.split(":")
    timed(w, k, bool(int(f)))
