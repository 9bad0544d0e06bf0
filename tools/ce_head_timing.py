"""Same-box step times of the class-loss choices at BASELINE shapes (bf16 storage, 128^3, batch 4): config 2 with loss="CE" and
config 4 with class_loss="CE", each with the fused CE head and with MEDNET_FUSE_HEAD_LOSS off (the two-node path), back to back in
one process, and config 4 with Dice beside them.  Prints one JSON line per case.  Usage: python tools/ce_head_timing.py [warmup]
[steps] (defaults 10, 50).  CE_WHICH=cfg2ce,cfg4ce,cfg4dice picks the cases, CE_FUSED=1,0 the head forms.  To time another commit's
package and library on the same box (the tools/ab_lib.sh way): CE_PKG=<directory that holds that commit's mednet_hip/>
MEDNET_LIB_PATH=<its libmednet_hip.so> python tools/ce_head_timing.py."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("CE_PKG") or os.path.join(ROOT, "torch-mednet_amd")
for p in (ROOT, PKG):
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
DEV = "cuda:0"
F = [32, 64, 128, 256]


def seg(loss):
    net = O.keyed_init_(HM.ResidualUNet3D(in_channels=1, out_channels=4, final_sigmoid=False, f_maps=F)).to(DEV)
    return SegmentationStep(net, loss_weight=[0.05, 1.0, 1.0, 1.0], lr=1e-3, loss=loss), O.synthetic_batch(4, 1, (128,) * 3, 4, 0, seed=1)


def ldmk(class_loss):
    net = O.keyed_init_(HM.ResidualUNet3D(in_channels=1, out_channels=18, final_sigmoid=False, f_maps=F)).to(DEV)
    step = LandmarkStep(net, class_weight=[0.05, 1.0], regression_weight=[0.015] * 16, regression="L2", lr=1e-3, class_loss=class_loss)
    return step, O.synthetic_batch(4, 1, (128,) * 3, 2, 16, seed=2)


def timed(name, make, fused):
    ops.FUSE_HEAD_LOSS = fused
    with mednet_hip.precision("bf16"):
        step, batch = make()
        batch = {k: v.to(DEV) for k, v in batch.items()}
        for _ in range(WARM):
            step(batch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            out = step(batch)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / STEPS
        loss = float(out[0] if isinstance(out, tuple) else out)
        step.flat.release()
    print(json.dumps({"case": name, "fused_head": fused, "package": os.path.dirname(os.path.abspath(mednet_hip.__file__)),
                      "ms_per_step": round(dt * 1e3, 3), "patches_per_s": round(4 / dt, 2),
                      "warmup": WARM, "steps": STEPS, "last_loss": loss}), flush=True)


which = os.environ.get("CE_WHICH", "cfg2ce,cfg4ce,cfg4dice")
forms = [bool(int(f)) for f in os.environ.get("CE_FUSED", "1,0").split(",")]
if "cfg2ce" in which:
    for fused in forms:
        timed("cfg2 loss=CE", lambda: seg("CE"), fused)
if "cfg4ce" in which:
    for fused in forms:
        timed("cfg4 class_loss=CE", lambda: ldmk("CE"), fused)
if "cfg4dice" in which:
    timed("cfg4 class_loss=DICE", lambda: ldmk("DICE"), True)
