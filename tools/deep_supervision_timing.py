"""Same-box step times of deep supervision: SegmentationStep on ResidualUNet3D(1, C, f_maps=[32, 64, 128, 256], deep_supervision=k) at
128^3, batch 4, bf16 storage, for C = 4 and 14 and three forms alternating in one process: "fused" (ops.ds_head at the junctions),
"composed" (library option ds_head_fuse=0: the auxiliary head, a strided label copy and the stock loss per level, autograd adding the
two feature gradients) and "off" (the same network without deep supervision).  Prints one JSON line per case: the mean step time,
the means of the timed steps taken in five consecutive blocks (their range is the spread inside a run quoted in
profiles/deep_supervision.md), and how the blocks' backward passes found their GroupNorm-3 sums in one step (ops.GN3_COUNT).
Usage: python tools/deep_supervision_timing.py [warmup] [steps] (defaults 10, 50).  DS_CLASSES=4,14 picks the class counts,
DS_FORMS=fused,composed,off the forms, DS_LOSS=DICE|CE|DICE_CE the loss (default DICE_CE), DS_DEPTH the depth k (default 2).
Per-kernel times: DS_CLASSES=14 DS_FORMS=fused rocprofv3 --kernel-trace --stats --output-format csv -- python
tools/deep_supervision_timing.py 3 5."""
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
from mednet_hip import _lib as L  # noqa: E402
from mednet_hip import ops  # noqa: E402
from mednet_hip.train import SegmentationStep  # noqa: E402
from mednet_hip.unet import model as HM  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402

WARM = int(sys.argv[1]) if len(sys.argv) > 1 else 10
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 50
BLOCKS = 5
DEV = "cuda:0"
LOSS = os.environ.get("DS_LOSS", "DICE_CE")
DEPTH = int(os.environ.get("DS_DEPTH", "2"))


def timed(c, form):
    L.lib().mednet_set_option(b"ds_head_fuse", 0 if form == "composed" else 1)
    try:
        with mednet_hip.precision("bf16"):
            kw = {} if form == "off" else dict(deep_supervision=DEPTH)
            net = O.keyed_init_(HM.ResidualUNet3D(in_channels=1, out_channels=c, final_sigmoid=False, f_maps=[32, 64, 128, 256], **kw)).to(DEV)
            step = SegmentationStep(net, loss_weight=[0.05] + [1.0] * (c - 1), lr=1e-3, loss=LOSS)
            batch = {k: v.to(DEV) for k, v in O.synthetic_batch(4, 1, (128,) * 3, c, 0, seed=1).items()}
            for _ in range(WARM):
                step(batch)
            torch.cuda.synchronize()
            before = dict(ops.GN3_COUNT)
            step(batch)
            torch.cuda.synchronize()
            gn3 = {k: ops.GN3_COUNT[k] - before[k] for k in before}
            per, blocks = max(1, STEPS // BLOCKS), []
            for _ in range(BLOCKS):
                t0 = time.perf_counter()
                for _ in range(per):
                    loss = step(batch)
                torch.cuda.synchronize()
                blocks.append((time.perf_counter() - t0) / per * 1e3)
            ms = sum(blocks) / len(blocks)
            loss = float(loss)
            levels = [float(v) for v in step.scale_losses]
            step.flat.release()
    finally:
        L.lib().mednet_set_option(b"ds_head_fuse", 1)
    print(json.dumps({"case": f"C={c} {form}", "classes": c, "form": form, "depth": 0 if form == "off" else DEPTH, "loss_kind": LOSS,
                      "ms_per_step": round(ms, 3), "patches_per_s": round(4e3 / ms, 2), "block_ms": [round(b, 3) for b in blocks],
                      "spread_ms": round(max(blocks) - min(blocks), 3), "gn3_count": gn3, "warmup": WARM, "steps": per * BLOCKS,
                      "last_loss": loss, "level_losses": levels}), flush=True)
    del step, net, batch
    torch.cuda.empty_cache()


for cls in os.environ.get("DS_CLASSES", "4,14").split(","):
    for f in os.environ.get("DS_FORMS", "fused,composed,off").split(","):
        timed(int(cls), f)
