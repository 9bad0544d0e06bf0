"""Same-box step times of the segmentation head by class count: SegmentationStep on ResidualUNet3D(1, C, f_maps=[32, 64, 128, 256]) at
128^3, batch 4, bf16 storage, Dice, for C = 4 (control: the <= 4-class node either way), 5, 8, 14, 16; each class count with the
library option head_seg_mfma 1 (the matrix-core head + loss node) and 0 (1x1x1 head and loss as two nodes) alternating in one
process.  Prints one JSON line per case: the mean step time and the means of the timed steps taken in five consecutive blocks (their
range is the spread inside a run quoted in profiles/seg_heads.md).
Usage: python tools/seg_heads_timing.py [warmup] [steps] (defaults 10, 50).  SEG_CLASSES=4,5,8,14,16 picks the class counts,
SEG_SETTINGS=1,0 the option values, SEG_LOSS=DICE|CE the loss.  To time another commit's package and library on the same box (the
tools/ab_lib.sh way): SEG_PKG=<directory that holds that commit's mednet_hip/> MEDNET_LIB_PATH=<its libmednet_hip.so> SEG_SETTINGS=1
python tools/seg_heads_timing.py.  Per-kernel times: SEG_CLASSES=14 SEG_SETTINGS=1 rocprofv3 --kernel-trace --stats --output-format
csv -- python tools/seg_heads_timing.py 3 5 (and once more with SEG_SETTINGS=0)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("SEG_PKG") or os.path.join(ROOT, "torch-mednet_amd")
for p in (ROOT, PKG):
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
LOSS = os.environ.get("SEG_LOSS", "DICE")


def timed(c, setting):
    L.lib().mednet_set_option(b"head_seg_mfma", setting)
    fn = getattr(ops, "HeadSegFn", None)  # (absent in a package from before the wide node)
    calls = {"n": 0}
    if fn is not None:
        real = fn.apply

        def counted(*a):
            calls["n"] += 1
            return real(*a)
        fn.apply = counted
    try:
        with mednet_hip.precision("bf16"):
            net = O.keyed_init_(HM.ResidualUNet3D(in_channels=1, out_channels=c, final_sigmoid=False, f_maps=[32, 64, 128, 256])).to(DEV)
            step = SegmentationStep(net, loss_weight=[0.05] + [1.0] * (c - 1), lr=1e-3, loss=LOSS)
            batch = {k: v.to(DEV) for k, v in O.synthetic_batch(4, 1, (128,) * 3, c, 0, seed=1).items()}
            for _ in range(WARM):
                step(batch)
            torch.cuda.synchronize()
            per, blocks = max(1, STEPS // BLOCKS), []
            for _ in range(BLOCKS):
                t0 = time.perf_counter()
                for _ in range(per):
                    loss = step(batch)
                torch.cuda.synchronize()
                blocks.append((time.perf_counter() - t0) / per * 1e3)
            ms = sum(blocks) / len(blocks)
            loss = float(loss)
            step.flat.release()
    finally:
        if fn is not None:
            fn.apply = real
        L.lib().mednet_set_option(b"head_seg_mfma", 1)
    print(json.dumps({"case": f"C={c} head_seg_mfma={setting}", "classes": c, "head_seg_mfma": setting, "wide_node": calls["n"] > 0,
                      "loss_kind": LOSS, "package": os.path.dirname(os.path.abspath(mednet_hip.__file__)), "ms_per_step": round(ms, 3),
                      "patches_per_s": round(4e3 / ms, 2), "block_ms": [round(b, 3) for b in blocks],
                      "spread_ms": round(max(blocks) - min(blocks), 3), "warmup": WARM, "steps": per * BLOCKS, "last_loss": loss}),
          flush=True)
    del step, net, batch
    torch.cuda.empty_cache()


for cls in os.environ.get("SEG_CLASSES", "4,5,8,14,16").split(","):
    for s in os.environ.get("SEG_SETTINGS", "1,0").split(","):
        timed(int(cls), int(s))
