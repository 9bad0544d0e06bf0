"""Same-box step times of multi-channel network inputs: SegmentationStep on ResidualUNet3D(c, 4, f_maps=[32, 64, 128, 256]) at
128^3, batch 4, bf16 storage, for c = 1, 2, 4 input channels; cases back to back in one process.  Prints one JSON line per case:
the mean step time, and the means of the timed steps taken in five consecutive blocks (their range is the spread inside a run
quoted in profiles/multichannel_input.md).
Usage: python tools/multichannel_timing.py [warmup] [steps] (defaults 10, 50).  MC_CHANNELS=1,2,4 picks the cases.  To time another
commit's package and library on the same box (the tools/ab_lib.sh way): MC_PKG=<directory that holds that commit's mednet_hip/>
MEDNET_LIB_PATH=<its libmednet_hip.so> python tools/multichannel_timing.py.  The per-kernel times of the first layer come from
MC_CHANNELS=4 rocprofv3 --kernel-trace --stats --output-format csv -- python tools/multichannel_timing.py 3 5."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("MC_PKG") or os.path.join(ROOT, "torch-mednet_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import mednet_hip  # noqa: E402
from mednet_hip.train import SegmentationStep  # noqa: E402
from mednet_hip.unet import model as HM  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402

WARM = int(sys.argv[1]) if len(sys.argv) > 1 else 10
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 50
BLOCKS = 5
DEV = "cuda:0"


def timed(c):
    with mednet_hip.precision("bf16"):
        net = O.keyed_init_(HM.ResidualUNet3D(in_channels=c, out_channels=4, final_sigmoid=False, f_maps=[32, 64, 128, 256])).to(DEV)
        step = SegmentationStep(net, loss_weight=[0.05, 1.0, 1.0, 1.0], lr=1e-3)
        batch = {k: v.to(DEV) for k, v in O.synthetic_batch(4, c, (128,) * 3, 4, 0, seed=1).items()}
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
    print(json.dumps({"case": f"c={c}", "package": os.path.dirname(os.path.abspath(mednet_hip.__file__)), "ms_per_step": round(ms, 3),
                      "patches_per_s": round(4e3 / ms, 2), "block_ms": [round(b, 3) for b in blocks],
                      "spread_ms": round(max(blocks) - min(blocks), 3), "warmup": WARM, "steps": per * BLOCKS, "last_loss": loss}),
          flush=True)
    del step, net, batch
    torch.cuda.empty_cache()


for ch in os.environ.get("MC_CHANNELS", "1,2,4").split(","):
    timed(int(ch))
