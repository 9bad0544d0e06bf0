"""Same-box times of the optimiser options (profiles/optim.md).

  launch   every optimiser launch ALONE on flat buffers of config 2's and config 5's parameter counts (device events around `reps`
           back-to-back launches; config 5's four buffers of 565 MB are far larger than the 256 MiB Infinity Cache, config 2's four of
           35 MB fit into it, which a launch inside a training step cannot count on): the existing Adam and scaled-Adam entries, the
           norm pass, SGD (momentum + Nesterov) without and behind the norm pass, AdamW behind it; with the bytes each moves per
           element and the achieved bytes/s
  adam     the whole step at config 2 (bf16, 128^3, batch 4) with the default optimiser -- the case a parent commit's package can run too
  sgd      the same step with optimizer="sgd" (momentum 0.99, Nesterov, weight decay 3e-5), PolyLR and clip_grad_norm=12
  adamw    the same step with optimizer="adamw" (weight decay 1e-2) and clip_grad_norm=12

Usage: python tools/optim_timing.py [warmup] [steps] (defaults 10, 50).  OPT_CASES=launch,adam,sgd,adamw picks the cases, one JSON line
each.  To time another commit's package and library on the same box (the tools/ab_lib.sh way): OPT_PKG=<directory that holds that
commit's mednet_hip/> MEDNET_LIB_PATH=<its libmednet_hip.so> OPT_CASES=adam python tools/optim_timing.py."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("OPT_PKG") or os.path.join(ROOT, "torch-mednet_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import mednet_hip  # noqa: E402
from mednet_hip import _lib as L  # noqa: E402
from mednet_hip import ops, train  # noqa: E402
from mednet_hip.unet import model as HM  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402

WARM = int(sys.argv[1]) if len(sys.argv) > 1 else 10
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 50
BLOCKS = 5
DEV = "cuda:0"
F_MAPS = {"config2": [32, 64, 128, 256], "config5": [64, 128, 256, 512, 1024]}


def flat_count(f_maps):
    """Elements of the flat buffer train.FlatParams lays out for that network (64-element aligned slices); no memory is touched."""
    with torch.device("meta"):
        net = HM.ResidualUNet3D(in_channels=1, out_channels=4, final_sigmoid=False, f_maps=f_maps)
    return sum((p.numel() + 63) // 64 * 64 for p in net.parameters() if p.requires_grad)


def launches(name, count, reps=40):
    g = torch.Generator(device=DEV).manual_seed(1)
    p, gr, m = (torch.randn(count, device=DEV, generator=g) for _ in range(3))
    v = torch.rand(count, device=DEV, generator=g) * 0.01
    gr *= 1e-3
    ost, sc = ops.new_opt_state(DEV), train.LossScaler(DEV)
    sc.state[0] = 1.0
    hp = (1e-3, 0.9, 0.999, 1e-8)
    lib = L.lib()

    def scaled():
        L.check(lib.mednet_adam_step_scaled(p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), count, *hp, 0.0, 1.0, sc.state.data_ptr(),
                                            2.0, 0.5, 2000, L.stream()), "adam_step_scaled")

    def norm_then(update):
        ops.grad_norm_(gr, ost, 12.0)
        update()

    sgd = lambda o: ops.sgd_step_(p, gr, m, 1e-3, 0.99, True, 3e-5, 1.0, o)
    adamw = lambda: ops.adamw_step_(p, gr, m, v, *hp, 1e-2, ost, True)
    cases = [("adam_step (existing)", 28, lambda: ops.adam_step_(p, gr, m, v, *hp, 0.0, 7)),
             ("adam_step_scaled (existing: sweep + update + scaler)", 32, scaled),
             ("grad_norm", 4, lambda: ops.grad_norm_(gr, ost, 12.0)),
             ("sgd_step momentum nesterov, unguarded", 20, lambda: sgd(None)),
             ("grad_norm + sgd_step", 24, lambda: norm_then(lambda: sgd(ost))),
             ("grad_norm + adamw_step", 32, lambda: norm_then(adamw)),
             ("adamw_step alone (state from an earlier norm pass)", 28, adamw)]
    out = {"case": "launch", "buffers": name, "count": count, "reps": reps, "rows": []}
    for what, bytes_per_elt, fn in cases:
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(3):                       # three windows: their range is the spread
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / reps * 1e3)
        us = min(times)
        out["rows"].append({"launch": what, "bytes_per_element": bytes_per_elt, "us": round(us, 1), "us_windows": [round(t, 1) for t in times],
                            "TB_per_s": round(bytes_per_elt * count / (us * 1e-6) / 1e12, 2)})
    assert float(ost[3]) == 0.0 and bool(torch.isfinite(p).all())
    print(json.dumps(out), flush=True)
    del p, gr, m, v
    torch.cuda.empty_cache()


def timed(case):
    kw = {"adam": {},
          "sgd": dict(optimizer="sgd", optimizer_args=dict(momentum=0.99, nesterov=True, weight_decay=3e-5),
                      lr=train.PolyLR(1e-2, 100000) if hasattr(train, "PolyLR") else 1e-2, clip_grad_norm=12.0),
          "adamw": dict(optimizer="adamw", optimizer_args=dict(weight_decay=1e-2), clip_grad_norm=12.0)}[case]
    with mednet_hip.precision("bf16"):
        net = O.keyed_init_(HM.ResidualUNet3D(in_channels=1, out_channels=4, final_sigmoid=False, f_maps=F_MAPS["config2"])).to(DEV)
        step = train.SegmentationStep(net, loss_weight=[0.05, 1.0, 1.0, 1.0], **({"lr": 1e-3, **kw}))
        batch = {k: v.to(DEV) for k, v in O.synthetic_batch(4, 1, (128,) * 3, 4, 0, seed=1).items()}
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
        extra = {}
        if case != "adam":
            extra = {"grad_norm": float(step.grad_norm), "skipped_steps": step.skipped_steps()}
        loss = float(loss)
        step.flat.release()
    print(json.dumps({"case": case, "package": os.path.dirname(os.path.abspath(mednet_hip.__file__)), "library": L.LIB_PATH,
                      "ms_per_step": round(ms, 3), "patches_per_s": round(4e3 / ms, 2), "block_ms": [round(b, 3) for b in blocks],
                      "spread_ms": round(max(blocks) - min(blocks), 3), "warmup": WARM, "steps": per * BLOCKS, "last_loss": loss, **extra}),
          flush=True)
    del step, net, batch
    torch.cuda.empty_cache()


for c in os.environ.get("OPT_CASES", "launch,adam,sgd,adamw").split(","):
    if c == "launch":
        for name, f_maps in F_MAPS.items():
            launches(name, flat_count(f_maps))
    else:
        timed(c)
