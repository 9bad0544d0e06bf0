"""SHA-256 digests of what the optimisers and the training / validation step classes compute (mednet_hip/train.py, csrc/optim.hip) on
seeded inputs: two commits whose host code launches the same kernels with the same arguments print the same lines.  Only names that
every commit since the optimisers landed has are used, so the tool runs against any such commit's package and library:
HD_PKG=<directory that holds that commit's mednet_hip/> MEDNET_LIB_PATH=<its libmednet_hip.so> python tools/train_digest.py
(as tools/norm_digest.py); without them it takes this tree's.  One process per package; compare the outputs with diff.

One JSON line per case: its name and ONE SHA-256 over the digests of everything it hashes (DIGEST_FULL=1 adds each tensor's digest).
Families:
  launch  every optimiser entry on flat buffers, three consecutive calls, p / moments / optimiser state / scaler state hashed after
          each.  Counts 1, 3, 255, 1025, 4101 and 2048 * 1024 + 1029 (two trips of the update grid), each behind a pointer 0 and 1
          float past a 16-byte boundary (the 16-byte and the scalar walk).  mednet_adam_step at steps 1, 2, 1000 (wd 0 / 0.01,
          grad_scale 1 / 1/3) and once at 2 * 8192 * 1024 + 1027, past the cap of its own grid; mednet_adam_step_scaled clean, with a
          non-finite element first / last in the second call, and at growth interval 2; grad_norm with and without a scaler state;
          sgd_step plain / momentum / Nesterov x wd 0 / 0.5 x unguarded / guarded / behind a scaler; adamw_step decoupled or not, with
          and without a scaler.  Every guarded sequence has a non-finite gradient in its second call.
  step    SegmentationStep and LandmarkStep, three calls on the nets of tests/test_gpu_optim.py::_step_case (ResidualUNet3D, f_maps
          [16, 32], 16^3, batch 2) in fp32 / bf16 / fp16 storage x DICE / CE / DICE_CE x {default Adam; AdamW + weight decay +
          clipping; SGD + Nesterov + PolyLR + clipping; skip_nonfinite with an out-of-range label in the second batch}; a 6-class head
          on f_maps [32, 64] (the matrix-core head_seg route; bf16, fp16); deep_supervision=1 (f_maps [16, 32, 64]); graph=True (two eager calls, capture,
          one more replay) for one case of each class; a state_dict round trip after call 2 into a fresh step whose call 3 is hashed.
  val     SegmentationValidation / LandmarkValidation.validation_step on the same nets, DICE / CE / DICE_CE, bf16 and fp32, with a
          logging callback (panels.to_host() hashed).
Usage: python tools/train_digest.py [families, default launch,step,val] > digest.jsonl"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("HD_PKG") or os.path.join(ROOT, "torch-mednet_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mednet_hip  # noqa: E402
from mednet_hip import _lib as L  # noqa: E402
from mednet_hip import ops, train  # noqa: E402
from mednet_hip.unet import model as HM  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402

DEV = "cuda:0"
FULL = os.environ.get("DIGEST_FULL", "0") == "1"
FAMILIES = (sys.argv[1] if len(sys.argv) > 1 else "launch,step,val").split(",")
COUNTS = (1, 3, 255, 1025, 4101, 2048 * 1024 + 1029)
ADAM_CAP_COUNT = 2 * 8192 * 1024 + 1027
HP = (1e-3, 0.9, 0.999, 1e-8)
_CACHE = {}


def rnd(tag, count):
    """Seeded on the CPU by the tag alone; cached, so every case of a count sees the same tensor."""
    if (tag, count) not in _CACHE:
        g = torch.Generator().manual_seed(int.from_bytes(hashlib.sha256(tag.encode()).digest()[:6], "little"))
        _CACHE[(tag, count)] = torch.randn(count, generator=g, dtype=torch.float32)
    return _CACHE[(tag, count)]


def digest(t):
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        return hashlib.sha256(np.ascontiguousarray(t).tobytes()).hexdigest()
    if not torch.is_tensor(t):
        return repr(t)
    t = t.detach().contiguous().cpu()
    if t.dtype in (torch.bfloat16, torch.float16):
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def emit(name, res):
    line = {"case": name, "tensors": len(res), "sha256": hashlib.sha256("".join(f"{k}={v};" for k, v in res.items()).encode()).hexdigest()}
    print(json.dumps({**line, **res} if FULL else line), flush=True)


# ================================================================================================ launch
def placed(t, off):
    """`t` on the device behind a pointer `off` floats past a 16-byte boundary."""
    buf = torch.zeros(t.numel() + 4, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + t.numel()]
    view.copy_(t)
    return view


def scaler(interval=2000):
    sc = train.LossScaler(DEV, init_scale=1024.0, growth_interval=interval)
    return sc


def grad(count, off, call, scale=1.0, bad=None):
    g = rnd(f"g{call}", count) * (1e-2 * scale)
    if bad == "first":
        g[0] = float("inf")
    elif bad == "last":
        g[-1] = float("nan")
    return placed(g, off)


def state(count, off, names):
    return {k: placed(rnd(k, count).abs() * 1e-3 if k == "v" else rnd(k, count), off) for k in names}


def sweep(fn, counts=COUNTS):
    """fn(count, off, put) over every count and both alignments; put(key, tensor) records a digest."""
    res = {}
    for count in counts:
        for off in (0, 1):
            fn(count, off, lambda k, t: res.__setitem__(f"{count}+{off}/{k}", digest(t)))
            torch.cuda.synchronize()
    return res


def launch_family():
    # ---- mednet_adam_step
    for wd, gs in ((0.0, 1.0), (0.01, 1.0 / 3.0)):
        def run(count, off, put):
            st = state(count, off, ("p", "m", "v"))
            for call, step in enumerate((1, 2, 1000)):
                ops.adam_step_(st["p"], grad(count, off, call), st["m"], st["v"], *HP, wd, step, gs)
                for k, t in st.items():
                    put(f"{call}/{k}", t)
        emit(f"launch adam_step wd={wd} grad_scale={gs:.4f}", sweep(run))
    emit("launch adam_step past the grid cap", sweep(run, (ADAM_CAP_COUNT,)))
    _CACHE.clear()

    # ---- mednet_adam_step_scaled
    for what, bad, interval in (("clean", None, 2000), ("nonfinite first", "first", 2000), ("nonfinite last", "last", 2000),
                                ("growth interval 2", None, 2)):
        def run(count, off, put):
            st, sc = state(count, off, ("p", "m", "v")), scaler(interval)
            for call in range(3):
                g = grad(count, off, call, float(sc.state[0]), bad if call == 1 else None)
                L.check(L.lib().mednet_adam_step_scaled(st["p"].data_ptr(), g.data_ptr(), st["m"].data_ptr(), st["v"].data_ptr(), count,
                                                        *HP, 0.01, 0.5, sc.state.data_ptr(), sc.growth_factor, sc.backoff_factor,
                                                        sc.growth_interval, L.stream()), "adam_step_scaled")
                for k, t in st.items():
                    put(f"{call}/{k}", t)
                put(f"{call}/scaler", sc.state)
        emit(f"launch adam_step_scaled {what}", sweep(run))

    # ---- grad_norm
    for with_sc in (False, True):
        def run(count, off, put):
            ost, sc = ops.new_opt_state(DEV), scaler() if with_sc else None
            for call in range(3):
                g = grad(count, off, call, 1024.0 if with_sc else 1.0, "last" if call == 1 else None)
                ops.grad_norm_(g, ost, 0.05 if call else None, 0.5, None if sc is None else sc.state)
                put(f"{call}/ost", ost)
                put(f"{call}/scaler", None if sc is None else sc.state)
        emit(f"launch grad_norm scaler={int(with_sc)}", sweep(run))

    # ---- sgd_step
    for mom, nesterov in ((0.0, False), (0.9, False), (0.9, True)):
        for wd in (0.0, 0.5):
            for form in ("unguarded", "guarded", "scaler"):
                def run(count, off, put):
                    st = state(count, off, ("p", "buf") if mom else ("p",))
                    ost = None if form == "unguarded" else ops.new_opt_state(DEV)
                    sc = scaler(2) if form == "scaler" else None
                    for call in range(3):
                        g = grad(count, off, call, 1.0 if sc is None else float(sc.state[0]), "first" if ost is not None and call == 1 else None)
                        if ost is not None:
                            ops.grad_norm_(g, ost, 0.05, 0.5, None if sc is None else sc.state)
                        ops.sgd_step_(st["p"], g, st.get("buf"), 1e-2, mom, nesterov, wd, 0.5, ost, sc)
                        for k, t in st.items():
                            put(f"{call}/{k}", t)
                        put(f"{call}/ost", ost)
                        put(f"{call}/scaler", None if sc is None else sc.state)
                emit(f"launch sgd_step momentum={mom} nesterov={int(nesterov)} wd={wd} {form}", sweep(run))

    # ---- adamw_step
    for decoupled in (True, False):
        for with_sc in (False, True):
            def run(count, off, put):
                st, ost, sc = state(count, off, ("p", "m", "v")), ops.new_opt_state(DEV), scaler(2) if with_sc else None
                for call in range(3):
                    g = grad(count, off, call, 1.0 if sc is None else float(sc.state[0]), "last" if call == 1 else None)
                    ops.grad_norm_(g, ost, 0.05, 0.5, None if sc is None else sc.state)
                    ops.adamw_step_(st["p"], g, st["m"], st["v"], *HP, 0.01, ost, decoupled, 0.5, sc)
                    for k, t in st.items():
                        put(f"{call}/{k}", t)
                    put(f"{call}/ost", ost)
                    put(f"{call}/scaler", None if sc is None else sc.state)
            emit(f"launch adamw_step decoupled={int(decoupled)} scaler={int(with_sc)}", sweep(run))
    _CACHE.clear()


# ================================================================================================ step
OPTIMS = {"adam": dict(),
          "adamw": dict(optimizer="adamw", optimizer_args=dict(weight_decay=1e-2), clip_grad_norm=0.5),
          "sgd": dict(optimizer="sgd", optimizer_args=dict(momentum=0.99, nesterov=True, weight_decay=3e-5), clip_grad_norm=0.5),
          "skip": dict(skip_nonfinite=True)}


def make_step(which, loss, optim, ncls=3, f_maps=(16, 32), ds=None, graph=None):
    kw = dict(OPTIMS[optim], lr=train.PolyLR(1e-2, 10) if optim == "sgd" else 1e-3, graph=graph)
    ctor = {} if ds is None else dict(deep_supervision=ds)
    if which == "seg":
        net = O.keyed_init_(HM.ResidualUNet3D(1, ncls, False, f_maps=list(f_maps), **ctor)).to(DEV)
        batches = [O.synthetic_batch(2, 1, (16, 16, 16), ncls, 0, seed=900 + i) for i in range(4)]
        step = train.SegmentationStep(net, loss_weight=[0.05] + [1.0] * (ncls - 1), loss=loss, **kw)
    else:
        net = O.keyed_init_(HM.ResidualUNet3D(1, 4, False, f_maps=list(f_maps), **ctor)).to(DEV)
        batches = [O.synthetic_batch(2, 1, (16, 16, 16), 2, 2, seed=900 + i) for i in range(4)]
        step = train.LandmarkStep(net, [0.05, 1.0], [0.015] * 2, "L2", class_loss=loss, **kw)
    batches = [{k: v.to(DEV) for k, v in b.items()} for b in batches]
    if optim == "skip":
        batches[1]["label"][0, -1, 3, 4, 5] = 200  # out of range: a NaN loss, every gradient non-finite, the update skipped
    return step, batches


def step_state(step, out, res, call):
    opt = step.opt
    outs = out if isinstance(out, tuple) else (out,)
    res.update({f"{call}/loss{i}": digest(o) for i, o in enumerate(outs)})
    res.update({f"{call}/scale_loss{i}": digest(o) for i, o in enumerate(getattr(step, "scale_losses", ()))})
    res[f"{call}/p"] = digest(step.flat.flat)
    for k in ("buf", "m", "v", "opt_state"):
        res[f"{call}/{k}"] = digest(getattr(opt, k, None))
    res[f"{call}/scaler"] = digest(None if step.scaler is None else step.scaler.state)
    res[f"{call}/steps_taken"] = opt.steps_taken(step.scaler)
    res[f"{call}/skipped"] = step.skipped_steps()
    try:
        res[f"{call}/grad_norm"] = digest(step.grad_norm)
    except RuntimeError:
        res[f"{call}/grad_norm"] = None


def run_step(mode, which, loss, optim, calls=3, round_trip=False, **kw):
    res = {}
    with mednet_hip.precision(mode):
        step, batches = make_step(which, loss, optim, **kw)
        for call in range(calls):
            if round_trip and call == 2:
                sd, params = step.opt.state_dict(step.scaler), step.flat.flat.clone()
                step.flat.release()
                step, _ = make_step(which, loss, optim, **kw)
                step.flat.flat.copy_(params)
                step.opt.load_state_dict(sd, step.scaler)
            out = step(batches[call])
            torch.cuda.synchronize()
            if not round_trip or call == 2:
                step_state(step, out, res, call)
        step.flat.release()
    torch.cuda.empty_cache()
    return res


def step_family():
    for which in ("seg", "landmark"):
        for loss in ("DICE", "CE", "DICE_CE"):
            for optim in OPTIMS:
                res = {}
                for mode in ("fp32", "bf16", "fp16"):
                    res.update({f"{mode}/{k}": v for k, v in run_step(mode, which, loss, optim).items()})
                emit(f"step {which} {loss} {optim}", res)
    for loss in ("DICE", "CE", "DICE_CE"):
        res = {}
        for mode in ("bf16", "fp16"):
            res.update({f"{mode}/{k}": v for k, v in run_step(mode, "seg", loss, "adam", ncls=6, f_maps=(32, 64)).items()})
        emit(f"step seg {loss} 6 classes on f_maps [32, 64]", res)
        res = {}
        for mode in ("fp32", "bf16", "fp16"):
            res.update({f"{mode}/{k}": v for k, v in run_step(mode, "seg", loss, "adamw", f_maps=(16, 32, 64), ds=1).items()})
        emit(f"step seg {loss} deep_supervision=1 on f_maps [16, 32, 64]", res)
    for which, mode, optim in (("seg", "bf16", "adam"), ("landmark", "bf16", "sgd")):
        emit(f"step {which} {mode} DICE {optim} graph", run_step(mode, which, "DICE", optim, calls=4, graph=True))
    for which, mode, optim in (("seg", "bf16", "adam"), ("seg", "fp16", "adamw"), ("landmark", "fp16", "sgd"), ("landmark", "bf16", "skip")):
        emit(f"step {which} {mode} CE {optim} state_dict round trip", run_step(mode, which, "CE", optim, round_trip=True))


# ================================================================================================ val
def val_family():
    for which in ("seg", "landmark"):
        for loss in ("DICE", "CE", "DICE_CE"):
            res = {}
            for mode in ("bf16", "fp32"):
                with mednet_hip.precision(mode):
                    step, batches = make_step(which, loss, "adam")
                    step(batches[0])  # (one training step first: the parameters are no longer the initial ones)
                    seen = []
                    kw = dict(log_interval=2, on_samples=lambda panels, nb: seen.append((nb, panels.to_host())))
                    if which == "seg":
                        val = train.SegmentationValidation(step.model, loss_weight=[0.05, 1.0, 1.0], loss=loss, **kw)
                    else:
                        val = train.LandmarkValidation(step.model, [0.05, 1.0], [0.015] * 2, class_loss=loss, **kw)
                    outs = [val.validation_step(batches[nb + 1], nb) for nb in range(3)]
                    torch.cuda.synchronize()
                    for nb, o in enumerate(outs):
                        res.update({f"{mode}/{nb}/{k}": digest(v) for k, v in o.items()})
                    end = val.validation_epoch_end(outs)
                    res.update({f"{mode}/end/{k}": digest(v) for k, v in end["log"].items()})
                    res[f"{mode}/end/val_loss"] = digest(end["val_loss"])
                    res[f"{mode}/logged"] = repr([nb for nb, _ in seen])
                    for nb, panels in seen:
                        res.update({f"{mode}/panels{nb}/{k}": digest(v) for k, v in panels.items()})
                    res[f"{mode}/training"] = step.model.training
                    step.flat.release()
                torch.cuda.empty_cache()
            emit(f"val {which} {loss}", res)


print(f"train_digest: package {os.path.dirname(os.path.abspath(mednet_hip.__file__))}, library {L.LIB_PATH}", file=sys.stderr, flush=True)
RUN = {"launch": launch_family, "step": step_family, "val": val_family}
for family in FAMILIES:
    RUN[family]()
