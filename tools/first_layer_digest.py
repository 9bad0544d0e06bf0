"""SHA-256 digests of what the first layer's matrix-core kernels (1-4 input channels, 16-bit storage modes) compute on seeded random
fp32 inputs that are NOT numbers of the storage type: two commits whose kernels run the same arithmetic in the same order print the
same lines.  Only the package's public surface is used, so the tool runs against any commit's package and library:
MC_PKG=<directory that holds that commit's mednet_hip/> MEDNET_LIB_PATH=<its libmednet_hip.so> python tools/first_layer_digest.py
(as tools/multichannel_timing.py); without them it takes this tree's.  One process per package; compare the outputs with diff.

One JSON line per case: its name and ONE SHA-256 over the digests of its tensors (DIGEST_FULL=1 adds the digest of every tensor,
to find which one moved).  form = "plain": hnn.Conv3d(cin, cout, 3, bias=False).forward_with_stats and its backward -> y, the fused
GroupNorm partial rows, dw.  form = "gn": ExtResNetBlock(cin, cout, "cge") forward and backward, whose first weight gradient takes
GroupNorm's backward inside its staging -> the block's output and every parameter gradient ("gn_fused": 1 when that form ran).
Cases: cin 1..4 x {bf16, fp16, fp16x2} x cout {16, 32, 48, 64} x {(9, 11, 21) with n = 2, (40, 72, 80) with n = 3: the persistent
walk and the weight gradient's multi-brick loop}; the input planar and channels-last for cin >= 2, fp32 and in the storage type for
cin = 1.  (cin = 1 with cout = 48: the matrix-core weight gradient does not take it; dw and the gn form are left out.)
Usage: python tools/first_layer_digest.py [forms, default plain,gn] > digest.jsonl"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("MC_PKG") or os.path.join(ROOT, "torch-mednet_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import mednet_hip  # noqa: E402
from mednet_hip import block  # noqa: E402
from mednet_hip import nn as hnn  # noqa: E402
from mednet_hip.unet import components as HC  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402

DEV = "cuda:0"
CL = torch.channels_last_3d
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp16x2": torch.float16}
SHAPES = [(2, (9, 11, 21)), (3, (40, 72, 80))]
FULL = os.environ.get("DIGEST_FULL", "0") == "1"
FORMS = (sys.argv[1] if len(sys.argv) > 1 else "plain,gn").split(",")
_CACHE = {}


def rnd(tag, *shape):
    """Seeded on the CPU by the tag alone; cached, so every case of a shape sees the same tensor."""
    if (tag, shape) not in _CACHE:
        gen = torch.Generator().manual_seed(int.from_bytes(hashlib.sha256(tag.encode()).digest()[:6], "little"))
        _CACHE[(tag, shape)] = torch.randn(*shape, generator=gen, dtype=torch.float32)
    return _CACHE[(tag, shape)]


def digest(t):
    t = t.detach().contiguous().cpu()
    if t.dtype in (torch.bfloat16, torch.float16):
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def inputs(cin, n, shape, mode):
    """(name, tensor on the device) of every form the input arrives in."""
    x = rnd(f"x{cin}", n, cin, *shape)
    if cin == 1:
        return [("fp32", x.to(DEV)), ("x16", x.to(DT[mode]).to(DEV))]
    return [("planar", x.to(DEV)), ("channels_last", x.to(DEV).contiguous(memory_format=CL))]


def plain(mode, cin, cout, n, shape, xname, x):
    conv = hnn.Conv3d(cin, cout, 3, bias=False).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(rnd(f"w{cin}_{cout}", cout, cin, 3, 3, 3) * (27 * cin) ** -0.5)
    y, partial = conv.forward_with_stats(x)
    y.backward(rnd(f"g{cout}", n, cout, *shape).to(DEV).to(DT[mode]))
    torch.cuda.synchronize()
    out = {"y": digest(y), "partial": None if partial is None else digest(partial), "partial_rows": 0 if partial is None else partial.shape[1]}
    if not (cin == 1 and cout == 48):
        out["dw"] = digest(conv.weight.grad)
    return out


def gn(mode, cin, cout, n, shape, xname, x):
    before = block.C1GN_COUNT["fused"]
    net = O.keyed_init_(HC.ExtResNetBlock(cin, cout, order="cge", num_groups=8)).to(DEV)
    y = net(x)
    (y.float() * rnd(f"g{cout}", n, cout, *shape).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    out = {"y": digest(y), "gn_fused": block.C1GN_COUNT["fused"] - before}
    for k, p in net.named_parameters():
        out["d_" + k] = digest(p.grad)
    return out


for form in FORMS:
    for cin in (1, 2, 3, 4):
        for mode in DT:
            for cout in (16, 32, 48, 64):
                if form == "gn" and cin == 1 and cout == 48:
                    continue
                for n, shape in SHAPES:
                    with mednet_hip.precision(mode):
                        for xname, x in inputs(cin, n, shape, mode):
                            res = (plain if form == "plain" else gn)(mode, cin, cout, n, shape, xname, x)
                            line = {"case": f"{form} cin={cin} {mode} cout={cout} n={n} {'x'.join(map(str, shape))} {xname}",
                                    "sha256": hashlib.sha256("".join(f"{k}={v};" for k, v in res.items()).encode()).hexdigest()}
                            if form == "gn":
                                line["gn_fused"] = res["gn_fused"]
                            print(json.dumps({**line, **res} if FULL else line), flush=True)
                    torch.cuda.empty_cache()
