"""Refusal table of csrc/norm_act.hip and of the two Adam entries that lived there (now csrc/optim.hip): every extern "C" entry called with argument sets that trip each of its
MEDNET_REQUIREs in turn -- null pointers, a bad dtype, C % groups != 0, a C with C / vec > 256, a workspace one byte short, two
violations at once (the first check in the entry's order answers).  Every case is refused before any launch, so the tool needs
no device; pointers that only have to be non-null are the address 4096, which nothing reads.  Prints one JSON line per case:
{"entry", "case", "rc", "error"} (error = mednet_last_error()), and for the entries that answer a number instead of a code the
number under "rc" and an empty error.  Two builds whose host code checks the same things in the same order print the same lines:
MEDNET_LIB_PATH=<libmednet_hip.so> python tools/norm_refusals.py > table.jsonl      (one process per library; compare with diff)
tests/test_host_logic.py freezes the table (tests/golden/norm_refusals.jsonl)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("HD_PKG") or os.path.join(ROOT, "torch-mednet_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

from mednet_hip import _lib as L  # noqa: E402

P = 4096  # a non-null pointer nobody dereferences
BAD_DT = 7
BIG = 1 << 40
N, S, C_, G = 2, 720, 32, 8  # a shape every entry takes; (D, H, W) = (12, 10, 6)
D, H, W = 12, 10, 6


def table(lib, options=()):
    """-> list of (entry, case, callable returning rc-or-number, is_refusal).  `options`: the options switched off for this pass;
    what the entries take only while an option is on is refused now, and is called only now."""
    ws = lib.mednet_gn_ws_bytes(N, C_, S)
    rows = []

    def entry(name, base, cases):
        """base: ordered (argument, valid value) pairs; cases: (case name, {argument: value})."""
        keys = [k for k, _ in base]
        fn = getattr(lib, "mednet_" + name)
        for case, over in cases:
            assert set(over) <= set(keys), (name, case)
            args = [over.get(k, v) for k, v in base]
            rows.append((name, case, (lambda fn=fn, args=args: fn(*args)), True))

    def value(name, *args):
        fn = getattr(lib, "mednet_" + name)
        rows.append((name, "value " + " ".join(map(str, args)), (lambda: fn(*args)), False))

    tail = [("ws", P), ("ws_bytes", ws), ("stream", None)]
    shape_cases = [("bad dtype", {"dtype": BAD_DT}),
                   ("C=2056 (C/vec > 256)", {"c": 2056, "ws_bytes": BIG}),
                   ("C=257 (odd, > 256)", {"c": 257, "groups": 1, "ws_bytes": BIG}),
                   ("fp32 C=1028 (no width fits)", {"c": 1028, "groups": 4, "dtype": L.F32, "ws_bytes": BIG}),
                   ("workspace one byte short", {"ws_bytes": ws - 1}),
                   ("workspace empty", {"ws_bytes": 0}),
                   ("fp32 workspace one byte short", {"dtype": L.F32, "ws_bytes": ws - 1}),
                   ("C=1024 workspace one byte short", {"c": 1024, "ws_bytes": lib.mednet_gn_ws_bytes(N, 1024, S) - 1}),
                   ("bad dtype + C % groups", {"dtype": BAD_DT, "c": 36}),
                   ("C/vec > 256 + workspace short", {"c": 2056, "ws_bytes": 1})]
    if "gn_f32_vec4" in options:  # C = 516 in fp32: 129 columns of 4, but neither 8 wide nor <= 256
        shape_cases.append(("fp32 C=516", {"c": 516, "groups": 4, "dtype": L.F32, "ws_bytes": BIG}))
    valid = lambda opt: [("valid arguments", {})] if opt in options else []  # noqa: E731
    no_groups = lambda cases: [(k, {a: b for a, b in v.items() if a != "groups"}) for k, v in cases if "groups" not in k]  # noqa: E731

    for v in ((1, 32, 720), (2, 32, 720), (2, 16, 720), (2, 24, 10080), (3, 12, 720), (2, 512, 720), (2, 1024, 720), (2, 257, 720),
              (1, 2056, 64), (4, 64, 128 ** 3)):
        value("gn_ws_bytes", *v)

    entry("gn_stats", [("x", P), ("gamma", P), ("beta", P), ("stats", P), ("coef", P), ("n", N), ("spatial", S), ("c", C_), ("groups", G),
                       ("eps", 1e-5), ("dtype", L.BF16)] + tail,
          shape_cases + [("n = 0", {"n": 0}), ("c = 0", {"c": 0}), ("groups = 0", {"groups": 0}), ("C % groups", {"c": 36}),
                         ("spatial = 0", {"spatial": 0}), ("C % groups + workspace short", {"c": 36, "ws_bytes": 0})])
    entry("gn_finalize", [("partial", P), ("chunks", 1), ("gamma", P), ("beta", P), ("stats", P), ("coef", P), ("n", N), ("spatial", S),
                          ("c", C_), ("groups", G), ("eps", 1e-5)] + tail,
          [("n = 0", {"n": 0}), ("c = 0", {"c": 0}), ("groups = 0", {"groups": 0}), ("C % groups", {"c": 36}), ("chunks = 0", {"chunks": 0})])
    entry("gn_act_fwd", [("x", P), ("coef", P), ("residual", None), ("z", P), ("n", N), ("spatial", S), ("c", C_), ("act", L.ACT_RELU),
                         ("x_dtype", L.BF16), ("z_dtype", L.BF16), ("stream", None)],
          [("bad x dtype", {"x_dtype": BAD_DT}), ("bad z dtype", {"z_dtype": BAD_DT}), ("x and z differ", {"x_dtype": L.F32}),
           ("C=2056", {"c": 2056}), ("C=257", {"c": 257}), ("fp32 C=1028", {"c": 1028, "x_dtype": L.F32, "z_dtype": L.F32}),
           ("dtypes differ + C=2056", {"z_dtype": L.F16, "c": 2056})] +
          ([("fp32 C=516", {"c": 516, "x_dtype": L.F32, "z_dtype": L.F32})] if "gn_f32_vec4" in options else []))
    bwd = [("dz", P), ("dz2", None), ("x", P), ("z", None), ("coef", P), ("stats", P), ("gamma", P), ("dx", P), ("dres", None),
           ("dgamma", P), ("dbeta", P), ("n", N), ("spatial", S), ("c", C_), ("groups", G), ("act", L.ACT_RELU), ("in_act", L.ACT_NONE),
           ("dtype", L.BF16)] + tail
    entry("gn_act_bwd", bwd,
          shape_cases + [("C % groups", {"c": 36}), ("act without z and coef", {"coef": None}),
                         ("C % groups + act without z and coef", {"c": 36, "coef": None}),
                         ("act without z and coef + workspace short", {"coef": None, "ws_bytes": 0})])
    fused = [("dz", P), ("x", P), ("coef", P), ("stats", P), ("gamma", P), ("fused_partial", P), ("rows", 4), ("dx", P), ("dgamma", P),
             ("dbeta", P), ("n", N), ("spatial", S), ("c", C_), ("groups", G), ("act", L.ACT_RELU), ("in_act", L.ACT_NONE),
             ("dtype", L.BF16)] + tail
    fused_cases = shape_cases + [("C % groups", {"c": 36}), ("rows = 0", {"rows": 0}), ("no fused_partial", {"fused_partial": None}),
                                 ("no coef", {"coef": None}), ("rows = 0 + workspace short", {"rows": 0, "ws_bytes": 0})]
    entry("gn_act_bwd_fused", fused, fused_cases)
    entry("gn_bwd_coefficients", [("stats", P), ("gamma", P), ("fused_partial", P), ("rows", 4), ("bcoef", P), ("dgamma", P), ("dbeta", P),
                                  ("n", N), ("spatial", S), ("c", C_), ("groups", G)] + tail,
          [("C % groups", {"c": 36}), ("rows = 0", {"rows": 0}), ("no fused_partial", {"fused_partial": None}), ("no bcoef", {"bcoef": None}),
           ("no stats", {"stats": None}), ("no gamma", {"gamma": None}), ("all null", {k: None for k in ("stats", "gamma", "fused_partial", "bcoef")}),
           ("workspace one byte short", {"ws_bytes": ws - 1}), ("workspace empty", {"ws_bytes": 0}),
           ("no gamma + workspace short", {"gamma": None, "ws_bytes": 0})])
    res = [("dz", P), ("x", P), ("z", P), ("coef", P), ("stats", P), ("gamma", P), ("fused_partial", P), ("rows", 4), ("dx", P), ("dres", P),
           ("dgamma", P), ("dbeta", P), ("n", N), ("spatial", S), ("c", C_), ("groups", G), ("act", L.ACT_RELU), ("dtype", L.BF16)] + tail
    entry("gn_act_bwd_fused_res", res,
          fused_cases + [("no z", {"z": None}), ("no dres", {"dres": None}), ("no z + bad dtype", {"z": None, "dtype": BAD_DT})])
    entry("gn_act_bwd_fused_res_pool",
          [("dy_pool", P), ("skip_grad", None), ("x", P), ("z", P), ("stats", P), ("gamma", P), ("fused_partial", P), ("rows", 4), ("dx", P),
           ("dres", P), ("dgamma", P), ("dbeta", P), ("n", N), ("d", D), ("h", H), ("w", W), ("c", C_), ("groups", G), ("act", L.ACT_RELU),
           ("pool_mode", L.POOL_MAX), ("dtype", L.BF16)] + tail,
          [("bad dtype", {"dtype": BAD_DT}), ("C % groups", {"c": 36}), ("rows = 0", {"rows": 0}), ("no fused_partial", {"fused_partial": None}),
           ("no dy_pool", {"dy_pool": None}), ("no x", {"x": None}), ("no z", {"z": None}), ("no dx", {"dx": None}), ("no dres", {"dres": None}),
           ("odd depth", {"d": 11}), ("odd height", {"h": 9}), ("odd width", {"w": 7}), ("C % 8", {"c": 12, "groups": 4}),
           ("workspace one byte short", {"ws_bytes": ws - 1}), ("fp32 workspace one byte short", {"dtype": L.F32, "ws_bytes": ws - 1}),
           ("C=2056 workspace short", {"c": 2056, "ws_bytes": ws}), ("bad dtype + no dx", {"dtype": BAD_DT, "dx": None}),
           ("odd width + workspace short", {"w": 7, "ws_bytes": 0})])

    entry("bn_stats", [("x", P), ("gamma", P), ("beta", P), ("running_mean", P), ("running_var", P), ("num_batches_tracked", P),
                       ("momentum", 0.1), ("stats", P), ("coef", P), ("n", N), ("spatial", S), ("c", C_), ("eps", 1e-5),
                       ("dtype", L.BF16)] + tail,
          no_groups(shape_cases) + [("n = 0", {"n": 0}), ("c = 0", {"c": 0}), ("spatial = 0", {"spatial": 0}), ("no x", {"x": None}),
                                    ("no stats", {"stats": None}), ("no coef", {"coef": None}), ("running_mean alone", {"running_var": None}),
                                    ("running_var alone", {"running_mean": None}), ("C=257", {"c": 257, "ws_bytes": BIG}),
                                    ("running_var alone + workspace short", {"running_mean": None, "ws_bytes": 0})])
    entry("bn_eval_coef", [("running_mean", P), ("running_var", P), ("gamma", P), ("beta", P), ("stats", P), ("coef", P), ("n", N), ("c", C_),
                           ("eps", 1e-5), ("stream", None)],
          [("n = 0", {"n": 0}), ("c = 0", {"c": 0}), ("no running_mean", {"running_mean": None}), ("no running_var", {"running_var": None}),
           ("no stats", {"stats": None}), ("no coef", {"coef": None})])
    bn_cases = no_groups(shape_cases) + [("n = 0", {"n": 0}), ("c = 0", {"c": 0}), ("spatial = 0", {"spatial": 0}), ("no dz", {"dz": None}),
                                         ("no x", {"x": None}), ("no coef", {"coef": None}), ("no stats", {"stats": None}), ("no dx", {"dx": None}),
                                         ("C=257", {"c": 257, "ws_bytes": BIG}), ("no dx + workspace short", {"dx": None, "ws_bytes": 0})]
    entry("bn_act_bwd", [("dz", P), ("x", P), ("z", None), ("coef", P), ("stats", P), ("gamma", P), ("dx", P), ("dres", None), ("dgamma", P),
                         ("dbeta", P), ("n", N), ("spatial", S), ("c", C_), ("act", L.ACT_RELU), ("in_act", L.ACT_NONE), ("frozen", 0),
                         ("dtype", L.BF16)] + tail, bn_cases)
    entry("bn_act_bwd_fused", [("dz", P), ("x", P), ("coef", P), ("stats", P), ("gamma", P), ("fused_partial", P), ("rows", 4), ("dx", P),
                               ("dgamma", P), ("dbeta", P), ("n", N), ("spatial", S), ("c", C_), ("act", L.ACT_RELU), ("in_act", L.ACT_NONE),
                               ("frozen", 0), ("dtype", L.BF16)] + tail,
          bn_cases + [("rows = 0", {"rows": 0}), ("no fused_partial", {"fused_partial": None})])

    entry("act_fwd", [("x", P), ("z", P), ("count", 64), ("act", L.ACT_RELU), ("dtype", L.BF16), ("stream", None)], [("bad dtype", {"dtype": BAD_DT})])
    entry("act_bwd", [("dz", P), ("z", P), ("dx", P), ("count", 64), ("act", L.ACT_RELU), ("dtype", L.BF16), ("stream", None)],
          [("bad dtype", {"dtype": BAD_DT})])
    entry("add", [("a", P), ("b", P), ("out", P), ("count", 64), ("dtype", L.BF16), ("stream", None)], [("bad dtype", {"dtype": -1})])
    dims = [("n", N), ("d", D), ("h", H), ("w", W), ("c", C_)]
    entry("pool2_fwd", [("x", P), ("y", P)] + dims + [("mode", L.POOL_MAX), ("dtype", L.BF16), ("stream", None)],
          [("bad dtype", {"dtype": BAD_DT}), ("depth 1", {"d": 1}), ("height 1", {"h": 1}), ("width 1", {"w": 1}),
           ("bad dtype + depth 1", {"dtype": BAD_DT, "d": 1})])
    for v in ((12, 10, 6, 32, L.BF16), (12, 10, 6, 32, L.F32), (12, 10, 7, 32, L.BF16), (12, 10, 6, 12, L.F16), (12, 10, 6, 32, BAD_DT),
              (1, 10, 6, 32, L.BF16)):
        value("gn_act_pool_supported", *v)
    entry("gn_act_pool_fwd", [("x", P), ("coef", P), ("residual", None), ("z", P), ("pooled", P)] + dims +
          [("act", L.ACT_RELU), ("mode", L.POOL_MAX), ("dtype", L.BF16), ("stream", None)],
          [("bad dtype", {"dtype": BAD_DT}), ("odd width", {"w": 7}), ("C % 8", {"c": 12}), ("n = 0", {"n": 0}), ("no x", {"x": None}),
           ("no coef", {"coef": None}), ("no z", {"z": None}), ("no pooled", {"pooled": None}), ("odd width + no z", {"w": 7, "z": None})] + valid("gn_pool_fuse"))
    entry("pool2_bwd_act", [("dy", P), ("x", P), ("add", P), ("add_channels", 0), ("dx", P)] + dims +
          [("mode", L.POOL_MAX), ("in_act", L.ACT_NONE), ("dtype", L.BF16), ("stream", None)],
          [("bad dtype", {"dtype": BAD_DT}), ("strided add without add", {"add": None, "add_channels": 64}),
           ("strided add narrower than C", {"add_channels": 16}), ("strided add % 8", {"add_channels": 36}),
           ("strided add, C % 8", {"c": 12, "add_channels": 16}), ("strided add, odd extent", {"add_channels": 64, "w": 7}),
           ("in_act with an odd extent", {"in_act": L.ACT_RELU, "h": 9}), ("bad dtype + strided add % 8", {"dtype": BAD_DT, "add_channels": 36}),
           ("strided add, odd extent + in_act", {"add_channels": 64, "w": 7, "in_act": L.ACT_RELU})])
    entry("pool2_bwd", [("dy", P), ("x", P), ("add", None), ("dx", P)] + dims + [("mode", L.POOL_MAX), ("dtype", L.BF16), ("stream", None)],
          [("bad dtype", {"dtype": BAD_DT})])
    for v in ((2, 12, 10, 6, 32, L.BF16), (2, 12, 10, 6, 32, L.F32), (2, 12, 10, 7, 32, L.BF16), (2, 12, 10, 6, 24, L.BF16),
              (2, 12, 10, 6, 1024, L.BF16), (2, 128, 128, 128, 64, L.BF16), (2, 12, 10, 6, 32, BAD_DT)):
        value("pool2_bwd_gn_rows", *v)
    entry("pool2_bwd_gn", [("dy", P), ("x", P), ("add", None), ("dx", P), ("gn_y", P), ("gn_act", L.ACT_RELU), ("gn_partial", P)] + dims +
          [("mode", L.POOL_MAX), ("dtype", L.BF16), ("stream", None)],
          [("bad dtype", {"dtype": BAD_DT}), ("odd width", {"w": 7}), ("C / 8 no power of two", {"c": 24}), ("C = 1024", {"c": 1024}),
           ("no gn_y", {"gn_y": None}), ("no gn_partial", {"gn_partial": None}), ("odd width + no gn_y", {"w": 7, "gn_y": None})] + valid("gn3_fuse"))
    up = [("n", N), ("d", D), ("h", H), ("w", W), ("c_enc", 16), ("xd", D // 2), ("xh", H // 2), ("xw", W // 2), ("c_x", 32), ("dtype", L.BF16),
          ("stream", None)]
    entry("upcat_fwd", [("enc", P), ("x", P), ("out", P)] + up, [("bad dtype", {"dtype": BAD_DT})])
    for v in ((2, 12, 10, 6, 16, 32, L.BF16), (2, 12, 10, 6, 16, 32, L.F32), (2, 24, 20, 21, 16, 32, L.F16), (2, 12, 10, 6, 12, 32, L.BF16),
              (2, 12, 10, 6, 16, 36, L.BF16), (2, 12, 10, 6, 1024, 1032, L.BF16), (2, 12, 10, 6, 16, 32, BAD_DT), (2, 128, 128, 128, 64, 128, L.BF16)):
        value("upcat_stats_chunks", *v)
    entry("upcat_fwd_stats", [("enc", P), ("x", P), ("out", P), ("partial", P)] + up,
          [("bad dtype", {"dtype": BAD_DT}), ("c_enc % 8", {"c_enc": 12}), ("c_x % 8", {"c_x": 36}), ("too many channels", {"c_enc": 1024, "c_x": 1032}),
           ("no partial", {"partial": None}), ("bad dtype + no partial", {"dtype": BAD_DT, "partial": None})] + valid("upcat_stats"))
    entry("upcat_bwd", [("dout", P), ("denc", P), ("dx", P)] + up, [("bad dtype", {"dtype": BAD_DT})])
    entry("adam_step_scaled", [("p", P), ("g", P), ("m", P), ("v", P), ("count", 64), ("lr", 1e-3), ("beta1", 0.9), ("beta2", 0.999), ("eps", 1e-8),
                               ("weight_decay", 0.0), ("inv_world", 1.0), ("scaler_state", P), ("growth_factor", 2.0), ("backoff_factor", 0.5),
                               ("growth_interval", 2000), ("stream", None)],
          [("no scaler state", {"scaler_state": None}), ("growth_interval = 0", {"growth_interval": 0})])
    entry("adam_step", [("p", P), ("g", P), ("m", P), ("v", P), ("count", 64), ("lr", 1e-3), ("beta1", 0.9), ("beta2", 0.999), ("eps", 1e-8),
                        ("weight_decay", 0.0), ("step", 1), ("grad_scale", 1.0), ("stream", None)], [("step = 0", {"step": 0})])
    return rows


def run(lib):
    """-> the table as a list of dicts, in a fixed order; once more for the entries whose answer an option changes."""
    out = []
    for options, only in (({}, None), ({"gn_f32_vec4": 0}, ("gn_ws_bytes", "gn_stats", "gn_act_fwd", "gn_act_bwd", "bn_act_bwd")),
                          ({"gn_pool_fuse": 0, "gn3_fuse": 0, "upcat_stats": 0},
                           ("gn_act_pool_supported", "gn_act_pool_fwd", "pool2_bwd_gn_rows", "pool2_bwd_gn", "upcat_stats_chunks", "upcat_fwd_stats"))):
        before = {k: lib.mednet_get_option(k.encode(), 1) for k in options}
        for k, v in options.items():
            lib.mednet_set_option(k.encode(), v)
        tag = "".join(f" [{k}={v}]" for k, v in options.items())
        try:
            for name, case, call, refusal in table(lib, tuple(options)):
                if only is not None and name not in only:
                    continue
                rc = call()
                out.append({"entry": "mednet_" + name, "case": case + tag, "rc": rc,
                            "error": lib.mednet_last_error().decode(errors="replace") if refusal else ""})
        finally:
            for k, v in before.items():
                lib.mednet_set_option(k.encode(), v)
    return out


if __name__ == "__main__":
    for line in run(L.lib()):
        print(json.dumps(line))
