"""Routes of the convolution family without a device, in two parts, one JSON line per case:

(a) the refusal table of every conv-family extern "C" entry of csrc/api.hip: argument sets that trip each check in turn (bad
    dtype, ksize = 2, a zero extent, null gn_* pointers, negative `workgroups`, a workspace one byte short for the bias gradient or
    empty for the partial sums, MEDNET_ALGO_MFMA on shapes the matrix-core path does not take, an activation out of range, two
    violations at once) and valid arguments with conv_fuse_gnb, gn3_fuse, conv_cm or conv_fuse_stats switched off where that makes
    the entry refuse.  {"entry", "case", "rc", "error"}; every case is refused before any launch (run() asserts a negative code
    other than MEDNET_E_HIP), pointers that only have to be non-null are the address 4096.
(b) the answers of every entry that returns a number, one line per grid point with every entry's answer there:
    {"case": "point <volume> <cin>-><cout> dtype=<d> algo=<a>", "answers": {...}} over five volumes x nine channel pairs, two of
    the fifteen (storage type, algo) pairs at each, walking through all fifteen (the full product was 5000 lines); and
    {"case": "plan <volume> <cin>-><cout> dtype=<d>", "answers": {...}} with the launch plans (gnb bit and split bit x stride) and
    the weight-gradient plans of the channel pairs the 16-bit matrix-core kernels take.  Once more at 2 x 32^3 with the options off.

Everything runs with assume_cus = 256 (the plans of the one-workgroup-per-CU kernels need a CU count).  Which volume yields which
plan:
  mednet_conv3d_stats_plan kind 2 (general kernel, a row per wave and brick): every volume, (2, 3, 5, 7) -- below one brick -- among them;
    kind 3 (general kernel, accumulating): 32 -> 64 at (1, 64, 64, 64);
    kind 4 (conv32_mfma_kernel): 32 -> 32 at (1, 64, 64, 64);
    kind 5 (conv2b_mfma_kernel, a row per wave and brick): split weights at (1, 9, 17, 20), odd, 18 bricks;
    kind 6 (conv2b_mfma_kernel, accumulating): 64 -> 64 and 128 -> 64 at (1, 64, 64, 64), split weights at (2, 32, 32, 32);
    kind 7 (convt_dgrad32_mfma_kernel): stride 2, ConvTranspose3d 64 -> 32, at (2, 32, 32, 8) -- narrow --, (2, 32, 32, 32) and
    (1, 64, 64, 64).
  mednet_conv3d_wgrad_plan kind 4 (wgrad_mfma4_kernel): (1, 9, 17, 20), (2, 32, 32, 32), (1, 64, 64, 64); kind 2
    (wgrad_mfma2_kernel): (2, 3, 5, 7), (2, 32, 32, 8).
Two builds whose host code decides the same things in the same order print the same lines:
MEDNET_LIB_PATH=<libmednet_hip.so> python tools/conv_routes.py > table.jsonl      (one process per library; compare with diff)
tests/test_host_logic.py freezes the table (tests/golden/conv_routes.jsonl)."""
import ctypes
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
E_HIP = -4
N, D, H, W = 2, 12, 10, 6
VOLUMES = ((2, 3, 5, 7), (1, 9, 17, 20), (2, 32, 32, 8), (2, 32, 32, 32), (1, 64, 64, 64))
CHANNELS = ((1, 32), (3, 32), (16, 16), (32, 32), (32, 64), (64, 64), (64, 32), (128, 64), (24, 24))
DTYPES = (L.F32, L.BF16, L.F16)
ALGOS = (L.ALGO_AUTO, L.ALGO_MFMA, L.ALGO_DIRECT, L.ALGO_EXACT, L.ALGO_AUTO | L.ALGO_SPLITW_BIT)


def refusals(lib, options=()):
    """-> list of (entry, case, callable returning rc).  `options`: the options switched off for this pass; what the entries take
    only while an option is on is refused now, and is called only now."""
    rows = []

    def entry(name, base, cases):
        """base: ordered (argument, valid value) pairs; cases: (case name, {argument: value})."""
        keys = [k for k, _ in base]
        fn = getattr(lib, "mednet_" + name)
        for case, over in cases:
            assert set(over) <= set(keys), (name, case)
            args = [over.get(k, v) for k, v in base]
            rows.append((name, case, (lambda fn=fn, args=args: fn(*args))))

    valid = lambda opt, over=None, tag="": [("valid arguments" + tag, over or {})] if opt in options else []  # noqa: E731
    dims = [("n", N), ("d", D), ("h", H), ("w", W), ("cin", 32), ("cout", 32)]
    shape = [("zero depth", {"d": 0}), ("zero width", {"w": 0}), ("n = 0", {"n": 0}), ("cin = 0", {"cin": 0})]

    entry("conv3d_pack_elt", [("w", P), ("packed", P), ("cin", 32), ("cout", 32), ("ksize", 3), ("transposed_src", 0), ("elt_dtype", L.BF16),
                              ("stream", None)],
          [("bad dtype", {"elt_dtype": BAD_DT}), ("ksize = 2", {"ksize": 2}), ("cin = 0", {"cin": 0}), ("pack not 16-byte aligned", {"packed": P + 4}),
           ("bad dtype + ksize = 2", {"elt_dtype": BAD_DT, "ksize": 2})])
    entry("conv3d_pack_table", [("jobs", None), ("njobs", 1), ("table_host", P), ("max_blocks", P)], [("no jobs", {})])
    entry("conv3d_pack_many", [("table", P), ("njobs", 1), ("max_blocks", 8), ("elt_dtype", L.BF16), ("stream", None)],
          [("bad dtype", {"elt_dtype": BAD_DT}), ("high only for fp32", {"elt_dtype": L.F32 | L.PACK_HIGH_ONLY}), ("no table", {"table": None}),
           ("njobs = 0", {"njobs": 0}), ("max_blocks = 0", {"max_blocks": 0})])
    out = (ctypes.c_int * 16)()
    entry("conv3d_stats_plan", dims + [("dtype", L.BF16), ("gnb", 0), ("stride", 1), ("out", out)],
          [("no out", {"out": None}), ("stride = 3", {"stride": 3}), ("zero depth", {"d": 0}), ("fp32", {"dtype": L.F32}), ("cin = 24", {"cin": 24}),
           ("stride = 3 + fp32", {"stride": 3, "dtype": L.F32})])
    entry("conv3d_wgrad_plan", dims + [("dtype", L.BF16), ("workgroups", 0), ("out", out)],
          [("no out", {"out": None}), ("workgroups = -1", {"workgroups": -1}), ("zero depth", {"d": 0}), ("fp32", {"dtype": L.F32}),
           ("cout = 24", {"cout": 24})])
    entry("conv3d_wgrad_cm_plan", dims + [("dtype", L.BF16), ("gn", 0), ("out", out)],
          [("no out", {"cin": 3, "out": None}), ("zero depth", {"cin": 3, "d": 0}), ("cin = 32", {}), ("cin = 5", {"cin": 5}),
           ("fp32", {"cin": 3, "dtype": L.F32}), ("cout = 24", {"cin": 3, "cout": 24})])

    fwd = [("x", P), ("packed", P), ("bias", None), ("y", P)] + dims + [("ksize", 3), ("x_dtype", L.BF16), ("x_layout", L.NDHWC),
                                                                       ("y_dtype", L.BF16), ("y_layout", L.NDHWC), ("dgrad", 0),
                                                                       ("algo", L.ALGO_AUTO), ("gn_partial", None), ("stream", None)]
    mfma = {"algo": L.ALGO_MFMA}
    entry("conv3d_fwd", fwd,
          [("bad x dtype", {"x_dtype": BAD_DT}), ("bad y dtype", {"y_dtype": BAD_DT}), ("ksize = 2", {"ksize": 2})] + shape +
          [("bad dtype + ksize = 2", {"x_dtype": BAD_DT, "ksize": 2}), ("ksize = 2 + zero depth", {"ksize": 2, "d": 0}),
           ("MFMA, cin = 24", dict(mfma, cin=24)), ("MFMA, cout = 24", dict(mfma, cout=24)), ("MFMA with a bias", dict(mfma, bias=P)),
           ("MFMA, planar y", dict(mfma, y_layout=L.NCDHW)), ("MFMA, ksize = 1", dict(mfma, ksize=1)),
           ("MFMA, bf16 -> fp16", dict(mfma, y_dtype=L.F16)), ("MFMA, data gradient, planar x", dict(mfma, dgrad=1, x_layout=L.NCDHW)),
           ("MFMA + exact, fp32 -> bf16", {"algo": L.ALGO_MFMA | L.ALGO_EXACT_BIT, "x_dtype": L.F32, "cin": 24}),
           ("MFMA, ksize = 1, fp32", dict(mfma, ksize=1, x_dtype=L.F32, y_dtype=L.F32)),
           ("partials, DIRECT", {"algo": L.ALGO_DIRECT, "gn_partial": P}), ("partials, cin = 24", {"cin": 24, "gn_partial": P}),
           ("partials, fp32 exact", {"algo": L.ALGO_EXACT, "x_dtype": L.F32, "y_dtype": L.F32, "gn_partial": P}),
           ("partials, fp32 cin = 24", {"cin": 24, "x_dtype": L.F32, "y_dtype": L.F32, "gn_partial": P}),
           ("partials, ksize = 1", {"ksize": 1, "gn_partial": P}), ("partials, DIRECT + zero depth", {"algo": L.ALGO_DIRECT, "gn_partial": P, "d": 0})] +
          valid("conv_cm", dict(mfma, cin=3, x_dtype=L.F32), ", MFMA, 3 -> 32") +
          valid("conv_cm", {"cin": 3, "x_dtype": L.F32, "gn_partial": P}, ", partials, 3 -> 32"))
    entry("conv3d_act_fwd", [("x", P), ("packed", P), ("y", P)] + dims + [("act", L.ACT_RELU), ("algo", L.ALGO_AUTO), ("gn_partial", None),
                                                                         ("dtype", L.BF16), ("stream", None)],
          [("bad dtype", {"dtype": BAD_DT}), ("fp32", {"dtype": L.F32})] + shape +
          [("activation 4", {"act": 4}), ("activation -1", {"act": -1}), ("DIRECT", {"algo": L.ALGO_DIRECT}), ("cin = 24", {"cin": 24}),
           ("cout = 8", {"cout": 8}), ("fp32 + activation 4", {"dtype": L.F32, "act": 4}), ("activation 4 + cin = 24", {"act": 4, "cin": 24}),
           ("zero depth + activation 4", {"d": 0, "act": 4})])
    f32 = {"dtype": L.F32}
    entry("conv3d_dgrad_add", [("dy", P), ("packed", P), ("add", P), ("dx", P)] + dims + [("algo", L.ALGO_AUTO), ("dtype", L.BF16), ("stream", None)],
          [("bad dtype", {"dtype": BAD_DT})] + shape + [("fp32, " + k, dict(f32, **v)) for k, v in shape] +
          [("DIRECT", {"algo": L.ALGO_DIRECT}), ("cin = 24", {"cin": 24}), ("cout = 24", {"cout": 24}), ("fp32, DIRECT", dict(f32, algo=L.ALGO_DIRECT)),
           ("fp32, exact", dict(f32, algo=L.ALGO_EXACT)), ("fp32, MFMA + exact", dict(f32, algo=L.ALGO_MFMA | L.ALGO_EXACT_BIT)),
           ("fp32, cin = 24", dict(f32, cin=24)), ("fp32, cout = 3", dict(f32, cout=3)), ("bad dtype + zero depth", {"dtype": BAD_DT, "d": 0}),
           ("zero depth + DIRECT", {"d": 0, "algo": L.ALGO_DIRECT}), ("fp32, zero depth + DIRECT", dict(f32, d=0, algo=L.ALGO_DIRECT))])
    gn_cases = [("bad dtype", {"dtype": BAD_DT})] + shape + [("fp32, " + k, dict(f32, **v)) for k, v in shape]
    for pre, base in (("", {}), ("fp32, ", f32)):
        gn_cases += [(pre + "no gn_y", dict(base, gn_y=None)), (pre + "no gn_coef", dict(base, gn_coef=None)),
                     (pre + "no gn_partial", dict(base, gn_partial=None)), (pre + "activation 4", dict(base, gn_act=4)),
                     (pre + "activation -1", dict(base, gn_act=-1)), (pre + "DIRECT", dict(base, algo=L.ALGO_DIRECT)),
                     (pre + "cin = 24", dict(base, cin=24)), (pre + "zero depth + no gn_y", dict(base, d=0, gn_y=None)),
                     (pre + "no gn_y + activation 4", dict(base, gn_y=None, gn_act=4)),
                     (pre + "activation 4 + DIRECT", dict(base, gn_act=4, algo=L.ALGO_DIRECT))]
    gn_cases += [("fp32, exact", dict(f32, algo=L.ALGO_EXACT)), ("bad dtype + no gn_y", {"dtype": BAD_DT, "gn_y": None})]
    entry("conv3d_dgrad_gn", [("dy", P), ("packed", P), ("add", None), ("dx", P), ("gn_y", P), ("gn_coef", P), ("gn_act", L.ACT_RELU),
                              ("gn_partial", P)] + dims + [("algo", L.ALGO_AUTO), ("dtype", L.BF16), ("stream", None)],
          gn_cases + valid("conv_fuse_gnb") + valid("conv_fuse_gnb", f32, ", fp32") + valid("conv_fuse_gnb", {"add": P, "dtype": L.F16}, ", fp16 with add"))
    entry("head_dgrad_gn", [("dy", P), ("packed", P), ("dx", P), ("gn_y", P), ("gn_z", P), ("gn_act", L.ACT_RELU), ("gn_partial", P)] + dims +
          [("dtype", L.BF16), ("stream", None)],
          shape + [("no dy", {"dy": None}), ("no gn_y", {"gn_y": None}), ("no gn_z", {"gn_z": None}), ("no gn_partial", {"gn_partial": None}),
                   ("cin = 24", {"cin": 24}), ("cin = 128", {"cin": 128}), ("bad dtype", {"dtype": BAD_DT}), ("no gn_z + cin = 24", {"gn_z": None, "cin": 24})] +
          valid("gn3_fuse"))

    ct = [("n", N), ("d", D), ("h", H), ("w", W), ("cin", 64), ("cout", 32)]
    ct_mfma = [("MFMA, cin = 16", dict(mfma, cin=16)), ("MFMA, cout = 48", dict(mfma, cout=48))]
    entry("convt3d_fwd", [("x", P), ("packed", P), ("bias", None), ("skip", None), ("y", P)] + ct +
          [("x_dtype", L.BF16), ("y_dtype", L.BF16), ("algo", L.ALGO_AUTO), ("stream", None)],
          [("bad x dtype", {"x_dtype": BAD_DT}), ("bad y dtype", {"y_dtype": BAD_DT})] + shape + ct_mfma +
          [("MFMA, bf16 -> fp16", dict(mfma, y_dtype=L.F16)), ("MFMA, fp32 -> bf16", dict(mfma, x_dtype=L.F32)),
           ("bad dtype + MFMA, cin = 16", dict(mfma, cin=16, x_dtype=BAD_DT))])
    entry("convt3d_dgrad", [("dy", P), ("packed", P), ("dx", P)] + ct + [("dy_dtype", L.BF16), ("dx_dtype", L.BF16), ("algo", L.ALGO_AUTO), ("stream", None)],
          [("bad dy dtype", {"dy_dtype": BAD_DT}), ("bad dx dtype", {"dx_dtype": BAD_DT})] + shape + ct_mfma +
          [("MFMA, bf16 -> fp16", dict(mfma, dx_dtype=L.F16)), ("MFMA, fp32 -> bf16", dict(mfma, dy_dtype=L.F32)),
           ("zero depth + MFMA, cin = 16", dict(mfma, cin=16, d=0))])
    entry("convt3d_dgrad_gn", [("dy", P), ("packed", P), ("dx", P), ("gn_y", P), ("gn_z", P), ("gn_act", L.ACT_RELU), ("gn_partial", P)] + ct +
          [("dtype", L.BF16), ("algo", L.ALGO_AUTO), ("stream", None)],
          [("bad dtype", {"dtype": BAD_DT})] + shape +
          [("no gn_y", {"gn_y": None}), ("no gn_z", {"gn_z": None}), ("no gn_partial", {"gn_partial": None}), ("DIRECT", {"algo": L.ALGO_DIRECT}),
           ("cin = 16", {"cin": 16}), ("cout = 48", {"cout": 48}), ("fp32", f32), ("zero depth + no gn_y", {"d": 0, "gn_y": None}),
           ("no gn_z + DIRECT", {"gn_z": None, "algo": L.ALGO_DIRECT})] + valid("gn3_fuse"))

    # bytes of the bias gradient's partial rows (channel_sum_ws_bytes of csrc/conv_direct.hip for 32 channels-last channels: one
    # chunk of 65536 / 32 voxels each) -- the entries refuse a workspace one byte short of them and take one that holds them
    bias_need = lambda spatial: N * ((spatial + 2047) // 2048) * 32 * 4 + 256  # noqa: E731
    short, short_t = bias_need(D * H * W) - 1, bias_need(8 * D * H * W) - 1
    wg =[("x", P), ("dy", P), ("dw", P), ("dbias", None)] + dims + [("ksize", 3), ("x_dtype", L.BF16), ("x_layout", L.NDHWC), ("dy_dtype", L.BF16),
                                                                     ("dy_layout", L.NDHWC), ("algo", L.ALGO_AUTO), ("workgroups", 0), ("ws", P),
                                                                     ("ws_bytes", BIG), ("stream", None)]
    entry("conv3d_wgrad", wg,
          [("workgroups = -1", {"workgroups": -1}), ("bad x dtype", {"x_dtype": BAD_DT}), ("bad dy dtype", {"dy_dtype": BAD_DT}), ("ksize = 2", {"ksize": 2})] +
          shape + [("bias gradient, workspace one byte short", {"dbias": P, "ws_bytes": short}), ("bias gradient, no workspace", {"dbias": P, "ws_bytes": 0}),
                   ("fp32 bias gradient, workspace one byte short", {"dbias": P, "ws_bytes": short, "x_dtype": L.F32, "dy_dtype": L.F32}),
                   ("MFMA, cin = 24", dict(mfma, cin=24)), ("MFMA, cout = 24", dict(mfma, cout=24)), ("MFMA, fp32 x", dict(mfma, x_dtype=L.F32)),
                   ("MFMA, planar dy", dict(mfma, dy_layout=L.NCDHW)), ("MFMA, bf16 x fp16 dy", dict(mfma, dy_dtype=L.F16)),
                   ("no workspace", {"ws_bytes": 0}), ("fp16, no workspace", {"ws_bytes": 0, "x_dtype": L.F16, "dy_dtype": L.F16}),
                   ("no workspace, 32^3", {"ws_bytes": 0, "d": 32, "h": 32, "w": 32}),
                   ("workgroups = -1 + bad dtype", {"workgroups": -1, "x_dtype": BAD_DT}), ("ksize = 2 + bias gradient, no workspace",
                                                                                           {"ksize": 2, "dbias": P, "ws_bytes": 0}),
                   ("bias gradient, workspace 1 byte + MFMA, cin = 24", dict(mfma, cin=24, dbias=P, ws_bytes=1))])
    entry("convt3d_wgrad", [("x", P), ("dy", P), ("dw", P), ("dbias", None)] + ct +
          [("x_dtype", L.BF16), ("dy_dtype", L.BF16), ("algo", L.ALGO_AUTO), ("workgroups", 0), ("ws", P), ("ws_bytes", BIG), ("stream", None)],
          [("workgroups = -1", {"workgroups": -1}), ("bad x dtype", {"x_dtype": BAD_DT}), ("bad dy dtype", {"dy_dtype": BAD_DT})] + shape +
          [("bias gradient, workspace one byte short", {"dbias": P, "ws_bytes": short_t}), ("bias gradient, no workspace", {"dbias": P, "ws_bytes": 0}),
           ("fp32 bias gradient, workspace one byte short", {"dbias": P, "ws_bytes": short_t, "x_dtype": L.F32, "dy_dtype": L.F32})] + ct_mfma +
          [("MFMA, bf16 x fp16 dy", dict(mfma, dy_dtype=L.F16)), ("no workspace", {"ws_bytes": 0}),
           ("workgroups = -1 + zero depth", {"workgroups": -1, "d": 0}), ("bias gradient, workspace 1 byte + MFMA, cin = 16", dict(mfma, cin=16, dbias=P, ws_bytes=1))])
    entry("conv3d_wgrad_c1_gn", [("x", P), ("dz", P), ("y", P), ("coef", P), ("bcoef", P), ("dw", P), ("n", N), ("d", D), ("h", H), ("w", W),
                                 ("cout", 32), ("act", L.ACT_RELU), ("x_dtype", L.F32), ("dtype", L.BF16), ("ws", P), ("ws_bytes", BIG), ("stream", None)],
          [("no x", {"x": None}), ("no bcoef", {"bcoef": None}), ("no ws", {"ws": None}), ("fp32 dz", {"dtype": L.F32}), ("bad x dtype", {"x_dtype": BAD_DT}),
           ("zero depth", {"d": 0}), ("cout = 0", {"cout": 0}), ("cout = 24", {"cout": 24}), ("no workspace", {"ws_bytes": 0}),
           ("no x + fp32 dz", {"x": None, "dtype": L.F32})])
    entry("conv3d_wgrad_cm_gn", [("x", P), ("x_layout", L.NCDHW), ("dz", P), ("y", P), ("coef", P), ("bcoef", P), ("dw", P), ("n", N), ("d", D),
                                 ("h", H), ("w", W), ("cin", 3), ("cout", 32), ("act", L.ACT_RELU), ("x_dtype", L.F32), ("dtype", L.BF16), ("ws", P),
                                 ("ws_bytes", BIG), ("stream", None)],
          [("no dz", {"dz": None}), ("no ws", {"ws": None}), ("bf16 x", {"x_dtype": L.BF16}), ("fp32 dz", {"dtype": L.F32}), ("x_layout = 2", {"x_layout": 2}),
           ("zero depth", {"d": 0}), ("cin = 5", {"cin": 5}), ("cin = 1", {"cin": 1}), ("cout = 24", {"cout": 24}), ("no workspace", {"ws_bytes": 0}),
           ("bf16 x + x_layout = 2", {"x_dtype": L.BF16, "x_layout": 2})])
    return rows


def values(lib):
    """-> list of (case, callable returning {entry and arguments that vary: answer}).  One case per grid point, holding every entry's answer
    there: "point" cases (a volume, a channel pair, a storage type, an algo) and "plan" cases (a volume, a channel pair the 16-bit
    matrix-core kernels take: the launch plans, gnb bit / split bit x stride, and the weight-gradient plans)."""
    rows = []

    def plan(name, count, *args):
        out = (ctypes.c_int * count)()
        rc = getattr(lib, "mednet_" + name)(*args, out)
        return list(out) if rc == 0 else rc

    def point(n, d, h, w, cin, cout, dt, algo):
        x_dt = L.F32 if cin < 16 else dt  # (the first layer reads the fp32 input volume)
        v = (n, d, h, w)
        return {"pack_bytes k=1,3": [lib.mednet_conv3d_pack_bytes(cin, cout, k) for k in (1, 3)],
                "cm_supported": lib.mednet_conv3d_cm_supported(cin, cout, 3, L.F32, dt, algo),
                "head_dgrad_gn_rows": lib.mednet_head_dgrad_gn_rows(*v, cin, dt),
                "wgrad_ws_bytes (k, workgroups)=(1,0),(3,0),(3,128)": [lib.mednet_conv3d_wgrad_ws_bytes(*v, cin, cout, k, g)
                                                                      for k, g in ((1, 0), (3, 0), (3, 128))],
                "convt_wgrad_ws_bytes workgroups=0,128": [lib.mednet_convt3d_wgrad_ws_bytes(*v, cin, cout, g) for g in (0, 128)],
                "wgrad_cm_plan gn=0,1": [plan("conv3d_wgrad_cm_plan", 4, *v, cin, cout, dt, gn) for gn in (0, 1)] if cin < 16 else None,
                "act_supported": lib.mednet_conv3d_act_supported(*v, cin, cout, algo),
                "dgrad_gn_rows": lib.mednet_conv3d_dgrad_gn_rows(*v, cin, cout, algo),
                "fused_stats_chunks": lib.mednet_conv3d_fused_stats_chunks(*v, cin, cout, 3, x_dt, dt, algo),
                "wgrad_coresident": lib.mednet_conv3d_wgrad_coresident(*v, cin, cout, 3, x_dt, dt, algo),
                "dgrad_add_supported": lib.mednet_conv3d_dgrad_add_supported(*v, cin, cout, algo, dt),
                "dgrad_gn_rows_dt": lib.mednet_conv3d_dgrad_gn_rows_dt(*v, cin, cout, algo, dt),
                "convt_dgrad_gn_rows": lib.mednet_convt3d_dgrad_gn_rows(*v, cin, cout, dt, algo)}

    def plans(n, d, h, w, cin, cout, dt):
        return {"stats_plan (gnb, stride)=(0,1),(0,2),(1,1),(1,2),(2,1),(2,2),(3,1),(3,2)":
                [plan("conv3d_stats_plan", 13, n, d, h, w, cin, cout, dt, gnb, stride) for gnb in (0, 1, 2, 3) for stride in (1, 2)],
                "wgrad_plan workgroups=0,128": [plan("conv3d_wgrad_plan", 10, n, d, h, w, cin, cout, dt, g) for g in (0, 128)]}

    seen = set()
    for i, vol in enumerate(VOLUMES):
        for j, (cin, cout) in enumerate(CHANNELS):
            # two of the fifteen (storage type, algo) pairs per (volume, channel pair), walking through all of them
            for k in (2 * (i * len(CHANNELS) + j), 2 * (i * len(CHANNELS) + j) + 1):
                dt, algo = DTYPES[k % 3], ALGOS[k % 5]
                seen.add((dt, algo))
                rows.append((f"point {vol} {cin}->{cout} dtype={dt} algo={algo}", (lambda a=(*vol, cin, cout, dt, algo): point(*a))))
            if cin % 16 == 0 and cout % 16 == 0:
                dt = (L.BF16, L.F16)[(i + j) % 2]
                rows.append((f"plan {vol} {cin}->{cout} dtype={dt}", (lambda a=(*vol, cin, cout, dt): plans(*a))))
    assert len(seen) == len(DTYPES) * len(ALGOS)
    return rows


def run(lib):
    """-> the table as a list of dicts, in a fixed order; once more with the options off that switch a fused form off: the valid
    arguments the entries refuse then, and the answers at 2 x 32^3."""
    out = []
    off = {"conv_fuse_gnb": 0, "gn3_fuse": 0, "conv_cm": 0, "conv_fuse_stats": 0}
    for options in ({}, off):
        before = {k: lib.mednet_get_option(k.encode(), 0 if k == "assume_cus" else 1) for k in ("assume_cus", *options)}
        for k, v in {"assume_cus": 256, **options}.items():
            lib.mednet_set_option(k.encode(), v)
        tag = "".join(f" [{k}={v}]" for k, v in options.items())
        try:
            for name, case, call in refusals(lib, tuple(options)):
                if options and not case.startswith("valid arguments"):
                    continue
                rc = call()
                assert rc < 0 and rc != E_HIP, (name, case, rc)  # (refused by a check: nothing reached a launch)
                out.append({"entry": "mednet_" + name, "case": case + tag, "rc": rc, "error": lib.mednet_last_error().decode(errors="replace")})
            for case, call in values(lib):
                if not options or str(VOLUMES[3]) in case:
                    out.append({"case": case + tag, "answers": call()})
        finally:
            for k, v in before.items():
                lib.mednet_set_option(k.encode(), v)
    return out


if __name__ == "__main__":
    for line in run(L.lib()):
        print(json.dumps(line))
