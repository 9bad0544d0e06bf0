"""Inputs, restatements and checkers of the optimiser tests (csrc/optim.hip; profiles/optim_bounds.md derives the bounds).

  * the plan numbers of the norm pass and a numpy model of its block decomposition (which element goes to which workgroup, thread and
    accumulator; every addition in fp32, in the kernel's order),
  * lattice gradients {0, +-1, +-2, +-3} * 2^e on which every fp32 partial of that model is exact,
  * torch restatements of the three update rules and the clip coefficient, evaluated in fp64 (the reference) or fp32 (its own error),
  * a reference stepper with the skip rule and the loss scaler's rule, with injectable faults,
  * the checkers the GPU tests assert with.  tests/test_optim_util.py runs all of it on the CPU.
"""
import types

import numpy as np
import torch

U32 = 2.0 ** -24
# ---- plan numbers of grad_sumsq_partial_kernel (the row count comes from the library: ops.grad_norm_rows)
THREADS, VEC, ACC, MAX_ROWS = 256, 4, 4, 2048
PER_ROW = THREADS * VEC * ACC               # elements one workgroup takes in one trip of its main loop
FRESH = (0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0)   # optimiser state {sumsq, norm, coef, nonfinite, steps taken, steps skipped, -, -}


def rows_of(count):
    from mednet_hip import ops
    return ops.grad_norm_rows(count)


def max_rows_count():
    """The smallest count that reaches MAX_ROWS partial rows (asserted against the library by the tests)."""
    return (MAX_ROWS - 1) * PER_ROW + 1


def ragged_count():
    """max_rows_count() plus one workgroup's share plus 5: the grid-stride loop takes a second trip, with a ragged tail."""
    return max_rows_count() + PER_ROW + 5


def gamma(k, u=U32):
    return k * u / (1.0 - k * u)


def head_of(offset):
    """Elements in front of the first 16-byte boundary for a pointer `offset` floats behind a 16-byte aligned address."""
    return (4 - offset % 4) % 4


# ------------------------------------------------------------------------------------------------ inputs
def _rng(tag):
    import zlib
    return np.random.default_rng(zlib.crc32(tag.encode()))


def lattice_grad(tag, count, e=0):
    """{0, +-1, +-2, +-3} * 2^e, float32: squares are integers <= 9 (times 4^e), a sum of fewer than 2^24 / 9 of them is exact in fp32."""
    v = _rng(tag).integers(-3, 4, size=count).astype(np.float32)
    return v * np.float32(2.0 ** e)


def exact_sumsq(g, gscale=1.0):
    """The exact sum of (g * gscale)^2 for lattice gradients and a power-of-two gscale, as a Python float (exactly representable in fp64:
    an integer below 2^53 times a power of two)."""
    g64 = g.astype(np.float64) * float(gscale)
    nz = g64[g64 != 0]
    if nz.size == 0:
        return 0.0
    unit = float(np.abs(nz).min())
    m = np.rint(g64 / unit).astype(np.int64)
    assert np.array_equal(m.astype(np.float64) * unit, g64) and int(np.abs(m).max()) <= 3 * 2 ** 20, "not a lattice input"
    total = int((m * m).sum())
    assert total < 2 ** 53
    return float(total) * unit * unit


# ------------------------------------------------------------------------------------------------ the norm pass, modelled
def norm_model(g, gscale, rows, head, fault=None):
    """fp32 partials [rows] of grad_sumsq_partial_kernel for the element array g (float32) behind a pointer whose first `head` elements
    lie in front of a 16-byte boundary.  -> (partials float32, longest accumulator chain, exact: every addition was exact).
    fault: 'skip_last' (the last element is never read), 'drop_tail' (the count % 4 trailing elements are never read)."""
    g = np.asarray(g, dtype=np.float32)
    count = g.size
    head = min(head, count)
    nvec, tail = (count - head) // VEC, (count - head) % VEC
    if fault == "drop_tail":
        tail = 0
    if fault == "skip_last":
        g = g.copy()
        g[-1] = 0.0
    s = (g * np.float32(gscale)).astype(np.float32)
    exact = [True]

    def fma(x, acc, mask=None):
        wide = x.astype(np.float64) * x.astype(np.float64) + acc.astype(np.float64)
        out = wide.astype(np.float32)
        ok = out.astype(np.float64) == wide
        exact[0] &= bool(ok.all() if mask is None else ok[mask].all())
        return out

    def add(a, b):
        wide = a.astype(np.float64) + b.astype(np.float64)
        out = wide.astype(np.float32)
        exact[0] &= bool(np.array_equal(out.astype(np.float64), wide))
        return out

    acc = np.zeros((ACC, rows, THREADS), dtype=np.float32)
    chain = np.zeros((ACC, rows, THREADS), dtype=np.int64)
    # head and tail: workgroup 0, threads 0..2 and 4..6, accumulator 0 starts as the square
    for t in range(head):
        acc[0, 0, t] = fma(s[t:t + 1], np.zeros(1, np.float32))[0]
        chain[0, 0, t] = 1
    for t in range(tail):
        acc[0, 0, 4 + t] = fma(s[head + VEC * nvec + t:head + VEC * nvec + t + 1], np.zeros(1, np.float32))[0]
        chain[0, 0, 4 + t] = 1
    body = s[head:head + VEC * nvec].reshape(nvec, VEC)
    stride = rows * THREADS
    trips = -(-nvec // stride) if nvec else 0
    padded = np.zeros((max(trips, 1) * stride, VEC), dtype=np.float32)
    live = np.zeros(max(trips, 1) * stride, dtype=bool)
    padded[:nvec] = body
    live[:nvec] = True
    padded = padded.reshape(-1, rows, THREADS, VEC)      # [trip][row][thread][component]
    live = live.reshape(-1, rows, THREADS)
    n_t = live.sum(axis=0)                               # float4s of each thread
    main = n_t // ACC                                    # trips of the unrolled loop (they need all four loads in range)
    for j in range(trips):
        k = np.where(j < main * ACC, j % ACC, 0)         # accumulator of this thread's j-th float4
        for a in range(ACC):
            sel = live[j] & (k == a)
            if not sel.any():
                continue
            cur = acc[a]
            for c in range(VEC):
                upd = fma(padded[j, :, :, c], cur, sel)
                cur = np.where(sel, upd, cur)
            acc[a] = cur
            chain[a] += VEC * sel
    thread = add(add(acc[0], acc[1]), add(acc[2], acc[3]))          # (a0 + a1) + (a2 + a3)
    lanes = thread.reshape(rows, THREADS // 64, 64)
    for step in (1, 2):                                             # quad_perm: lane ^ 1, lane ^ 2
        idx = np.arange(64) ^ step
        lanes = add(lanes, lanes[..., idx])
    for ror in (4, 8):                                              # row_ror within 16-lane rows
        idx = (np.arange(64) & ~15) | ((np.arange(64) + ror) & 15)
        lanes = add(lanes, lanes[..., idx])
    for step in (16, 32):
        idx = np.arange(64) ^ step
        lanes = add(lanes, lanes[..., idx])
    wave = lanes[..., 0]                                            # [rows][4]
    part = np.zeros(rows, dtype=np.float32)
    for w in range(THREADS // 64):                                  # block_sum: t = 0; t += scratch[w]
        part = add(part, wave[:, w])
    return part, int(chain.max()), exact[0]


def chain_length(count, rows, head):
    """The longest accumulator chain of the norm pass (fused multiply-adds into one accumulator) for this plan, without running
    the model: a thread with q float4s runs q // 4 unrolled trips (4 fmas into each accumulator) and q % 4 single ones (4 fmas into
    accumulator 0 each); accumulator 0 of workgroup 0 may start from a head or tail element."""
    head = min(head, count)
    nvec = (count - head) // VEC
    q = -(-nvec // (rows * THREADS))
    best = max((n // ACC + n % ACC) for n in {q, max(q - 1, 0)})
    return VEC * best + 1


def sumsq_terms(count, rows, head):
    """k of the bound |sumsq - S| <= gamma_k S (profiles/optim_bounds.md): one rounding of g * gscale counted twice (it is squared),
    the accumulator chain, 2 additions joining the accumulators, 6 wave levels, 4 block additions, 1 for the fp64 finalize, 1 final."""
    return 2 + chain_length(count, rows, head) + 2 + 6 + 4 + 1 + 1


def norm_bound(count, rows, head):
    """Relative bound of `norm`: half the sum's (before its final rounding) plus the rounding of the square root's result."""
    return 0.5 * gamma(sumsq_terms(count, rows, head)) + 2.0 * U32


def finalize64(partials, max_norm):
    """grad_norm_finalize_kernel: the fp64 sum of the partials -> the fp32 fields {sumsq, norm, coef, nonfinite}."""
    total = float(np.sum(partials.astype(np.float64)))      # (exact inputs: any order; random ones: compared with a tolerance)
    with np.errstate(invalid="ignore", over="ignore"):
        sumsq = np.float32(total)
        norm = np.float32(np.sqrt(total))
    bad = not np.isfinite(sumsq)
    coef = np.float32(min(1.0, max_norm / (np.sqrt(total) + 1e-6))) if (max_norm and not bad) else np.float32(1.0)
    return float(sumsq), float(norm), float(coef), float(bad)


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def check_norm_exact(state, g, gscale, what):
    """Lattice gradient: sumsq is the correctly rounded exact sum, norm within one ulp of the fp64 square root, nonfinite clear."""
    st = [float(x) for x in state[:4]]
    S = exact_sumsq(g, gscale)
    assert st[0] == float(np.float32(S)), f"{what}: sumsq {st[0]!r}, the exact sum is {S!r} (fp32 {float(np.float32(S))!r})"
    root = float(np.sqrt(S))
    assert abs(st[1] - root) <= ulp32(root), f"{what}: norm {st[1]!r} against sqrt {root!r}"
    assert st[3] == 0.0, f"{what}: nonfinite is set"


def check_norm_random(state, g64_scaled, count, rows, head, what):
    """-> (observed relative error of sumsq, of norm); asserts both against the derived bounds."""
    S = float(np.sum(g64_scaled * g64_scaled))
    k = sumsq_terms(count, rows, head)
    e_s = abs(float(state[0]) - S) / S
    e_n = abs(float(state[1]) - np.sqrt(S)) / np.sqrt(S)
    assert e_s <= gamma(k), f"{what}: sumsq relative error {e_s:.3e} > gamma_{k} = {gamma(k):.3e}"
    assert e_n <= norm_bound(count, rows, head), f"{what}: norm relative error {e_n:.3e} > {norm_bound(count, rows, head):.3e}"
    return e_s, e_n


# ------------------------------------------------------------------------------------------------ the update rules, restated
def _s(x, dtype):
    return torch.tensor(float(np.float32(x)), dtype=dtype)     # the fp32 number the C ABI receives


def clip_coef(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient: min(1, max_norm / (norm + 1e-6)); 1 when clipping is off."""
    if not max_norm:
        return 1.0
    return min(1.0, float(max_norm) / (float(norm) + 1e-6))


def effective_grad(g, gscale, coef, dtype):
    """gr = (g * gscale) * coef, in that order."""
    return (g.to(dtype) * _s(gscale, dtype)) * torch.as_tensor(coef, dtype=dtype)


def sgd_lines(p, g, buf, lr, mu, nesterov, wd, gscale, coef, dtype, fault=None):
    """torch.optim.SGD with dampening 0, as the kernel states it.  -> p', buf' (buf' is None when mu == 0), norms of the bound."""
    p = p.to(dtype)
    gr0 = effective_grad(g, gscale, coef, dtype)
    gr = gr0 + _s(wd, dtype) * p if wd else gr0
    terms = gr0.abs() + (_s(wd, dtype) * p).abs() if wd else gr0.abs()
    if mu:
        b = _s(mu, dtype) * buf.to(dtype) + gr
        terms_b = (_s(mu, dtype) * buf.to(dtype)).abs() + terms
        d = gr + _s(mu, dtype) * b if (nesterov and fault != "no_nesterov") else b
        terms_d = terms + _s(mu, dtype) * terms_b if nesterov else terms_b
    else:
        b, terms_b, d, terms_d = None, None, gr, terms
    delta = _s(lr, dtype) * d
    return types.SimpleNamespace(p=p - delta, buf=b, delta=delta, terms_b=terms_b, terms_d=_s(lr, dtype) * terms_d)


def adam_lines(p, g, m, v, lr, b1, b2, eps, wd, step, gscale, coef, decoupled, dtype, fault=None):
    """torch.optim.Adam (L2 decay) / torch.optim.AdamW (decoupled) with the clip coefficient on the gradient.  -> p', m', v', norms."""
    if fault == "coupled":
        decoupled = False
    p, m, v = p.to(dtype), m.to(dtype), v.to(dtype)
    lr_, b1_, b2_, eps_, wd_, one = (_s(x, dtype) for x in (lr, b1, b2, eps, wd, 1.0))
    gr0 = effective_grad(g, gscale, coef, dtype)
    shrunk = p * (one - lr_ * wd_) if (decoupled and wd) else p
    gr = gr0 + wd_ * p if (wd and not decoupled) else gr0
    terms = gr0.abs() + ((wd_ * p).abs() if (wd and not decoupled) else 0.0)
    m1 = b1_ * m + (one - b1_) * gr
    v1 = b2_ * v + (one - b2_) * gr * gr
    t = _s(step, dtype)
    bc1, bc2 = one - b1_ ** t, one - b2_ ** t
    denom = v1.sqrt() / bc2.sqrt() + eps_
    delta = (lr_ / bc1) * (m1 / denom)
    terms_m = (b1_ * m).abs() + (one - b1_) * terms
    terms_d = (lr_ / bc1) * (terms_m / denom) + (p - shrunk).abs()
    return types.SimpleNamespace(p=shrunk - delta, m=m1, v=v1, delta=(p - shrunk) + delta, terms_m=terms_m, terms_v=v1, terms_d=terms_d)


class Reference:
    """The whole step on the host in `dtype`: norm of the unscaled mean gradient, clip coefficient, skip rule, update, counters and
    the loss scaler's rule.  kind: 'sgd' | 'adam' | 'adamw'.  State tensors: p and (buf) or (m, v).  scaler: None or
    [scale, good, steps, found_inf, skipped] with (growth, backoff, interval).  fault: see tests/test_optim_util.py."""

    def __init__(self, kind, p, hp, max_norm=None, inv_world=1.0, scaler=None, rule=(2.0, 0.5, 2000), dtype=torch.float64, fault=None):
        self.kind, self.hp, self.max_norm, self.inv_world, self.dtype, self.fault = kind, dict(hp), max_norm, inv_world, dtype, fault
        self.p = p.to(dtype).clone()
        self.buf = torch.zeros_like(self.p) if (kind == "sgd" and hp.get("mu")) else None
        self.m, self.v = (torch.zeros_like(self.p), torch.zeros_like(self.p)) if kind != "sgd" else (None, None)
        self.steps, self.skipped = 0, 0
        self.scaler, self.rule = (None if scaler is None else list(scaler)), rule
        self.norm = self.coef = None
        self.last = None

    def gscale(self):
        s = np.float32(self.inv_world)
        return float(s / np.float32(self.scaler[0])) if self.scaler is not None else float(s)

    def step(self, g, coef=None):
        """One call with the (scaled) gradient g.  coef: override (the exact tests set it by hand)."""
        gscale = self.gscale()
        gs = g.to(self.dtype) * _s(gscale, self.dtype)       # (the fp32 evaluation takes its norm in fp32 as well)
        sumsq = float((gs * gs).sum())
        with np.errstate(over="ignore", invalid="ignore"):
            bad = not np.isfinite(np.float32(sumsq))
        self.norm = float(np.sqrt(sumsq)) if not bad else float("nan")
        norm_for_clip = float((g.double() ** 2).sum().sqrt()) if self.fault == "clip_before_unscale" else self.norm
        self.coef = coef if coef is not None else (1.0 if bad else clip_coef(norm_for_clip, self.max_norm))
        if bad and self.fault != "no_skip":
            self.skipped += 1
            if self.fault == "count_on_skip":
                self.steps += 1
            self._scaler_rule(True)
            return False
        h = self.hp
        if self.kind == "sgd":
            r = sgd_lines(self.p, g, self.buf, h["lr"], h.get("mu", 0.0), h.get("nesterov", False), h.get("wd", 0.0), gscale, self.coef,
                          self.dtype, self.fault)
            self.p, self.buf = r.p, r.buf
        else:
            r = adam_lines(self.p, g, self.m, self.v, h["lr"], h["b1"], h["b2"], h["eps"], h.get("wd", 0.0), self.steps + 1, gscale,
                           self.coef, self.kind == "adamw", self.dtype, self.fault)
            self.p, self.m, self.v = r.p, r.m, r.v
        self.last = r
        self.steps += 1
        self._scaler_rule(False)
        return True

    def _scaler_rule(self, bad):
        if self.scaler is None:
            return
        sc, (growth, backoff, interval) = self.scaler, self.rule
        if bad:
            sc[0], sc[1], sc[4] = max(sc[0] * backoff, 1.0), 0.0, sc[4] + 1.0
        else:
            sc[2], sc[1] = sc[2] + 1.0, sc[1] + 1.0
            if sc[1] >= interval:
                sc[0], sc[1] = sc[0] * growth, 0.0
        sc[3] = 0.0

    def state(self):
        return {k: t for k, t in (("p", self.p), ("buf", self.buf), ("m", self.m), ("v", self.v)) if t is not None}


# ------------------------------------------------------------------------------------------------ checkers
def check_bits(got, ref, what):
    """Every state tensor equals the fp64 reference bit for bit (the reference must be representable in fp32: exact arithmetic)."""
    for k, r in ref.items():
        r = r.double().cpu()
        assert torch.equal(r.float().double(), r), f"{what}: the reference's {k} is not representable in fp32 -- the case is not exact"
        g = got[k].double().cpu()
        bad = (g != r) | torch.isnan(g)
        assert not bool(bad.any()), (f"{what}: {k} differs at {int(bad.sum())} of {g.numel()} elements, first at "
                                     f"{int(bad.nonzero()[0])}: got {g[bad][0].item()!r} want {r[bad][0].item()!r}")


def check_unchanged(got, before, what):
    """A skipped step: every state tensor keeps its bits (NaNs compared as bits)."""
    for k, b in before.items():
        same = torch.equal(got[k].cpu().view(torch.int32), b.cpu().view(torch.int32))
        assert same, f"{what}: {k} changed on a skipped step"


def check_counts(steps, skipped, want_steps, want_skipped, what):
    assert (steps, skipped) == (want_steps, want_skipped), \
        f"{what}: steps taken / skipped {steps} / {skipped}, want {want_steps} / {want_skipped}"


def one_step(kind, state, g, hp, step, gscale, coef, dtype, fault=None):
    """One update from `state` (dict of p and buf or m, v; fp32 tensors) in `dtype` -> the namespace of sgd_lines / adam_lines."""
    if kind == "sgd":
        return sgd_lines(state["p"], g, state.get("buf"), hp["lr"], hp.get("mu", 0.0), hp.get("nesterov", False), hp.get("wd", 0.0), gscale,
                         coef, dtype, fault)
    return adam_lines(state["p"], g, state["m"], state["v"], hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp.get("wd", 0.0), step, gscale, coef,
                      kind == "adamw", dtype, fault)


def _tensors(kind, r, hp):
    """(name, value, norm of the bound, the quantity whose fp32 error is r32) of one step's results.  For p that quantity is the
    update p - p', not p': the final rounding of p' (2^-24 |p|, which check_update allows on top) is no part of the update's error
    and would swamp it wherever the update is small against p."""
    if kind == "sgd":
        out = [("p", r.p, r.terms_d, r.delta)]
        return out + [("buf", r.buf, r.terms_b, r.buf)] if hp.get("mu") else out
    return [("p", r.p, r.terms_d, r.delta), ("m", r.m, r.terms_m, r.m), ("v", r.v, r.terms_v, r.v)]


def update_reference(kind, state, g, hp, step, gscale, max_norm):
    """fp64 and fp32 evaluations of one whole step (norm, clip coefficient, update) from `state`, and the project's per-tensor rule
    eps_case = max(2^-20, 8 * r32) (gpu_util.ref_error with LOSS_EPS_FLOOR), r32 the fp32 evaluation's own error in the bound's norm."""
    import gpu_util as GU
    out = types.SimpleNamespace(eps={}, r32s={})
    for dtype in (torch.float64, torch.float32):
        gs = g.to(dtype) * _s(gscale, dtype)
        norm = float((gs * gs).sum().sqrt())
        r = one_step(kind, state, g, hp, step, gscale, clip_coef(norm, max_norm), dtype)
        if dtype == torch.float64:
            out.r64, out.norm, out.coef = r, norm, clip_coef(norm, max_norm)
        else:
            out.r32 = r
    for (name, _, n64, e64), (_, _, _, e32) in zip(_tensors(kind, out.r64, hp), _tensors(kind, out.r32, hp)):
        out.r32s[name], out.eps[name] = GU.ref_error(e32, e64, n64, f"{kind} {name}", floor=GU.LOSS_EPS_FLOOR)
    return out


def check_update(kind, ref, got, hp, what):
    """|got - ref64| <= eps_case * (the tensor's sum of |terms|) (+ 2^-24 |p64| for p: its own final rounding).  -> observed ratios."""
    import gpu_util as GU
    return {name: GU.check_gradient(got[name], x64, n64, ref.eps[name], f"{what}: {name}", u=U32 if name == "p" else 0.0)
            for name, x64, n64, _ in _tensors(kind, ref.r64, hp)}


DYADIC = dict(lr=0.5, mu=0.5, wd=0.5, coef=0.5)   # each step adds at most 3 fraction bits to p (wd, the Nesterov term, lr)


def dyadic_case(tag, count, steps=5):
    """p and the gradients of `steps` steps as small integers: with lr, mu, wd and coef powers of two every line of the SGD rule is
    exact in fp32, fused or not.  With DYADIC's values p holds 15 fraction bits and fewer than 5 integer bits after five steps, the
    buffer 13 and 5 (check_bits asserts that the fp64 reference is representable in fp32)."""
    r = _rng(tag)
    p = torch.from_numpy(r.integers(-8, 9, size=count).astype(np.float32))
    gs = [torch.from_numpy(r.integers(-4, 5, size=count).astype(np.float32)) for _ in range(steps)]
    return p, gs


def random_case(tag, count, steps=5, gstd=1.0):
    r = _rng(tag)
    f = lambda a: torch.from_numpy(a.astype(np.float32))
    p = f(r.standard_normal(count))
    gs = [f(gstd * r.standard_normal(count)) for _ in range(steps)]
    for g in gs:
        g[::16] = 0.0
    return p, gs
