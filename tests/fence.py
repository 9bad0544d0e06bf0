"""Guard bands around every tensor an operator touches: where do the kernels read and write?

`with Fence() as fence:` puts each allocation into a uint8 slab of its own and hands out a strided tensor over its storage,

    [ front guard | payload | back guard ]        (uint8; the WHOLE slab, payload included, holds the byte pattern)

and `fence.check()` compares every guard byte with the pattern afterwards.  The pattern 0x7FC07FC0 reads as NaN in fp32, bf16
and fp16 and as an out-of-range class in uint8 (192 / 127) and int64 labels, so

  * a store outside an output changes a guard: check() names the allocation (the call site's function, shape, dtype), the side,
    the first and last changed byte relative to the payload and the number of changed bytes;
  * a load outside an input, or of an output element nobody wrote, brings a NaN (or an impossible label) into the result: the
    operator's own exact result check fails by value;
  * a workspace query that under-reports is seen, because `mednet_hip._lib.workspace(nbytes, device)` hands out a fenced buffer
    of EXACTLY nbytes while the fence is open (ops.py passes ws.numel() on as ws_bytes), and so is a row query that
    under-reports, because the partial buffers come from the fenced `torch.empty`.

While the fence is open `torch.empty`, `torch.empty_like`, `torch.empty_strided` (ops.py allocates outputs with all three) and
`_lib.workspace` are replaced for tensors on the fence's device; CPU (unless the fence itself is a CPU fence), meta and pinned
allocations pass through.  All four are the originals again on exit, also after an exception.  `fence.put(t)` copies an input
into a slab with its strides kept, so that the `to_cl` / `.contiguous()` calls of ops.py stay no-ops and the kernel reads the
fenced copy.  `fence.owns(t)` says whether a tensor lives in a slab: a code path that bypasses the fence must not pass
silently, so every test asserts it for what the operator returned.  Nothing else is replaced here; where a test drives runners of
another test module that make device tensors with torch.zeros / torch.full / torch.tensor, tests/test_gpu_footprint.py (factories_in)
wraps those three itself for the duration of the test and puts each result into a slab: the kernel then sees the copy `put` made.

Alignment: the front guard is a multiple of 4096 bytes and the slab comes from the caching allocator, so a payload starts at
the alignment the allocator would have given it and the library's vector / scalar dispatch is the one of an ordinary run.  The
back guard starts at the payload's last byte + 1 -- no rounding, also at an odd address.

What the fence does not see: an access farther away from the payload than `guard` bytes (256 KiB by default, more than one
z-plane h * w * c * itemsize of every case of tests/test_gpu_footprint.py), a stray LOAD whose value never reaches a checked
result, and a store that writes the very bytes of the pattern.  It looks at memory contents only: everything an overrun of up
to `guard` bytes can hit lies inside an allocation of the test's own, no page boundary is mapped and no fault is provoked.
"""
import sys

import torch

DEV = "cuda:0"
PAGE = 4096
_THIS = __file__[:-1] if __file__.endswith(".pyc") else __file__

# the allocator entry points as they are outside a fence (the fence's own allocations use them)
_EMPTY, _EMPTY_LIKE, _EMPTY_STRIDED = torch.empty, torch.empty_like, torch.empty_strided


class FenceError(AssertionError):
    pass


def _caller():
    """Name of the first function outside this module on the stack: the allocation's call site."""
    f = sys._getframe(1)
    while f is not None and f.f_code.co_filename == _THIS:
        f = f.f_back
    return "?" if f is None else f.f_code.co_name


def _extent(shape, strides):
    """Elements spanned by a strided tensor (0 for an empty one)."""
    if any(s == 0 for s in shape):
        return 0
    return 1 + sum((s - 1) * st for s, st in zip(shape, strides))


class _Slab:
    __slots__ = ("raw", "front", "nbytes", "site", "shape", "dtype", "kind")

    def describe(self):
        return f"{self.kind} allocated in {self.site}(): shape {tuple(self.shape)} {self.dtype}, {self.nbytes} bytes"


class Fence:
    def __init__(self, pattern=0x7FC07FC0, guard=256 * 1024, device=DEV):
        self.pattern, self.guard = int(pattern), int(guard)
        self.device = torch.device(device)
        self.front = -(-self.guard // PAGE) * PAGE
        self.slabs = []
        self.ws_requests = []       # (bytes asked for, bytes served, call site)
        self._owned = {}            # storage address -> slab
        self._expected = {}         # (length, phase) -> the pattern's bytes
        self._open = False

    # ------------------------------------------------------------------------------------------------ the pattern
    def pattern_bytes(self):
        return [(self.pattern >> (8 * k)) & 0xFF for k in range(4)]

    def _pattern_run(self, length, phase):
        """`length` bytes of the pattern as they lie at slab offset `phase` (mod 4)."""
        key = (length, phase % 4)
        if key not in self._expected:
            four = torch.tensor(self.pattern_bytes(), dtype=torch.uint8)
            self._expected[key] = four.repeat(length // 4 + 2)[key[1]:key[1] + length].to(self.device)
        return self._expected[key]

    # ------------------------------------------------------------------------------------------------ slabs
    def _mine(self, device):
        d = torch.device(device) if device is not None else torch.tensor(()).device
        if d.type != self.device.type:
            return False
        return d.index is None or self.device.index is None or d.index == self.device.index

    def _slab(self, shape, strides, dtype, kind, site):
        shape, strides = tuple(int(s) for s in shape), tuple(int(s) for s in strides)
        item = _EMPTY((), dtype=dtype, device="meta").element_size()
        nbytes = _extent(shape, strides) * item
        total = -(-(self.front + nbytes + self.guard) // 4) * 4      # (whole pattern words; the back guard gets the remainder)
        s = _Slab()
        s.raw = _EMPTY(total, dtype=torch.uint8, device=self.device)
        s.raw.view(torch.int32).fill_(self.pattern - (1 << 32) if self.pattern >= (1 << 31) else self.pattern)
        s.front, s.nbytes, s.site, s.shape, s.dtype, s.kind = self.front, nbytes, site, shape, dtype, kind
        self.slabs.append(s)
        self._owned[s.raw.untyped_storage().data_ptr()] = s
        # The strided tensor over the slab's storage.  Not Tensor.as_strided: autograd refuses an in-place operation on an output
        # of a custom Function that is a view, and the fenced run must take the code path of an ordinary one.
        with torch.no_grad():
            return _EMPTY(0, dtype=dtype, device=self.device).set_(s.raw.untyped_storage(), s.front // item, shape, strides)

    def alloc(self, shape, dtype=torch.float32, memory_format=None, device=None, _kind="tensor"):
        """A tensor of `shape` in a slab of its own, filled with the pattern.  Strides come from a meta tensor of the same shape and
        memory format."""
        if device is not None and not self._mine(device):
            raise ValueError(f"fence.alloc: device {device} is not the fence's {self.device}")
        if isinstance(shape, int):
            shape = (shape,)
        kw = {} if memory_format is None else {"memory_format": memory_format}
        meta = _EMPTY(tuple(shape), dtype=dtype, device="meta", **kw)
        return self._slab(meta.shape, meta.stride(), dtype, _kind, _caller())

    def put(self, t):
        """A fenced copy of `t` with its strides kept (None stays None)."""
        if t is None:
            return None
        with torch.no_grad():
            out = self._slab(t.shape, t.stride(), t.dtype, "input", _caller())
            out.copy_(t.detach())
        return out

    def owns(self, t):
        """Does the tensor's storage lie in a slab of this fence?"""
        return t is not None and t.untyped_storage().data_ptr() in self._owned

    # ------------------------------------------------------------------------------------------------ the replacements
    def _empty(self, *size, **kw):
        if kw.get("out") is not None or kw.get("pin_memory") or kw.get("layout", torch.strided) is not torch.strided \
                or kw.get("names") is not None or not self._mine(kw.get("device")):
            return _EMPTY(*size, **kw)
        if "size" in kw:
            size = kw["size"]
        elif len(size) == 1 and not isinstance(size[0], int):
            size = size[0]
        dtype = kw.get("dtype") or torch.get_default_dtype()
        mf = kw.get("memory_format")
        meta = _EMPTY(tuple(size), dtype=dtype, device="meta", **({} if mf is None else {"memory_format": mf}))
        out = self._slab(meta.shape, meta.stride(), dtype, "torch.empty", _caller())
        return out.requires_grad_() if kw.get("requires_grad") else out

    def _empty_like(self, t, **kw):
        device = kw.get("device", t.device)
        if kw.get("pin_memory") or kw.get("layout", torch.strided) is not torch.strided or t.layout is not torch.strided \
                or not self._mine(device):
            return _EMPTY_LIKE(t, **kw)
        dtype = kw.get("dtype") or t.dtype
        like = _EMPTY_STRIDED(tuple(t.shape), t.stride(), dtype=t.dtype, device="meta")
        mf = kw.get("memory_format")
        meta = _EMPTY_LIKE(like, dtype=dtype, **({} if mf is None else {"memory_format": mf}))
        out = self._slab(meta.shape, meta.stride(), dtype, "torch.empty_like", _caller())
        return out.requires_grad_() if kw.get("requires_grad") else out

    def _empty_strided(self, size, stride, **kw):
        if kw.get("pin_memory") or kw.get("layout", torch.strided) is not torch.strided or not self._mine(kw.get("device")):
            return _EMPTY_STRIDED(size, stride, **kw)
        dtype = kw.get("dtype") or torch.get_default_dtype()
        out = self._slab(size, stride, dtype, "torch.empty_strided", _caller())
        return out.requires_grad_() if kw.get("requires_grad") else out

    def workspace(self, nbytes, dtype=torch.uint8):
        """A workspace of exactly `nbytes` bytes (as elements of `dtype`) for a test that calls the C ABI itself; counted like the
        requests of the library's wrappers."""
        nbytes, item = int(nbytes), _EMPTY((), dtype=dtype, device="meta").element_size()
        assert nbytes % item == 0, f"fence.workspace: {nbytes} bytes are no whole number of {dtype} elements"
        site = _caller()
        buf = self._slab((nbytes // item,), (1,), dtype, "workspace", site)
        self.ws_requests.append((nbytes, buf.numel() * item, site))
        return buf

    def _workspace(self, nbytes, device):
        """mednet_hip._lib.workspace while the fence is open: exactly `nbytes`, a fresh slab per request, no cache."""
        if not self._mine(device):
            return self._saved["workspace"](nbytes, device)
        return self.workspace(nbytes)

    def __enter__(self):
        from mednet_hip import _lib
        assert not self._open
        self._lib = _lib
        self._saved = {"empty": torch.empty, "empty_like": torch.empty_like, "empty_strided": torch.empty_strided,
                       "workspace": _lib.workspace, "cache": dict(_lib._ws_cache)}
        torch.empty, torch.empty_like, torch.empty_strided = self._empty, self._empty_like, self._empty_strided
        _lib.workspace = self._workspace
        self._open = True
        return self

    def __exit__(self, *exc):
        torch.empty, torch.empty_like, torch.empty_strided = (self._saved[k] for k in ("empty", "empty_like", "empty_strided"))
        self._lib.workspace = self._saved["workspace"]
        self._lib._ws_cache.clear()
        self._lib._ws_cache.update(self._saved["cache"])
        self._open = False
        return False

    # ------------------------------------------------------------------------------------------------ checks
    def _guards(self, s):
        back_at = s.front + s.nbytes
        return (("front", s.raw[:s.front], 0, -s.front), ("back", s.raw[back_at:], back_at, s.nbytes))

    def check(self):
        """Synchronise and compare every guard byte of every slab with the pattern.  Raises FenceError naming each changed guard."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        with torch.no_grad():
            counts = []
            for s in self.slabs:
                for _, g, at, _ in self._guards(s):
                    counts.append(torch.count_nonzero(g != self._pattern_run(g.numel(), at)))
            if not counts:
                return
            counts = torch.stack(counts).cpu().tolist()
            found = []
            for k, s in enumerate(self.slabs):
                for j, (side, g, at, rel) in enumerate(self._guards(s)):
                    if counts[2 * k + j]:
                        idx = (g != self._pattern_run(g.numel(), at)).nonzero().flatten()
                        first, last = int(idx[0]) + rel, int(idx[-1]) + rel
                        found.append(f"{side} guard of the {s.describe()}: {counts[2 * k + j]} bytes changed, first at payload offset "
                                     f"{first}, last at {last} (payload bytes are 0 .. {s.nbytes - 1})")
        if found:
            raise FenceError(f"{len(found)} guard band(s) changed:\n  " + "\n  ".join(found))

    def summary(self):
        """Counts for the audit record: fenced allocations, workspace bytes asked for / served, the largest payload."""
        return dict(allocations=len(self.slabs), ws_requests=len(self.ws_requests), ws_asked=sum(r[0] for r in self.ws_requests),
                    ws_served=sum(r[1] for r in self.ws_requests), largest_payload=max((s.nbytes for s in self.slabs), default=0))
