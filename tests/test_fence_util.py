"""CPU side of tests/fence.py, no GPU and no kernel: the fence must reject the faults it is there for.  A CPU Fence
(device="cpu") around torch / numpy stand-ins for a kernel, ONE injected fault at a time: a store one byte outside a payload on
either side and at the far end of the guard, an 8-wide store on a ragged count, a reduce over one row too many, a load one vector
too far whose value is multiplied by zero, and a workspace whose query under-reports.  Every rejection must name the allocation
(call site, shape, dtype), the side and the byte offsets."""
import numpy as np
import pytest
import torch

from mednet_hip import _lib as L

import fence as F
from fence import Fence, FenceError

GUARD = 4096      # (small guards keep the CPU slabs small; the arithmetic of the fence does not depend on the size)


def raw_bytes(fence, t):
    """The numpy view of the whole slab a fenced CPU tensor lives in, and the payload's offset in it: what a kernel's pointer sees."""
    slab = fence._owned[t.untyped_storage().data_ptr()]
    return slab.raw.numpy(), slab.front


def test_clean_use_passes_and_the_layout_is_as_documented():
    with Fence(guard=GUARD, device="cpu") as fence:
        t = fence.alloc((3, 5), torch.float32)
        cl = fence.alloc((2, 4, 3, 5, 6), torch.bfloat16, memory_format=torch.channels_last_3d)
        assert fence.owns(t) and fence.owns(cl) and not fence.owns(torch.zeros(3))
        assert cl.stride() == torch.empty((2, 4, 3, 5, 6), device="meta", memory_format=torch.channels_last_3d).stride()
        assert cl.is_contiguous(memory_format=torch.channels_last_3d) and t.is_contiguous()
        raw, front = raw_bytes(fence, t)
        assert front % 4096 == 0 and front >= GUARD and t.data_ptr() == fence._owned[t.untyped_storage().data_ptr()].raw.data_ptr() + front
        assert raw.size >= front + 60 + GUARD
        assert bool(torch.isnan(t).all()) and bool(torch.isnan(cl.float()).all())   # (the payload holds the pattern too)
        t.copy_(torch.arange(15.0).reshape(3, 5))
        cl.zero_()
        fence.check()
        s = fence.summary()
        assert s["allocations"] == 2 and s["largest_payload"] == 2 * 4 * 3 * 5 * 6 * 2 and s["ws_requests"] == 0


def test_the_pattern_is_nan_in_every_float_type_and_no_class_in_the_label_types():
    with Fence(guard=GUARD, device="cpu") as fence:
        assert fence.pattern == 0x7FC07FC0
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            assert bool(torch.isnan(fence.alloc((7,), dt)).all()), dt
        assert int(fence.alloc((9,), torch.uint8).min()) >= 32
        lab = fence.alloc((9,), torch.int64)
        assert bool(((lab < 0) | (lab >= 32)).all())
        odd = fence.alloc((3,), torch.uint8)[1:]       # (whatever the phase, a byte of the pattern is 0xC0 or 0x7F)
        assert set(odd.tolist()) <= {0xC0, 0x7F}


@pytest.mark.parametrize("where,side,offset", [("behind", "back", 60), ("in_front", "front", -1), ("guard_end", "back", None)])
def test_one_byte_outside_the_payload_fails_the_check(where, side, offset):
    with Fence(guard=GUARD, device="cpu") as fence:
        def kernel_under_test():
            return fence.alloc((3, 5), torch.float32)
        t = kernel_under_test()
        t.zero_()
        raw, front = raw_bytes(fence, t)
        at = {"behind": front + 60, "in_front": front - 1, "guard_end": raw.size - 1}[where]
        raw[at] = np.uint8(raw[at] ^ 0x01)
        want = at - front
        with pytest.raises(FenceError) as e:
            fence.check()
    msg = str(e.value)
    assert f"{side} guard" in msg and "kernel_under_test()" in msg and "shape (3, 5)" in msg and "torch.float32" in msg
    assert f"1 bytes changed, first at payload offset {want}, last at {want}" in msg
    if offset is not None:
        assert want == offset


def test_an_eight_wide_store_on_a_ragged_count_changes_the_back_guard_by_the_right_size():
    count = 8 * 5 + 3
    with Fence(guard=GUARD, device="cpu") as fence:
        out = fence.alloc((count,), torch.bfloat16)
        raw, front = raw_bytes(fence, out)
        vec = np.zeros(8, dtype=np.uint16).view(np.uint8)
        for i in range(0, count, 8):                       # the faulty kernel: whole vectors, no tail handling
            raw[front + 2 * i:front + 2 * i + 16] = vec
        with pytest.raises(FenceError) as e:
            fence.check()
    msg = str(e.value)
    assert "back guard" in msg and "shape (43,)" in msg and "torch.bfloat16" in msg
    assert f"10 bytes changed, first at payload offset {2 * count}, last at {2 * count + 9}" in msg    # 5 elements of 2 bytes
    assert "front guard" not in msg


def test_a_reduce_over_one_row_too_many_gives_nan():
    rows, c = 3, 4
    with Fence(guard=GUARD, device="cpu") as fence:
        partial = fence.alloc((1, rows, c, 2), torch.float32)
        partial.copy_(torch.ones(1, rows, c, 2))
        raw, front = raw_bytes(fence, partial)
        flat = raw[front:front + (rows + 1) * c * 2 * 4].view(np.float32).reshape(rows + 1, c, 2)   # what the pointer reaches
        assert np.array_equal(flat[:rows].sum(0), np.full((c, 2), 3.0, dtype=np.float32))
        assert np.isnan(flat.sum(0)).all()       # rows + 1: the row query under-reported
        fence.check()                            # (a load changes nothing: the VALUE is what gives it away)


def test_a_load_one_vector_too_far_times_zero_still_gives_nan():
    with Fence(guard=GUARD, device="cpu") as fence:
        x = fence.put(torch.arange(16, dtype=torch.float32))
        assert fence.owns(x) and torch.equal(x, torch.arange(16.0))
        raw, front = raw_bytes(fence, x)
        seen = torch.from_numpy(raw[front:front + 4 * 24].view(np.float32))     # 16 elements and one 8-wide vector more
        w = torch.cat((torch.ones(16), torch.zeros(8)))                         # the tail is "masked" by a zero weight
        assert float((seen[:16] * w[:16]).sum()) == 120.0
        assert bool(torch.isnan((seen * w).sum()))
        front_too = torch.from_numpy(raw[front - 32:front + 64].view(np.float32))
        assert bool(torch.isnan((front_too * 0.0).sum()))


def test_put_keeps_strides_and_values():
    t = torch.arange(2 * 3 * 2 * 2 * 2, dtype=torch.float32).reshape(2, 3, 2, 2, 2).contiguous(memory_format=torch.channels_last_3d)
    lab = torch.arange(24, dtype=torch.int64).reshape(2, 3, 4)[:, -1]            # an int64 view with a sample stride
    with Fence(guard=GUARD, device="cpu") as fence:
        a, b = fence.put(t), fence.put(lab)
        assert a.stride() == t.stride() and torch.equal(a, t) and b.stride() == lab.stride() and torch.equal(b, lab)
        assert fence.put(None) is None
        fence.check()


def test_an_under_reported_workspace_is_caught():
    nbytes = 1000
    with Fence(guard=GUARD, device="cpu") as fence:
        def op_under_test():
            ws = L.workspace(nbytes, "cpu")
            assert ws.numel() == nbytes and ws.dtype == torch.uint8      # exactly what was asked for, not the cache's 1 MiB
            return ws
        ws = op_under_test()
        assert fence.owns(ws) and fence.ws_requests == [(nbytes, nbytes, "op_under_test")]
        raw, front = raw_bytes(fence, ws)
        raw[front:front + nbytes + 64] = 0          # the kernel needs 64 bytes more than its query said
        with pytest.raises(FenceError) as e:
            fence.check()
    msg = str(e.value)
    assert "back guard of the workspace allocated in op_under_test()" in msg
    assert f"first at payload offset {nbytes}, last at {nbytes + 63}" in msg
    assert fence.summary()["ws_asked"] == nbytes == fence.summary()["ws_served"]


def test_an_empty_workspace_is_still_fenced():
    with Fence(guard=GUARD, device="cpu") as fence:
        ws = L.workspace(0, "cpu")
        assert ws.numel() == 0 and fence.owns(ws)
        raw, front = raw_bytes(fence, ws)
        raw[front] = 0
        with pytest.raises(FenceError, match="first at payload offset 0"):
            fence.check()


def test_the_library_allocators_are_fenced_inside_and_the_originals_outside():
    empty, empty_like, empty_strided, workspace = torch.empty, torch.empty_like, torch.empty_strided, L.workspace
    cache = dict(L._ws_cache)
    with Fence(guard=GUARD, device="cpu") as fence:
        assert torch.empty is not empty and L.workspace is not workspace
        a = torch.empty((2, 3), dtype=torch.float32, device="cpu")
        b = torch.empty(2, 4, 2, 2, 2, dtype=torch.bfloat16, memory_format=torch.channels_last_3d)
        c = torch.empty_like(b, memory_format=torch.channels_last_3d)
        d = torch.empty_like(b, dtype=torch.float32)
        e = torch.empty_strided((2, 3), (1, 2), dtype=torch.float16)
        z = torch.empty(0)
        s = torch.empty((), dtype=torch.float32)
        for t in (a, b, c, d, e, z, s):
            assert fence.owns(t)
        assert c.stride() == b.stride() == d.stride() and d.dtype == torch.float32 and e.stride() == (1, 2) and s.dim() == 0
        assert not fence.owns(torch.empty((2, 3), device="meta"))
        assert bool(torch.isnan(a).all())
        fence.check()
    assert (torch.empty, torch.empty_like, torch.empty_strided, L.workspace) == (empty, empty_like, empty_strided, workspace)
    assert L._ws_cache == cache
    with pytest.raises(RuntimeError, match="boom"):
        with Fence(guard=GUARD, device="cpu"):
            raise RuntimeError("boom")
    assert (torch.empty, torch.empty_like, torch.empty_strided, L.workspace) == (empty, empty_like, empty_strided, workspace)
    assert F._EMPTY is empty


def test_a_device_fence_leaves_cpu_allocations_alone():
    f = Fence(guard=GUARD)          # (device cuda:0; nothing is allocated there)
    f._saved = {"workspace": None}
    assert not f._mine("cpu") and not f._mine(torch.device("meta")) and f._mine("cuda:0") and f._mine("cuda") and not f._mine("cuda:1")


def test_an_odd_payload_has_its_guard_at_the_next_byte():
    with Fence(guard=GUARD, device="cpu") as fence:
        lab = fence.put(torch.arange(37, dtype=torch.uint8))
        raw, front = raw_bytes(fence, lab)
        assert raw[front + 36] == 36 and raw[front + 37] in (0xC0, 0x7F)       # the last label, then the pattern at once
        fence.check()
        raw[front + 37] = 1                                                     # a label read one byte too far would see this address
        with pytest.raises(FenceError, match="1 bytes changed, first at payload offset 37, last at 37"):
            fence.check()
