"""Host side of the lazy head junction (no GPU): what mednet_gn_act_bwd_fused_res_head takes, and that only a block can mark a
GroupNorm-3 hook as accepting an unwritten head gradient (tests/test_gpu_head_lazy.py has the device side)."""
from mednet_hip import _lib as L
from mednet_hip import ops


def test_what_the_rebuilding_apply_pass_takes():
    lib = L.lib()
    for c, cout, dcode, ldt, want in ((32, 4, L.BF16, L.U8, 1), (32, 1, L.F16, L.I64, 1), (32, 5, L.BF16, L.U8, 0), (32, 4, L.F32, L.U8, 0),
                                      (16, 2, L.BF16, L.U8, 0), (64, 2, L.BF16, L.U8, 0), (32, 2, L.BF16, L.F32, 0)):
        assert lib.mednet_gn_act_bwd_fused_res_head_supported(c, cout, dcode, ldt) == want, (c, cout, dcode, ldt)


def test_a_hand_made_hook_is_never_lazy():
    assert ops.GN3Hook().lazy_head_ok is False and ops.GNBHook().lazy_head_ok is False
