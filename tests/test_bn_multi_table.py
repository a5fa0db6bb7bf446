"""CPU: the group table of liso_bn_relu_bwd_multi (include/liso_bn.h) is checked on the host -- what the call cannot run is
LISO_EINVAL from liso_bn_relu_bwd_multi_check before anything could be launched -- and mfma_conv.bn_group_table lays the offsets out
as that check wants them.  The pointers are placeholders here: the check only tests them against NULL."""
import ctypes

import pytest

BF16, F32 = 1, 0


def _table(L, groups, ptr=0x1000):
    tab = (L.BnGroup * max(len(groups), 1))()
    for k, (off, c) in enumerate(groups):
        tab[k].c_off, tab[k].c = off, c
        tab[k].gamma = tab[k].stats = tab[k].grad_gamma = tab[k].grad_beta = ptr
    return tab


def _check(groups, n_grads=1, elem=BF16, m=300, xs=None, ga=None, gb=None, ds=None, ptr=0x1000):
    from liso_amd import _lib as L

    width = max((o + c for o, c in groups), default=8)
    n_fin = ctypes.c_int(-1)
    rc = L.lib().liso_bn_relu_bwd_multi_check(_table(L, groups, ptr), len(groups), n_grads, elem, m, xs or width, ga or width, gb or width,
                                              ds or width, ctypes.byref(n_fin))
    return rc, n_fin.value


def test_good_tables_are_accepted_with_the_single_calls_segments():
    # few row blocks: one finalize block per group; nblk >= 64 and c a multiple of 32 above 32: 32-channel segments
    assert _check([(0, 8)]) == (0, 1)
    assert _check([(0, 8), (8, 16), (24, 24)], n_grads=2) == (0, 3)
    assert _check([(0, 128), (128, 128), (256, 128)], m=129) == (0, 3)
    assert _check([(0, 128), (128, 128), (256, 128)], m=128 * 64) == (0, 12)
    assert _check([(0, 64), (64, 256)], m=128 * 64) == (0, 2 + 8)
    assert _check([(0, 32), (32, 64)], m=128 * 64) == (0, 1 + 2)  # (32 channels stay one segment)
    assert _check([(0, 4), (4, 12)], elem=F32) == (0, 2)
    assert _check([(0, 8), (16, 8)], xs=32, ga=24, ds=40) == (0, 2)  # a gap between the groups, rows wider than the groups


@pytest.mark.parametrize("case", ["no_group", "five_groups", "wide_group", "overlap", "descending", "unaligned_offset", "partial_lane",
                                  "fp32_lane", "past_x_row", "past_dy_b_row", "past_dx_row", "unaligned_stride", "no_rows", "null_pointer",
                                  "three_gradients", "bad_element"])
def test_bad_tables_are_refused(case):
    ok = [(0, 8), (8, 16)]
    rc = {
        "no_group": lambda: _check([]),
        "five_groups": lambda: _check([(8 * k, 8) for k in range(5)]),
        "wide_group": lambda: _check([(0, 264)]),
        "overlap": lambda: _check([(0, 16), (8, 16)]),
        "descending": lambda: _check([(16, 8), (0, 8)]),
        "unaligned_offset": lambda: _check([(4, 8)]),
        "partial_lane": lambda: _check([(0, 12)]),
        "fp32_lane": lambda: _check([(0, 6)], elem=F32),
        "past_x_row": lambda: _check(ok, xs=16),
        "past_dy_b_row": lambda: _check(ok, n_grads=2, gb=16),
        "past_dx_row": lambda: _check(ok, ds=16),
        "unaligned_stride": lambda: _check(ok, xs=28),
        "no_rows": lambda: _check(ok, m=0),
        "null_pointer": lambda: _check(ok, ptr=None),
        "three_gradients": lambda: _check(ok, n_grads=3),
        "bad_element": lambda: _check(ok, elem=7),
    }[case]()[0]
    assert rc != 0


def test_one_gradient_ignores_the_second_stride():
    assert _check([(0, 8), (8, 16)], n_grads=1, gb=8)[0] == 0


def test_python_table_builder_matches_the_check():
    from liso_amd.utils import mfma_conv as MC

    assert MC.bn_group_table([128, 128, 128], 8) == [(0, 128), (128, 128), (256, 128)]
    assert MC.bn_group_table([4, 12], 4) == [(0, 4), (4, 12)]
    for cs, vec in (([128, 128, 128], 8), ([64] * 4, 8), ([4, 12], 4)):
        assert _check(MC.bn_group_table(cs, vec), elem=BF16 if vec == 8 else F32)[0] == 0
    assert MC.bn_group_table([], 8) is None
    assert MC.bn_group_table([64] * 5, 8) is None
    assert MC.bn_group_table([264], 8) is None
    assert MC.bn_group_table([12, 8], 8) is None  # (the second group would start inside a 16-byte lane)
    assert MC.bn_group_table([4, 12], 8) is None
