"""CPU: the table of liso_adamw_step_packed_f32 (include/liso_optim.h) is checked and laid out on the host -- a bad table is
LISO_EINVAL from liso_adamw_pack_table_plan / _fill, before anything could be launched.  The pointers are host memory here: the
planner only compares them."""
import ctypes

import pytest
import torch

from tests.adamw_pack_cases import build_items, layout, plan

EINVAL = -1


def _items(mode_name="CONV_BF16"):
    from liso_amd import _lib as L

    keep = []

    def panel(nbytes):
        keep.append(torch.zeros(nbytes, dtype=torch.uint8))
        return keep[-1]

    def f32(shape):
        keep.append(torch.zeros(shape))
        return keep[-1]

    arr, n, panels, mirrors, placed = build_items(L, panel, f32, getattr(L, mode_name))
    return L, arr, n, keep


@pytest.mark.parametrize("mode", ["CONV_BF16", "CONV_F32X3", "CONV_F32"])
def test_good_table_plans_and_fills(mode):
    L, arr, n, keep = _items(mode)
    total = layout()[2]
    rc, nbytes, blocks = plan(L, arr, n, total)
    assert rc == 0 and nbytes > 0
    # one block per tile or plain range: at least the 5 x 3 tiles of the large filter, the 2 row tiles, one per other tensor
    assert blocks >= 15 + 2 + (n - 2)
    image = (ctypes.c_ubyte * nbytes)()
    assert L.lib().liso_adamw_pack_table_fill(arr, n, total, image, nbytes) == 0
    assert L.lib().liso_adamw_pack_table_fill(arr, n, total, image, nbytes - 8) == EINVAL  # (not the planned size)
    assert L.lib().liso_adamw_pack_table_fill(arr, n, total, None, nbytes) == EINVAL
    # a buffer that ends inside the last tensor
    assert plan(L, arr, n, total - 8)[0] == EINVAL
    # no listed tensor at all: the plain update in plain ranges
    assert plan(L, arr, 0, total)[0] == 0
    assert plan(L, None, 3, total)[0] == EINVAL


def _first(arr, n, pred):
    return next(i for i in range(n) if pred(arr[i]))


def test_bad_tables_are_refused():
    L, arr, n, keep = _items()
    total = layout()[2]
    assert plan(L, arr, n, total)[0] == 0

    def broken(edit):
        L2, a2, n2, keep2 = _items()
        edit(a2, n2)
        return plan(L2, a2, n2, total)[0]

    i_w = 0  # the [24, 8, 3, 3] filter: two panels of its own

    def null_panel(a, n_):
        a[i_w].dest[1].dst = None
    assert broken(null_panel) == EINVAL

    def misaligned_panel(a, n_):
        a[i_w].dest[0].dst += 8
    assert broken(misaligned_panel) == EINVAL

    def beyond_k(a, n_):
        a[i_w].dest[0].k_offset = 1  # K = 8 of a panel with K = 8
    assert broken(beyond_k) == EINVAL

    def beyond_n(a, n_):
        a[i_w].dest[0].n_offset = 1
    assert broken(beyond_n) == EINVAL

    def negative_offset(a, n_):
        a[i_w].dest[0].n_offset = -1
    assert broken(negative_offset) == EINVAL

    def fp16_panel(a, n_):
        a[i_w].dest[0].mode = L.CONV_F16
    assert broken(fp16_panel) == EINVAL

    def overlapping_tensors(a, n_):
        a[1].offset = a[0].offset + 16  # the second filter starts inside the first
    assert broken(overlapping_tensors) == EINVAL

    def unaligned_tensor(a, n_):
        a[i_w].offset += 2
    assert broken(unaligned_tensor) == EINVAL

    def three_dests(a, n_):
        a[i_w].n_dest = 3
    assert broken(three_dests) == EINVAL

    # two concatenated filters at the same place of their panel: they would share chunks
    cat = [i for i in range(n) if arr[i].n_dest == 2 and arr[i].dest[0].N == 32 and arr[i].dest[0].K == 16]
    assert len(cat) == 4

    def shared_chunks(a, n_):
        a[cat[1]].dest[0].n_offset = a[cat[0]].dest[0].n_offset
    assert broken(shared_chunks) == EINVAL

    # diagonal blocks 0 and 1 of the data-gradient panel in the same columns: both would write chunk 0 along k
    diag = [i for i in range(n) if arr[i].n_dest == 2 and arr[i].dest[0].N == 8 and arr[i].dest[0].K == 32]
    assert len(diag) == 4

    def shared_k_chunk(a, n_):
        a[diag[1]].dest[1].n_offset = a[diag[0]].dest[1].n_offset
    assert broken(shared_k_chunk) == EINVAL

    def same_panel_other_geometry(a, n_):
        a[cat[1]].dest[0].N = 40
    assert broken(same_panel_other_geometry) == EINVAL

    def overlapping_mirrors(a, n_):
        a[cat[1]].mirror = a[cat[0]].mirror
    assert broken(overlapping_mirrors) == EINVAL

    def mirror_over_panel(a, n_):
        a[cat[1]].mirror = a[i_w].dest[0].dst
    assert broken(mirror_over_panel) == EINVAL

    def short_mirror_stride(a, n_):
        a[cat[1]].mirror_row_stride = 16 * 9 - 4
    assert broken(short_mirror_stride) == EINVAL


def test_step_refuses_null_and_misaligned_arguments():
    from liso_amd import _lib as L

    lib = L.lib()
    buf = torch.zeros(64)
    p = buf.data_ptr()
    args = (1e-3, 0.9, 0.999, 1e-8, 0.01, 1.0)
    assert lib.liso_adamw_step_packed_f32(p, p, p, p, 64, *args, 1, None, 1, None) == EINVAL
    assert lib.liso_adamw_step_packed_f32(p, p, p, None, 64, *args, 1, p, 1, None) == EINVAL
    assert lib.liso_adamw_step_packed_f32(p, p, p, p, 64, *args, 0, p, 1, None) == EINVAL  # step counts from 1
    assert lib.liso_adamw_step_packed_f32(p, p, p, p, 64, *args, 1, p, 0, None) == EINVAL
    assert lib.liso_adamw_step_packed_f32(p + 4, p, p, p, 60, *args, 1, p, 1, None) == EINVAL
    job = L.ConvPackPlacedJob(p, p, 8, 8, 3, 3, 0, 0, L.CONV_BF16, 8, 8, 1, 0)  # k_offset 1 + K 8 > 8
    assert lib.liso_conv_pack_weights_placed(ctypes.byref(job), 1, 0, None) == EINVAL
    job = L.ConvPackPlacedJob(p, None, 8, 8, 3, 3, 0, 0, L.CONV_BF16, 8, 8, 0, 0)
    assert lib.liso_conv_pack_weights_placed(ctypes.byref(job), 1, 1, None) == EINVAL
    assert lib.liso_conv_pack_weights_placed(None, 0, 1, None) == 0
