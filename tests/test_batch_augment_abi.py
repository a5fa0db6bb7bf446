"""CPU: the batched augmentation's entry points (include/liso_augment.h) check their arguments before anything is launched, so they
answer without a GPU.  (That every declared symbol is exported and typed is tests/test_abi.py's.)"""
import ctypes

import pytest

EINVAL, EWORKSPACE = -1, -2
FAKE = 0x10000  # a 16-byte aligned non-null address; the checks never dereference it


def _cfg(**over):
    from liso_amd import _lib

    f = dict(batch=3, n_max=2048, h=64, w=64, radius=4, max_num_objs=15, num_snippets=9, db_rows=2003, extra_capacity=300, selection=1,
             range_x=32.0, range_y=32.0, cell_x=0.5, cell_y=0.5, max_scale_delta=0.2, max_points_dropout=0.25, vmin=1.0, vmax=3.0)
    f.update(over)
    return _lib.AugmentBatchCfg(**f)


# the pointer arguments of liso_snippet_augment_batch between cfg and workspace, in order
POINTERS = ("pillar_coors", "counts", "db_points", "db_offsets", "db_dims", "db_pos_z", "db_lidar_rows", "state", "sample_ids",
            "extra_points", "extra_flow", "extra_counts", "object_offsets", "box_pos", "box_dims", "box_rot", "box_velo", "box_valid",
            "draws", "overflow", "kept_rows")
OPTIONAL = ("db_lidar_rows", "extra_flow", "kept_rows")  # (db_lidar_rows: optional unless the selection is the ray-drop)


def _call(cfg, workspace_bytes=None, **null):
    from liso_amd import _lib

    lib = _lib.lib()
    need = lib.liso_snippet_augment_batch_workspace_bytes(ctypes.byref(cfg))
    ptrs = [None if null.get(name) else ctypes.c_void_p(FAKE) for name in POINTERS]
    return lib.liso_snippet_augment_batch(ctypes.byref(cfg), *ptrs, ctypes.c_void_p(FAKE), need if workspace_bytes is None else workspace_bytes,
                                          None)


def test_workspace_size_and_one_byte_short():
    from liso_amd import _lib

    lib = _lib.lib()
    cfg = _cfg()
    need = lib.liso_snippet_augment_batch_workspace_bytes(ctypes.byref(cfg))
    # at least: occupancy + mask bytes, prefix, poses, kept rows
    assert need >= 3 * 64 * 64 * 2 + 3 * 65 * 4 + 3 * 15 * 12 * 8 + 3 * 300 * 8
    assert _call(cfg, workspace_bytes=need - 1) == EWORKSPACE
    assert lib.liso_snippet_augment_batch_workspace_bytes(None) == 0
    assert lib.liso_bev_free_mask_batch_workspace_bytes(3, 64, 70) == 3 * 64 * 128
    assert lib.liso_bev_free_mask_batch_workspace_bytes(0, 64, 64) == 0


@pytest.mark.parametrize("over", [dict(batch=0), dict(batch=-1), dict(max_num_objs=65), dict(max_num_objs=0), dict(num_snippets=0),
                                  dict(h=0), dict(w=-3), dict(radius=256), dict(radius=-1), dict(selection=3), dict(extra_capacity=-1),
                                  dict(db_rows=-1), dict(n_max=-1), dict(max_points_dropout=1.5), dict(cell_x=0.0),
                                  dict(range_y=float("nan")), dict(vmin=4.0)])
def test_refused_configurations(over):
    from liso_amd import _lib

    cfg = _cfg(**over)
    assert _lib.lib().liso_snippet_augment_batch_workspace_bytes(ctypes.byref(cfg)) == 0
    assert _call(cfg, workspace_bytes=1 << 30) == EINVAL


@pytest.mark.parametrize("name", [p for p in POINTERS if p not in OPTIONAL])
def test_null_tables_are_refused(name):
    assert _call(_cfg(), **{name: True}) == EINVAL


def test_optional_pointers_and_the_raydrop_rows():
    # with every optional pointer null the call gets as far as the workspace check
    cfg = _cfg()
    assert _call(cfg, workspace_bytes=0, db_lidar_rows=True, extra_flow=True, kept_rows=True) == EWORKSPACE
    assert _call(_cfg(selection=2), workspace_bytes=0, db_lidar_rows=True) == EINVAL  # the ray-drop reads the LiDAR rows
    assert _call(_cfg(n_max=0), workspace_bytes=0, pillar_coors=True) == EWORKSPACE    # no rows, no coordinates needed


def test_free_mask_batch_and_append_check_their_arguments():
    from liso_amd import _lib

    lib = _lib.lib()
    p = ctypes.c_void_p(FAKE)
    assert lib.liso_bev_free_mask_batch(p, p, 0, 10, 64, 64, 4, p, p, p, 1 << 20, None) == EINVAL
    assert lib.liso_bev_free_mask_batch(p, None, 2, 10, 64, 64, 4, p, p, p, 1 << 20, None) == EINVAL
    assert lib.liso_bev_free_mask_batch(p, p, 2, 10, 64, 64, 4, None, p, p, 1 << 20, None) == EINVAL
    assert lib.liso_bev_free_mask_batch(p, p, 2, 10, 64, 64, 4, p, p, p, 2 * 64 * 64 - 1, None) == EWORKSPACE
    assert lib.liso_cloud_append_batch(p, p, p, p, 0, 10, 5, 4, p, p, None) == EINVAL
    assert lib.liso_cloud_append_batch(p, p, p, p, 2, 10, 5, 0, p, p, None) == EINVAL
    assert lib.liso_cloud_append_batch(None, p, p, p, 2, 10, 5, 4, p, p, None) == EINVAL
    assert lib.liso_cloud_append_batch(p, p, p, p, 2, 10, 5, 4, p, None, None) == EINVAL
