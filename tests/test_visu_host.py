"""CPU: the host statements of the summary pictures (liso_amd/visu) against their fixtures, the colour tables against matplotlib,
the C ABI and the alias package."""
import os

import numpy as np
import pytest

from tests import visu_cases as VC


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def test_line_walk_equals_skimage_bit_for_bit(golden_dir):
    from liso_amd.visu.bbox_image import line_aa

    g = np.load(os.path.join(golden_dir, "visu_line_aa.npz"))
    lines, off = g["lines"], g["offsets"]
    assert len(lines) >= 150
    kinds = {"zero": 0, "horizontal": 0, "vertical": 0, "diagonal": 0, "negative": 0}
    for i, (r0, c0, r1, c1) in enumerate(lines):
        rows, cols, w = line_aa(r0, c0, r1, c1)
        sl = slice(off[i], off[i + 1])
        assert np.array_equal(rows, g["rows"][sl]) and np.array_equal(cols, g["cols"][sl]), (r0, c0, r1, c1)
        assert np.array_equal(_bits(w), _bits(g["weights"][sl])), (r0, c0, r1, c1)
        kinds["zero"] += (r0, c0) == (r1, c1)
        kinds["horizontal"] += r0 == r1 and c0 != c1
        kinds["vertical"] += c0 == c1 and r0 != r1
        kinds["diagonal"] += abs(r0 - r1) == abs(c0 - c1) != 0
        kinds["negative"] += min(r0, c0, r1, c1) < 0
    assert all(v >= 2 for v in kinds.values()), kinds


def test_line_entries_stay_within_the_kernel_bound():
    """the drawing kernel sizes a line's entry list as 3 * (max(dr, dc) + 1)"""
    from liso_amd.visu.bbox_image import line_aa

    rng = np.random.default_rng(0)
    for r0, c0, r1, c1 in rng.integers(-300, 600, (400, 4)):
        assert len(line_aa(r0, c0, r1, c1)[0]) <= 3 * (max(abs(r0 - r1), abs(c0 - c1)) + 1)


@pytest.mark.parametrize("name", ["summer", "gist_rainbow"])
def test_colour_tables_equal_matplotlib(name):
    matplotlib = pytest.importorskip("matplotlib")
    from liso_amd.visu import colormaps

    ref = matplotlib.colormaps[name]
    fn = getattr(colormaps, name)
    x = np.concatenate([np.random.default_rng(1).random(1000), [0.0, 1.0, np.nan]])
    for dtype in (np.float64, np.float32):
        assert np.array_equal(fn(x.astype(dtype)), ref(x.astype(dtype))[..., :3])
    assert np.array_equal(getattr(colormaps, name + "_table")(), ref(np.arange(256))[..., :3])
    i = np.arange(256) / 255.0
    if name == "summer":
        assert np.allclose(colormaps.summer_table(), np.stack([i, 0.5 + 0.5 * i, np.full(256, 0.4)], -1), rtol=0, atol=1e-15)


def test_abi_symbols_reachable():
    from liso_amd import _lib

    lib = _lib.lib()
    names = [n for n in _lib.SIGNATURES if n.startswith("liso_visu_")]
    assert len(names) == 8
    for n in names:
        assert getattr(lib, n).argtypes == _lib.SIGNATURES[n][1]
    # argument checks come before any launch
    assert lib.liso_visu_lines_workspace_bytes(2, 24, 40, 160) > 2 * 24 * 40 * 4
    assert lib.liso_visu_lines_workspace_bytes(2, 24, 40, -1) == 0
    assert lib.liso_visu_draw_lines_f32(1, 24, 40, 2, 5, 1, 0, 160, None, None, None, None, None, None, 0, None) == -1  # two channels
    assert lib.liso_visu_draw_lines_f32(1, 24, 40, 3, 7, 5, 1, 160, None, None, None, None, None, None, 0, None) == -1  # 7 lines in groups of 5
    assert lib.liso_visu_draw_lines_f32(1, 24, 40, 3, 0, 5, 1, 160, None, None, None, None, None, None, 0, None) == 0  # nothing to draw
    assert lib.liso_visu_flow_wheel_f32(0, 8, 12, None, None, None, None) == 0
    assert lib.liso_visu_flow_wheel_f32(1, 8, 12, None, None, None, None) == -1
    assert lib.liso_visu_box_corners_bev(1, 4, 24, 40, 3, None, 0, 0.0, 0.0, None, None, None, None, None) == -1  # range form 3
    assert lib.liso_visu_topdown_f32(1, 10, 4, 16, 24, None, None, None, None, None, None, 0, None) == -1


def test_install_as_resolves_visu():
    import liso_amd

    liso_amd.install_as("liso")
    import liso.visu.bbox_image
    import liso.visu.color_conversion
    import liso.visu.flow_image
    import liso.visu.pcl_image
    from liso.visu.bbox_image import draw_box_onto_image

    from liso_amd.visu import bbox_image

    assert draw_box_onto_image is bbox_image.draw_box_onto_image and liso.visu.pcl_image.create_occupancy_pcl_image is not None


def test_overflow_rule_and_reference_smear():
    from liso_amd.visu import bbox_image as BI

    far = ((5, 5), (8, VC.W - 1 + VC.REACH + 1))  # one column beyond the default reach
    near = ((5, 5), (8, VC.W - 1 + VC.REACH))
    base = np.random.default_rng(0).random((VC.H, VC.W, 3)).astype(np.float32)
    color = np.array([1.0, 0.5, 0.25], np.float32)
    img = base.copy()
    assert BI.draw_line_on_image(img, *far, color) == 1 and np.array_equal(img, base)  # skipped and counted
    assert BI.draw_line_on_image(img, *near, color) == 0 and not np.array_equal(img, base)
    # max_reach=None walks the far line in full: its tail is clipped onto the right border, rows 5..8, last entry wins
    img = base.copy()
    assert BI.draw_line_on_image(img, *far, color, max_reach=None) == 0
    changed = np.argwhere((img != base).any(-1))
    assert (changed[:, 1] == VC.W - 1).sum() >= 3 and changed[:, 0].min() >= 4 and changed[:, 0].max() <= 9
    rows, cols, w = BI.line_aa(*far[0], *far[1])
    last = np.flatnonzero((rows == 8) & (cols >= VC.W - 1))[-1]
    expect = ((1.0 - w[last]) * base[8, VC.W - 1].astype(np.float64) + w[last] * color.astype(np.float64)).astype(np.float32)
    assert np.array_equal(_bits(img[8, VC.W - 1]), _bits(expect))
    # the engine counts per image
    canvas, ends, valid, colors = VC.line_scene(40, 3)
    assert BI.draw_lines_host(canvas.copy(), ends, valid, colors).tolist() == [2, 0, 0]
    assert BI.draw_lines_host(canvas.copy(), ends, valid, colors, max_reach=None).tolist() == [0, 0, 0]


def test_line_rules_on_the_host():
    """every pixel reads the canvas before its line; the second of two equal lines blends over the first"""
    from liso_amd.visu import bbox_image as BI

    img = np.zeros((VC.H, VC.W, 1), np.float32)
    one = np.ones(1)
    BI.draw_line_on_image(img, (4, 10), (15, 33), one)
    first = img.copy()
    rows, cols, w = BI.line_aa(4, 10, 15, 33)
    assert np.array_equal(first[rows, cols, 0], w.astype(np.float32))  # no pixel is hit twice inside the canvas
    BI.draw_line_on_image(img, (4, 10), (15, 33), one)
    again = ((1.0 - w) * first[rows, cols, 0].astype(np.float64) + w).astype(np.float32)
    assert np.array_equal(_bits(img[rows, cols, 0]), _bits(again)) and not np.array_equal(img, first)
    # closed polygons equal their edges drawn one by one, in order
    poly = np.array([[[2, 3], [20, 30], [-5, 12], [10, 44], [7, 7]]])
    a = np.random.default_rng(1).random((VC.H, VC.W, 3)).astype(np.float32)
    b = a.copy()
    BI.draw_connected_lines_on_image(poly, a, np.array([[0.1, 0.9, 0.3]]))
    for i in range(5):
        BI.draw_line_on_image(b, poly[0, i], poly[0, (i + 1) % 5], np.array([0.1, 0.9, 0.3]))
    assert np.array_equal(_bits(a), _bits(b))


def test_flow_wheel_host_edges():
    from liso_amd.visu import flow_image as FI
    from liso_amd.visu.color_conversion import hsv2rgb

    import torch

    flow = VC.flow_cases()
    rgb = FI.pytorch_create_flow_image(flow)
    assert rgb.dtype == np.float32 and not np.isnan(rgb).any()
    assert (rgb[0, 0] == 1.0).all() and (rgb[0, 1:] == 0.0).all()  # all-zero flow: value 1, full red
    assert rgb[2, 0, 0, 6] > 0.0 and (rgb[2, 1:, 0, 6] == 0.0).all()  # -1e-7 rad: hue exactly 1, sector 6 % 6 = 0
    assert np.abs(rgb - VC.flow_wheel_fp64(flow)).max() < 2e-6
    # the tensor form of hsv2rgb states the same arithmetic
    hsv = np.random.default_rng(2).random((2, 3, 5, 7)).astype(np.float32)
    hsv[0, 0, 0, :3] = (0.0, 1.0, 0.5)
    assert np.array_equal(_bits(hsv2rgb(torch.from_numpy(hsv)).numpy()), _bits(hsv2rgb(hsv)))

    class Rec:
        def add_images(self, tag, array, global_step=None, dataformats=None):
            self.got = (tag, array.shape, global_step, dataformats)

    rec = Rec()
    FI.log_flow_image(rec, VC.cfg(2), 5, flow, suffix="x")
    assert rec.got == ("DATA/FLOW_T0_T1/x", (2, 3, 8, 12), 5, "NCHW")


def test_pillar_coordinates_and_projection_host():
    from liso_amd.visu import pcl_image as PI

    import torch

    pts, _ = VC.occupancy_points()
    rc = PI.pillarize_pointcloud(pts[0], np.array(VC.RANGE2), np.array([VC.H, VC.W]))
    assert rc.dtype == np.int32 and rc.min() >= 0 and rc[:, 0].max() <= VC.H - 1 and rc[:, 1].max() <= VC.W - 1
    assert rc[3].tolist() == [0, 0] and rc[5].tolist() == [0, 0] and rc[6].tolist() == [VC.H - 1, VC.W - 1]
    ok = np.isfinite(pts).all(-1)
    _, trc = PI.torch_batched_pillarize_pointcloud(torch.from_numpy(pts.astype(np.float64)), torch.tensor(VC.RANGE2, dtype=torch.float64),
                                                   torch.tensor([VC.H, VC.W]))
    assert np.array_equal(trc[0].numpy()[ok[0]], rc[ok[0]])
    # both axes take the smaller factor
    p = np.array([[0.0, 0.0], [3.5, 8.5]], np.float32)
    out = PI.project_2d_pcl_to_rowcol_nonsquare_bev_range(p, VC.TD_MIN, VC.TD_MAX, VC.TD_GRID)
    f = np.float32(24.0) / np.float32(14.0)
    assert np.array_equal(out, (p - VC.TD_MIN) * f)
    t = PI.project_2d_pcl_to_rowcol_nonsquare_bev_range(torch.from_numpy(p), torch.from_numpy(VC.TD_MIN), torch.from_numpy(VC.TD_MAX),
                                                        torch.tensor(VC.TD_GRID))
    assert np.array_equal(t.numpy(), out)


def test_box_colors_host_branches():
    from liso_amd.visu import bbox_image as BI, colormaps

    table = colormaps.summer_table()
    sc = np.array([[0.2, 0.8, 0.5, 0.9]], np.float32)
    valid = np.array([[True, True, True, False]])
    c = BI.box_colors_host(sc, valid)
    assert np.array_equal(c[0, 0], table[0]) and np.array_equal(c[0, 1], table[255])
    t = (sc[0, 2] - sc[0, 0]) / (sc[0, 1] - sc[0, 0])
    assert np.array_equal(c[0, 2], table[int(t * np.float32(256))]) and t.dtype == np.float32
    assert np.array_equal(BI.box_colors_host(np.full((1, 4), 0.3, np.float32), valid)[0, :3], np.broadcast_to(table[255], (3, 3)))
    assert np.array_equal(BI.box_colors_host(sc, np.zeros_like(valid), "attribute"), np.broadcast_to(table[128], (1, 4, 3)))
    assert np.array_equal(BI.box_colors_host(np.full((1, 4), 0.3, np.float32), valid, "attribute")[0, :3], np.broadcast_to(table[0], (3, 3)))


# ---- the host statements against what the reference's own functions made of the same inputs (scripts/make_visu_golden.py) ----------
@pytest.fixture(scope="module")
def ref(golden_dir):
    return np.load(os.path.join(golden_dir, "visu_reference.npz"))


def _filled(base, idx, val):
    out = base.copy()
    out.ravel()[idx] = val
    return out


def _np_shape(d):
    from liso_amd.kabsch.shape_utils import Shape

    return Shape(**{k: v.copy() for k, v in d.items()})


def test_reference_flow_wheel(ref):
    from liso_amd.visu.flow_image import pytorch_create_flow_image

    got = pytorch_create_flow_image(VC.flow_cases())
    assert got.shape == ref["flow_rgb"].shape and np.abs(got - ref["flow_rgb"]).max() <= 1e-6  # fp32 atan2 on both sides
    assert np.array_equal(got[:2], ref["flow_rgb"][:2])  # nothing trigonometric decides the first two images


def test_reference_topdown_and_occupancy(ref):
    from liso_amd.visu import pcl_image as PI

    pcl, inten = VC.topdown_clouds()
    img, occ = PI.create_topdown_f32_pcl_image_variable_extent(pcl, inten, VC.TD_MIN, VC.TD_MAX, VC.TD_GRID)
    for b in range(2):
        assert np.array_equal(occ[b], ref[f"topdown_occ_{b}"]) and np.array_equal(_bits(img[b]), _bits(ref[f"topdown_img_{b}"])), b
    one = PI.create_topdown_f32_pcl_image_variable_extent(pcl[0], inten[0], VC.TD_MIN, VC.TD_MAX, VC.TD_GRID)
    assert np.array_equal(_bits(one[0]), _bits(ref["topdown_img_0"])) and occ.sum() > 200
    pts, valid = VC.occupancy_points()
    for b in range(2):
        rows = valid[b] & np.isfinite(pts[b]).all(-1)
        assert np.array_equal(PI.create_occupancy_pcl_image(pts[b], np.array(VC.RANGE2), (VC.H, VC.W), rows), ref[f"occupancy_{b}"])


def test_reference_corners_and_boxes_on_canvases(ref):
    from liso_amd.visu import bbox_image as BI

    boxes = VC.box_set(np.float32)
    corners = BI.get_box_corners_in_sensor_coordinates(_np_shape(boxes))
    ok = boxes["valid"]
    assert corners.dtype == np.float32 and np.abs(corners[ok] - ref["corners_sensor"][ok]).max() <= 1e-6
    canvas = np.random.default_rng(8).random((2, VC.H, VC.W, 3)).astype(np.float32)
    per_box = np.random.default_rng(9).random((2, 9, 3)).astype(np.float32)
    for form in (2, 4):
        rng = VC.RANGE2 if form == 2 else np.array(VC.RANGE4, np.float32)
        for name, color in (("triple", np.array([0.2, 0.9, 0.4], np.float32)), ("per_box", per_box), ("confidence", "confidence")):
            got = BI.draw_box_onto_image(_np_shape(boxes), canvas.copy(), rng, color, max_reach=None)
            want = _filled(canvas, ref[f"onto_{form}_{name}_idx"], ref[f"onto_{form}_{name}_val"])
            assert np.array_equal(_bits(got), _bits(want)), (form, name)
            assert len(ref[f"onto_{form}_{name}_idx"]) > 1000


def test_reference_draw_box_image_four_layers(ref):
    from liso_amd.visu import bbox_image as BI
    boxes = VC.box_set(np.float32)
    gray = np.random.default_rng(4).random((2, 1, VC.H, VC.W)).astype(np.float32)
    layers = {"pred_boxes": boxes, "gt_boxes": VC.shifted(boxes, 1), "gt_background_boxes": VC.shifted(boxes, 2), "gt_boxes_prev": VC.shifted(boxes, 3)}
    got = BI.draw_box_image(cfg=VC.cfg(), canvas_f32=gray, max_reach=None, **{k: _np_shape(v) for k, v in layers.items()})
    base = np.ascontiguousarray(np.repeat(np.transpose(gray, (0, 2, 3, 1)), 3, axis=-1))
    assert np.array_equal(_bits(got), _bits(_filled(base, ref["box_image_idx"], ref["box_image_val"])))
