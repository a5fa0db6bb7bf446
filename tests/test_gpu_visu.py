"""GPU: the summary pictures on the device (include/liso_visu.h) against the numpy host statements of liso_amd/visu, bit for bit
wherever only integers or fp64-rounded-once values are involved."""
import numpy as np
import pytest
import torch

from tests import visu_cases as VC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _shape(d, dev=None):
    from liso_amd.kabsch.shape_utils import Shape

    d = {k: v.copy() for k, v in d.items()}
    if dev is not None:
        d = {k: torch.from_numpy(v).to(dev) for k, v in d.items()}
    return Shape(**d)


cfg = VC.cfg


# ---- line drawing -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [3, 1, 4])
@pytest.mark.parametrize("n_lines", [40, 1, 63, 64, 65])
def test_lines_bit_equal(dev, n_lines, channels):
    from liso_amd.visu import bbox_image as BI

    canvas, ends, valid, colors = VC.line_scene(n_lines, channels)
    host = canvas.copy()
    skipped = BI.draw_lines_host(host, ends, valid, colors)
    d_canvas = torch.from_numpy(canvas).to(dev)
    overflow = torch.zeros(3, dtype=torch.int32, device=dev)
    out = BI.draw_lines(d_canvas, torch.from_numpy(ends).to(dev), torch.from_numpy(valid).to(dev), torch.from_numpy(colors).to(dev),
                        overflow=overflow)
    assert out.data_ptr() == d_canvas.data_ptr()
    got = out.cpu().numpy()
    assert np.array_equal(overflow.cpu().numpy(), skipped)
    if n_lines == 40:
        assert skipped[0] == 2  # the two lines beyond the reach
        assert not np.array_equal(_bits(host[0]), _bits(canvas[0]))
    assert np.array_equal(_bits(got[2]), _bits(canvas[2])), "an image without a valid line must come back bit-identical"
    assert np.array_equal(_bits(got), _bits(host))


def test_lines_closed_polygons_equal_explicit_endpoints(dev):
    from liso_amd.visu import bbox_image as BI

    rng = np.random.default_rng(2)
    corners = np.stack([rng.integers(-6, VC.H + 6, (2, 15)), rng.integers(-6, VC.W + 6, (2, 15))], -1).astype(np.int32)  # 3 polygons of 5
    ends = np.stack([corners, np.roll(corners.reshape(2, 3, 5, 2), -1, axis=2).reshape(2, 15, 2)], axis=2)
    valid = np.array([[True, False, True], [True, True, True]])
    colors = rng.random((2, 3, 3))
    canvas = rng.random((2, VC.H, VC.W, 3)).astype(np.float32)
    a = BI.draw_lines(torch.from_numpy(canvas).to(dev), torch.from_numpy(ends).to(dev), torch.from_numpy(valid).to(dev),
                      torch.from_numpy(colors).to(dev), group=5).cpu().numpy()
    b = BI.draw_lines(torch.from_numpy(canvas).to(dev), torch.from_numpy(corners).to(dev), torch.from_numpy(valid).to(dev),
                      torch.from_numpy(colors).to(dev), group=5, closed=True).cpu().numpy()
    host = canvas.copy()
    BI.draw_lines_host(host, corners, valid, colors, group=5, closed=True)
    assert np.array_equal(_bits(a), _bits(host)) and np.array_equal(_bits(b), _bits(host))


# ---- box corners --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("form", [2, 4])
@pytest.mark.parametrize("clamp", [None, (0.3, 15.0)])
def test_box_corners_equal_as_integers(dev, dtype, form, clamp):
    from liso_amd.visu import bbox_image as BI

    boxes = VC.box_set(dtype)
    rng_arg = VC.RANGE2 if form == 2 else np.array(VC.RANGE4, np.float32)
    values = VC.corner_values_fp64(boxes["pos"], boxes["dims"], boxes["rot"], form, clamp)
    margin = VC.edge_margin(values, form)
    finite = np.isfinite(values).all(axis=(-1, -2))
    assert finite.sum() == 17 and not finite[0, 8]
    assert margin[finite].min() >= VC.MARGIN, margin[finite].min()  # every corner of every finite slot
    host = BI.box_corner_rowcol(_shape(boxes), (VC.H, VC.W), rng_arg, clamp)
    expect = np.rint(values[finite]) if form == 2 else np.trunc(values[finite])
    assert np.array_equal(host[finite], expect.astype(np.int32))
    d_rng = rng_arg if form == 2 else torch.from_numpy(rng_arg).to(dev)
    got = BI.box_corner_rowcol(_shape(boxes, dev), (VC.H, VC.W), d_rng, clamp).cpu().numpy()
    assert got.dtype == np.int32 and got.shape == (2, 9, 5, 2)
    assert np.array_equal(got, host)
    assert (got[0, 8] == -(1 << 31)).all()  # the NaN slot


# ---- boxes onto canvases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [2, 4])
@pytest.mark.parametrize("color", ["triple", "per_box", "confidence"])
def test_draw_box_onto_image_bit_equal(dev, form, color):
    from liso_amd.visu import bbox_image as BI

    boxes = VC.box_set(np.float32)
    rng = np.random.default_rng(8)
    canvas = rng.random((2, VC.H, VC.W, 3)).astype(np.float32)
    col = {"triple": np.array([0.2, 0.9, 0.4], np.float32), "per_box": rng.random((2, 9, 3)).astype(np.float32), "confidence": "confidence"}[color]
    rng_arg = VC.RANGE2 if form == 2 else np.array(VC.RANGE4, np.float32)
    host_skipped = np.zeros(2, np.int32)
    host = BI.draw_box_onto_image(_shape(boxes), canvas.copy(), rng_arg, col, overflow=host_skipped)
    overflow = torch.zeros(2, dtype=torch.int32, device=dev)
    got = BI.draw_box_onto_image(_shape(boxes, dev), torch.from_numpy(canvas).to(dev), rng_arg if form == 2 else torch.from_numpy(rng_arg).to(dev),
                                 col, overflow=overflow).cpu().numpy()
    assert not np.array_equal(_bits(host), _bits(canvas))
    assert np.array_equal(_bits(got), _bits(host))
    assert np.array_equal(overflow.cpu().numpy(), host_skipped)


def test_confidence_degenerate_cases(dev):
    from liso_amd.visu import bbox_image as BI, colormaps

    boxes = VC.box_set(np.float32)
    top = colormaps.summer_table()[255]
    canvas = np.random.default_rng(9).random((2, VC.H, VC.W, 3)).astype(np.float32)
    # all probabilities equal; a single valid box; none valid
    equal = dict(boxes, probs=np.full_like(boxes["probs"], 0.37))
    single = dict(boxes, valid=np.zeros((2, 9), bool))
    single["valid"][0, 2] = single["valid"][1, 4] = True
    none = dict(boxes, valid=np.zeros((2, 9), bool))
    for case in (equal, single):
        colors = BI.box_colors(torch.from_numpy(case["probs"][..., 0]).to(dev), torch.from_numpy(case["valid"]).to(dev)).cpu().numpy()
        assert np.array_equal(colors[case["valid"]], np.broadcast_to(top, colors[case["valid"]].shape))
        assert np.array_equal(colors[case["valid"]], BI.box_colors_host(case["probs"][..., 0], case["valid"])[case["valid"]])
        host = BI.draw_box_onto_image(_shape(case), canvas.copy(), VC.RANGE2, "confidence")
        got = BI.draw_box_onto_image(_shape(case, dev), torch.from_numpy(canvas).to(dev), VC.RANGE2, "confidence").cpu().numpy()
        assert np.array_equal(_bits(got), _bits(host)) and not np.array_equal(_bits(got), _bits(canvas))
    got = BI.draw_box_onto_image(_shape(none, dev), torch.from_numpy(canvas).to(dev), VC.RANGE2, "confidence").cpu().numpy()
    assert np.array_equal(_bits(got), _bits(canvas))
    # the attribute colouring's own branches: spread floored at 1e-6, an image without a valid box takes 0.5
    sc = np.random.default_rng(3).normal(size=(2, 9)).astype(np.float32)
    sc[1] = 2.5
    valid = boxes["valid"].copy()
    for v in (valid, np.zeros_like(valid)):
        a = BI.box_colors(torch.from_numpy(sc).to(dev), torch.from_numpy(v).to(dev), "attribute").cpu().numpy()
        assert np.array_equal(a, BI.box_colors_host(sc, v, "attribute"))
    assert np.array_equal(a, np.broadcast_to(colormaps.summer_table()[128], a.shape))


def _layers(dev=None):
    base = VC.box_set(np.float32)
    return {"pred_boxes": _shape(base, dev), "gt_boxes": _shape(VC.shifted(base, 1), dev), "gt_background_boxes": _shape(VC.shifted(base, 2), dev),
            "gt_boxes_prev": _shape(VC.shifted(base, 3), dev)}


def test_draw_box_image_four_layers_bit_equal(dev):
    from liso_amd.visu import bbox_image as BI

    gray = np.random.default_rng(4).random((2, 1, VC.H, VC.W)).astype(np.float32)
    # (the shifted layers promise no rounding margin: host and device draw from the device's corner tables, checked above)
    host_layers, dev_layers = _layers(), _layers(dev)
    host = BI.draw_box_image(cfg=cfg(), canvas_f32=gray, **host_layers)
    got = BI.draw_box_image(cfg=cfg(), canvas_f32=torch.from_numpy(gray).to(dev), **dev_layers)
    assert tuple(got.shape) == (2, VC.H, VC.W, 3) and got.dtype == torch.float32
    tables_agree = all(np.array_equal(BI.box_corner_rowcol(dev_layers[k], (VC.H, VC.W), VC.RANGE2, c).cpu().numpy(),
                                      BI.box_corner_rowcol(host_layers[k], (VC.H, VC.W), VC.RANGE2, c))
                       for k, c in (("pred_boxes", BI.DIMS_CLAMP_M), ("gt_boxes", None), ("gt_background_boxes", None), ("gt_boxes_prev", None)))
    assert tables_agree, "cos / sin moved a corner of the unpinned layers across a rounding edge: choose other shifts"
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(host))
    # the slice: one image only
    one = BI.draw_box_image(cfg=cfg(1), canvas_f32=torch.from_numpy(gray).to(dev), **dev_layers)
    assert tuple(one.shape) == (1, VC.H, VC.W, 3) and np.array_equal(_bits(one.cpu().numpy()), _bits(host[:1]))
    # with the NMS: the device's survivors drawn by the host
    from liso_amd.utils.nms_iou import perform_nms_on_shapes_padded

    got = BI.draw_box_image(cfg=cfg(), canvas_f32=torch.from_numpy(gray).to(dev), perform_nms=True, max_num_boxes=5, **dev_layers)
    preds = dev_layers["pred_boxes"].clone()
    preds.dims = torch.clamp(preds.dims, min=0.3, max=15.0)
    kept = perform_nms_on_shapes_padded(preds, max_num_boxes=5, overlap_threshold=0.1, pre_nms_max_num_boxes=1000)
    assert int(kept.valid.sum()) <= 10
    host = BI.draw_box_image(cfg=cfg(), canvas_f32=gray, **dict(host_layers, pred_boxes=kept.numpy()))
    assert np.array_equal(BI.box_corner_rowcol(kept, (VC.H, VC.W), VC.RANGE2, BI.DIMS_CLAMP_M).cpu().numpy(),
                          BI.box_corner_rowcol(kept.numpy(), (VC.H, VC.W), VC.RANGE2, BI.DIMS_CLAMP_M))
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(host))


# ---- flow wheel ---------------------------------------------------------------------------------------------------------------------
def test_flow_wheel_against_fp64(dev):
    """measured on an MI355X: see DESIGN section 8"""
    from liso_amd.visu import flow_image as FI

    flow = VC.flow_cases()
    ref = VC.flow_wheel_fp64(flow)
    host = FI.pytorch_create_flow_image(flow)
    got = FI.pytorch_create_flow_image(torch.from_numpy(flow).to(dev)).cpu().numpy()
    assert got.shape == (3, 3, 8, 12) and got.dtype == np.float32
    assert not np.isnan(got).any() and not np.isnan(host).any()
    red = np.zeros((3, 8, 12), np.float32)
    red[0] = 1.0
    assert np.array_equal(got[0], red), "an all-zero flow image is full red"
    assert np.count_nonzero(got[1].sum(0)) == 1 and got[1][:, 3, 7].max() == 1.0
    assert got[2][0, 0, 6] > 0.0 and got[2][1, 0, 6] == 0.0 and got[2][2, 0, 6] == 0.0  # -1e-7 rad: hue 1.0, sector 6 % 6 = 0, red
    err_host, err_dev = np.abs(host - ref).max(), np.abs(got - ref).max()
    print(f"flow wheel max |error| against fp64: host {err_host:.3e} device {err_dev:.3e}")
    assert err_dev <= max(4.0 * err_host, 1e-6), (err_dev, err_host)


# ---- top-down and occupancy images --------------------------------------------------------------------------------------------------
def test_topdown_bit_equal(dev):
    from liso_amd.visu import pcl_image as PI

    pcl, inten = VC.topdown_clouds()
    h_img, h_occ = PI.create_topdown_f32_pcl_image_variable_extent(pcl, inten, VC.TD_MIN, VC.TD_MAX, VC.TD_GRID)
    lo, hi = torch.from_numpy(VC.TD_MIN).to(dev), torch.from_numpy(VC.TD_MAX).to(dev)
    d_img, d_occ = PI.create_topdown_f32_pcl_image_variable_extent(torch.from_numpy(pcl).to(dev), torch.from_numpy(inten).to(dev), lo, hi, VC.TD_GRID)
    assert d_occ.dtype == torch.bool and tuple(d_img.shape) == (2,) + VC.TD_GRID
    assert np.array_equal(d_occ.cpu().numpy(), h_occ) and np.array_equal(_bits(d_img.cpu().numpy()), _bits(h_img))
    # four points in one pixel: the highest index wins; cloud 0 is not rescaled, cloud 1 is
    f = np.float32(24.0 / 14.0)
    r, c = int((np.float32(1.35) + 4) * f), int((np.float32(2.25) + 5) * f)
    assert (r, c) == (9, 12)
    for b in range(2):
        inside, lin = PI.get_linear_bev_idx(pcl[b], VC.TD_MIN, VC.TD_MAX, VC.TD_GRID)
        on_pixel = np.flatnonzero(inside & (lin == r * VC.TD_GRID[1] + c))
        assert set(range(10, 14)) <= set(on_pixel.tolist())
        last = inten[b, on_pixel.max()]
        assert h_img[b, r, c] == (last if b == 0 else (last + np.float32(2.0)) / np.float32(7.0))
    # the 1 cm margin: of the eight edge points the four at 1.5 cm are in
    inside, _ = PI.get_linear_bev_idx(pcl[0], VC.TD_MIN, VC.TD_MAX, VC.TD_GRID)
    assert inside[20:28].tolist() == [False, True] * 4
    # unbatched
    u_img, u_occ = PI.create_topdown_f32_pcl_image_variable_extent(torch.from_numpy(pcl[0]).to(dev), torch.from_numpy(inten[0]).to(dev), lo, hi,
                                                                    VC.TD_GRID)
    assert np.array_equal(_bits(u_img.cpu().numpy()), _bits(h_img[0])) and np.array_equal(u_occ.cpu().numpy(), h_occ[0])


def test_occupancy_bit_equal(dev):
    from liso_amd.visu import pcl_image as PI

    pts, valid = VC.occupancy_points()
    rng = np.array(VC.RANGE2)
    host = PI.create_occupancy_pcl_image(pts, rng, (VC.H, VC.W), valid)
    got = PI.create_occupancy_pcl_image(torch.from_numpy(pts).to(dev), rng, (VC.H, VC.W), torch.from_numpy(valid).to(dev))
    assert tuple(got.shape) == (2, VC.H, VC.W, 1) and np.array_equal(got.cpu().numpy(), host)
    assert host[0, 0, 0, 0] == 1.0 and host[0, VC.H - 1, VC.W - 1, 0] == 1.0
    one = PI.create_occupancy_pcl_image(torch.from_numpy(pts[1]).to(dev), rng, (VC.H, VC.W))
    assert np.array_equal(one.cpu().numpy(), PI.create_occupancy_pcl_image(pts[1], rng, (VC.H, VC.W)))


# ---- no host read: the box-movement picture inside one captured graph ---------------------------------------------------------------
class _Recorder:
    def __init__(self):
        self.calls = []

    def add_images(self, tag, array, global_step=None, dataformats=None):
        self.calls.append((tag, array, global_step, dataformats))


def test_box_movement_in_one_graph(dev):
    from liso_amd.utils import graph_capture as GC
    from liso_amd.visu import bbox_image as BI

    layers = _layers(dev)
    gray = torch.from_numpy(np.random.default_rng(6).random((2, 1, VC.H, VC.W)).astype(np.float32)).to(dev)
    a = {"occupancy_f32_ta": gray, "gt": {"boxes": layers["gt_boxes"]}}
    b = {"occupancy_f32_ta": gray.flip(0).contiguous(), "gt": {"boxes": layers["gt_boxes_prev"]}}
    rec = _Recorder()

    def body():
        return BI.log_box_movement(cfg=cfg(), writer=rec, global_step=7, sample_data_a=a, sample_data_b=b, pred_boxes=layers["pred_boxes"],
                                   gt_background_boxes=layers["gt_background_boxes"], writer_prefix="val/")

    stream = torch.cuda.Stream(dev)
    graph, out = GC.capture(body, stream, warm_ups=2)
    assert rec.calls[-1][0] == "val/RECONSTRUCTION_TARGETS_t0_t1" and rec.calls[-1][2:] == (7, "NHWC")
    assert tuple(out.shape) == (2, 3 * VC.H, VC.W, 3)
    for seed in (21, 22):
        fresh = VC.shifted(VC.box_set(np.float32), seed)
        for k in ("pos", "rot"):  # refill the static box tensors
            getattr(layers["pred_boxes"], k).copy_(torch.from_numpy(fresh[k]))
            getattr(layers["gt_boxes"], k).copy_(torch.from_numpy(VC.shifted(fresh, seed + 10)[k]))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        replayed = out.cpu().numpy().copy()
        eager = body().cpu().numpy()
        assert np.array_equal(_bits(replayed), _bits(eager))


# ---- guard bands --------------------------------------------------------------------------------------------------------------------
def test_guard_bands_intact(dev):
    from liso_amd.visu import bbox_image as BI, flow_image as FI, pcl_image as PI
    from tests.guarded_alloc import guarded

    canvas, ends, valid, colors = VC.line_scene(65, 3)
    pcl, inten = VC.topdown_clouds()
    pts, pvalid = VC.occupancy_points()
    with guarded() as g:
        d_canvas = torch.empty((3, VC.H, VC.W, 3), dtype=torch.float32, device=dev)
        d_canvas.copy_(torch.from_numpy(canvas))
        BI.draw_lines(d_canvas, torch.from_numpy(ends).to(dev), torch.from_numpy(valid).to(dev), torch.from_numpy(colors).to(dev))
        img = torch.empty((2, VC.H, VC.W, 3), dtype=torch.float32, device=dev)
        img.copy_(torch.from_numpy(canvas[:2]))
        BI.draw_box_onto_image(_shape(VC.box_set(np.float32), dev), img, VC.RANGE2, "confidence")
        PI.create_topdown_f32_pcl_image_variable_extent(torch.from_numpy(pcl).to(dev), torch.from_numpy(inten).to(dev),
                                                        torch.from_numpy(VC.TD_MIN).to(dev), torch.from_numpy(VC.TD_MAX).to(dev), VC.TD_GRID)
        PI.create_occupancy_pcl_image(torch.from_numpy(pts).to(dev), np.array(VC.RANGE2), (VC.H, VC.W), torch.from_numpy(pvalid).to(dev))
        FI.pytorch_create_flow_image(torch.from_numpy(VC.flow_cases()).to(dev))
        assert g.check() >= 8
