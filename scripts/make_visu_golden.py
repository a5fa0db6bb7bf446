"""Writes the fixtures of the summary pictures under tests/golden/.  Run by hand, never by a test; plain arrays only.

    <python with scikit-image> scripts/make_visu_golden.py lines
        -> visu_line_aa.npz: skimage.draw.line_aa's rows, columns and weights for ~200 integer lines, concatenated with offsets.
           Needs numpy and scikit-image only (this package is not imported).
    python scripts/make_visu_golden.py reference <path of the reference tree>
        -> visu_reference.npz: small inputs and what the reference's own liso.visu functions make of them.  The reference is
           imported from its tree with stubs for the third-party modules that are absent;
           skimage.draw.line_aa is this package's restatement, which the first fixture pins.
"""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def line_cases():
    """[n, 4] integer (r0, c0, r1, c1)"""
    cases = [(5, 7, 5, 7), (-3, -3, -3, -3)]  # zero length
    for a, b in ((3, 4), (4, 3)):  # each direction
        cases += [(10, a, 10, 20 + b), (10, 20 + b, 10, a)]  # horizontal
        cases += [(a, 10, 20 + b, 10), (20 + b, 10, a, 10)]  # vertical
        cases += [(a, a, a + 17, a + 17), (a + 17, a + 17, a, a), (a, a + 17, a + 17, a), (a + 17, a, a, a + 17)]  # exact diagonals
    for n in (1, 2, 3, 8, 25, 60, 131):  # |slope| just under and just over 1, every sign
        for sr in (1, -1):
            for sc in (1, -1):
                cases += [(0, 0, sr * n, sc * (n + 1)), (0, 0, sr * (n + 1), sc * n)]
    for n in (2, 5, 11, 40, 97):  # steep and shallow
        for k in (1, 3, 7):
            cases += [(2, 3, 2 + n * k, 3 + n), (2, 3, 2 + n, 3 + n * k), (2 + n, 3 + n * k, 2, 3), (2, 3 + n, 2 + n * k, 3)]
    cases += [(-40, -12, 30, 9), (12, -35, -8, 290), (-1, -1, -30, -2), (299, -40, -40, 299), (-7, 100, 0, 0)]  # negative coordinates
    rng = np.random.default_rng(20240611)
    cases += [tuple(int(v) for v in rng.integers(-40, 300, 4)) for _ in range(30)]
    return np.array(cases, np.int64)


def make_lines():
    from skimage.draw import line_aa

    cases = line_cases()
    rows, cols, weights, offsets = [], [], [], [0]
    for r0, c0, r1, c1 in cases:
        rr, cc, ww = line_aa(int(r0), int(c0), int(r1), int(c1))
        rows.append(rr.astype(np.int64)), cols.append(cc.astype(np.int64)), weights.append(ww.astype(np.float64))
        offsets.append(offsets[-1] + len(rr))
    path = os.path.join(GOLDEN, "visu_line_aa.npz")
    np.savez_compressed(path, lines=cases, offsets=np.array(offsets, np.int64), rows=np.concatenate(rows), cols=np.concatenate(cols),
                        weights=np.concatenate(weights))
    print(path, len(cases), "lines", offsets[-1], "entries", os.path.getsize(path), "bytes")


def sparse(out, base):
    """the values of `out` that differ from `base` bit for bit: (flat indices int32, values fp32)"""
    idx = np.flatnonzero(np.ascontiguousarray(out).view(np.uint32).ravel() != np.ascontiguousarray(base).view(np.uint32).ravel())
    return idx.astype(np.int32), out.ravel()[idx].astype(np.float32)


def make_reference(ref_root):
    """imports the reference's liso.visu from its tree and records what it makes of tests/visu_cases.py's inputs"""
    from unittest.mock import MagicMock

    import torch

    sys.dont_write_bytecode = True
    sys.path.insert(0, ROOT)
    from liso_amd.visu.bbox_image import line_aa
    from tests import visu_cases as VC

    for name in ("torchvision", "torchvision.utils", "shapely", "shapely.affinity", "shapely.geometry", "iou3d_nms_cuda", "skimage", "skimage.draw",
                 "pynanoflann", "cv2", "tensorboard", "torch.utils.tensorboard"):
        sys.modules.setdefault(name, MagicMock())
    sys.modules["skimage.draw"].line_aa = line_aa
    for k in [k for k in sys.modules if k == "liso" or k.startswith("liso.")]:
        del sys.modules[k]
    sys.path.insert(0, ref_root)
    from liso.kabsch.shape_utils import Shape as RefShape
    from liso.visu import bbox_image as RB, flow_image as RF, pcl_image as RP

    def ref_shape(d):
        return RefShape(**{k: torch.from_numpy(v.copy()) for k, v in d.items()})

    class Cfg(dict):
        __getattr__ = dict.__getitem__

    cfg = Cfg(logging=Cfg(max_log_img_batches=4), data=Cfg(bev_range_m=VC.RANGE2), nms_iou_threshold=0.1)
    out = {}
    with torch.no_grad():
        out["flow_rgb"] = RF.pytorch_create_flow_image(torch.from_numpy(VC.flow_cases())).numpy()
        pcl, inten = VC.topdown_clouds()
        for b, n in ((0, 300), (1, 260)):  # (the reference takes one cloud without padding rows)
            img, occ = RP.create_topdown_f32_pcl_image_variable_extent(torch.from_numpy(pcl[b, :n]), torch.from_numpy(inten[b, :n]),
                                                                       torch.from_numpy(VC.TD_MIN), torch.from_numpy(VC.TD_MAX), torch.tensor(VC.TD_GRID))
            out[f"topdown_img_{b}"], out[f"topdown_occ_{b}"] = img.numpy(), occ.numpy()
        pts, valid = VC.occupancy_points()
        for b in range(2):
            rows = pts[b][valid[b] & np.isfinite(pts[b]).all(-1)]
            out[f"occupancy_{b}"] = RP.create_occupancy_pcl_image(rows, np.array(VC.RANGE2), np.array([VC.H, VC.W]))
        boxes = VC.box_set(np.float32)
        out["corners_sensor"] = RB.get_box_corners_in_sensor_coordinates(ref_shape(boxes)).numpy()
        canvas = np.random.default_rng(8).random((2, VC.H, VC.W, 3)).astype(np.float32)
        per_box = np.random.default_rng(9).random((2, 9, 3)).astype(np.float32)
        for form in (2, 4):
            rng = VC.RANGE2 if form == 2 else torch.tensor(VC.RANGE4)
            for name, color in (("triple", np.array([0.2, 0.9, 0.4], np.float32)), ("per_box", per_box), ("confidence", "confidence")):
                got = RB.draw_box_onto_image(ref_shape(boxes), canvas.copy(), rng, color)
                out[f"onto_{form}_{name}_idx"], out[f"onto_{form}_{name}_val"] = sparse(got, canvas)
        gray = np.random.default_rng(4).random((2, 1, VC.H, VC.W)).astype(np.float32)
        layers = {"pred_boxes": boxes, "gt_boxes": VC.shifted(boxes, 1), "gt_background_boxes": VC.shifted(boxes, 2), "gt_boxes_prev": VC.shifted(boxes, 3)}
        got = RB.draw_box_image(cfg=cfg, canvas_f32=torch.from_numpy(gray), **{k: ref_shape(v) for k, v in layers.items()})
        out["box_image_idx"], out["box_image_val"] = sparse(got.astype(np.float32), np.repeat(np.transpose(gray, (0, 2, 3, 1)), 3, axis=-1))
    path = os.path.join(GOLDEN, "visu_reference.npz")
    np.savez_compressed(path, **out)
    print(path, {k: v.shape for k, v in out.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "lines":
        make_lines()
    elif len(sys.argv) >= 3 and sys.argv[1] == "reference":
        make_reference(sys.argv[2])
    else:
        sys.exit(__doc__)
