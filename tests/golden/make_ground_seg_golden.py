"""Generates tests/golden/ground_seg_reference.npz from the reference's JPCGroundRemove (liso/jcp/jcp.py, imported unmodified by
path) on synthetic sweeps of liso_amd.datasets.synthetic.render (ground, walls, boxes), stored as float64.

Two stubs stand in for packages that are absent here:
  * cv2: getStructuringElement(MORPH_CROSS, (5, 5)) returns the cross footprint and dilate is
    scipy.ndimage.grey_dilation(img, footprint=cross, mode="constant", cval=0).  This is third-party arithmetic the reference does
    not contain, pinned to cv2's documented behaviour (centre anchor, nothing outside the image).
  * numba.njit as identity, with one shim: numpy 2 raises OverflowError on the `int + np.uint8` index of RECM (jcp.py:111),
    which numba types as int64, so RECM is handed region_.astype(np.int64) -- a dtype change only.  The same decorator records
    what RECM and JCP are called with / return (cloud_index_, region_minz_ after RECM, the candidate list).

Cases: the KITTI (2083x64, 1.73 m, delta_R 1), nuScenes (1024x32, 1.8 m, 1) and AV2 (2000x64, 1.8 m, 2) parameter sets, a cloud
in shuffled point order (last writer wins), a NaN-padded cloud (the padding is stripped before the reference sees it) and a
cloud with a raised, tilted ground patch so that every branch of RECM's scans fires (the counts are printed and asserted > 0).
To stay within the size limit of a committed file a cloud is a dense azimuth sector of the render plus every 40th azimuth step
of the rest (the sector is azimuth 0..17 degrees: the reference's transposed cloud_index_ read lands in the image's first
~96 columns, so a candidate survives the filter only where those columns are populated as densely as in a full sweep), and the shuffled cloud is stored as the
permutation of the KITTI cloud that it is.  Per cloud the generator asserts the near-tie condition -- smallest nonzero
|score_r - score_g| and smallest distance of a pre-truncation row / column / region value from an integer both >= 1e-9, every exact tie 0 vs 0 -- and records, for information,
how many labels differ between the reference on the float32 cloud and on its float64 widening.

A second file, ground_seg_edges_reference.npz, records the reference on the small edge clouds of tests/ground_stage_cases.py
(GOLDEN_CASES: images smaller than the 5x5 window, a 65-row image, one and 255 regions, the hand-placed degenerate rows without
the r_xy == 70 row in the last column, on which the reference's region_minz_ index leaves the table and numpy raises): the
float32 cloud, labels, cloud_index_, region_minz_ after RECM and the candidate list.  The near-tie condition of these clouds is
asserted by tests/test_ground_stage_cases.py.
Run in the build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ground_seg_golden.py"""
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_import  # noqa: E402

CAPTURE = {}
CROSS = np.zeros((5, 5), np.uint8)
CROSS[2, :] = 1
CROSS[:, 2] = 1


def _njit(*a, **k):
    def wrap(f):
        if f.__name__ == "RECM":
            def recm(**kw):
                kw["region_"] = kw["region_"].astype(np.int64)
                CAPTURE["cloud_index"] = kw["cloud_index_"].copy()
                img, minz = f(**kw)
                CAPTURE["region_minz"] = minz.copy()
                return img, minz
            return recm
        if f.__name__ == "JCP":
            def jcp(**kw):
                CAPTURE["candidates"] = kw["relevant_row_col_indices"].copy()
                return f(**kw)
            return jcp
        return f
    return wrap(a[0]) if len(a) == 1 and callable(a[0]) and not k else wrap


def load_reference():
    from scipy import ndimage

    cv2 = types.ModuleType("cv2")
    cv2.MORPH_CROSS = 2
    cv2.getStructuringElement = lambda shape, ksize: CROSS.copy() if (shape, tuple(ksize)) == (2, (5, 5)) else None
    cv2.dilate = lambda img, kernel, iterations=1: ndimage.grey_dilation(img, footprint=kernel.astype(bool), mode="constant", cval=0)
    sys.modules["cv2"] = cv2
    numba = types.ModuleType("numba")
    numba.njit = _njit
    sys.modules["numba"] = numba
    return ref_import.load("ref_jcp", "liso/jcp/jcp.py")


KITTI = dict(range_img_width=2083, range_img_height=64, sensor_height=1.73, delta_R=1)
NUSC = dict(range_img_width=1024, range_img_height=32, sensor_height=1.8, delta_R=1)
AV2 = dict(range_img_width=2000, range_img_height=64, sensor_height=1.8, delta_R=2)


def cloud(seed, sector_deg, rest_every=40):
    import torch

    from liso_amd.datasets.synthetic import make_scene, render

    boxes, _, _ = make_scene(seed, torch.device("cpu"))
    pts = render(boxes, torch.device("cpu"), seed)[0][:, :3].numpy()
    az = np.degrees(np.arctan2(pts[:, 1], pts[:, 0]))
    keep = (np.abs(az - sector_deg[0]) < sector_deg[1]) | (np.rint(az / (360.0 / 1875)).astype(np.int64) % rest_every == 0)
    return pts[keep]  # float32


def tilted_patch(p):
    """raise and tilt the ground in a wedge: steps of more than 0.5 m between neighbouring regions, holes behind the rise"""
    p = p.copy()
    r = np.hypot(p[:, 0], p[:, 1])
    az = np.degrees(np.arctan2(p[:, 1], p[:, 0]))
    wedge = (np.abs(az - 10.0) < 30.0) & (p[:, 2] < -1.4)
    bump = wedge & (r > 12) & (r < 14)
    p[bump, 2] += np.float32(0.9)
    ramp = wedge & (r > 20) & (r < 40)
    p[ramp, 2] += (np.float32(0.08) * (r[ramp] - 20)).astype(np.float32)
    gone = wedge & (((r > 16) & (r < 19)) | ((r > 45) & (r < 50)))
    return p[~gone]


def main():
    from liso_amd.jcp.jcp import jcp_host

    ref = load_reference()
    g = np.random.default_rng(7)
    cases = []
    c0 = cloud(0, (8.5, 8.5))
    cases.append(("kitti", c0, KITTI))
    cases.append(("nuscenes", cloud(1, (8.5, 8.5)), NUSC))
    cases.append(("av2", cloud(2, (8.5, 8.5)), AV2))
    perm = g.permutation(c0.shape[0])
    cases.append(("shuffled", c0[perm], KITTI))
    c4 = cloud(3, (8.5, 8.5))
    padded = np.full((c4.shape[0] + 700, 3), np.nan, np.float32)
    rows = np.sort(g.choice(padded.shape[0], c4.shape[0], replace=False))
    padded[rows] = c4
    cases.append(("nan_padded", padded, KITTI))
    cases.append(("tilted", tilted_patch(cloud(4, (8.5, 8.5), 20)), KITTI))

    out = {"names": np.array([c[0] for c in cases])}
    for name, pts32, prm in cases:
        pts = pts32.astype(np.float64)
        clean = pts[~np.isnan(pts).any(-1)]
        labels_clean = ref.JPCGroundRemove(pcl=clean.copy(), **prm)
        cap = {k: v.copy() for k, v in CAPTURE.items()}
        labels32 = ref.JPCGroundRemove(pcl=pts32[~np.isnan(pts32).any(-1)].copy(), **prm)
        labels = np.zeros(pts.shape[0], bool)
        labels[~np.isnan(pts).any(-1)] = labels_clean

        mine, info = jcp_host(pts, debug=True, **prm)
        assert np.array_equal(mine, labels), name
        assert np.array_equal(info["cloud_index"], cap["cloud_index"]), name
        assert np.array_equal(info["region_minz"], cap["region_minz"]), name
        assert np.array_equal(info["candidates"], cap["candidates"]), name
        assert info["bad_ties"] == 0, (name, "an exact tie that is not 0 vs 0")
        assert info["min_nonzero_margin"] >= 1e-9 and info["min_index_frac"] >= 1e-9, (name, info["min_nonzero_margin"], info["min_index_frac"])
        if name == "tilted":
            assert all(v > 0 for v in info["branch"].values()), info["branch"]
        print(name, "points", pts.shape[0], "ground", int(labels.sum()), "candidates", cap["candidates"].shape[0], "exact ties",
              info["exact_ties"], "min margin %.3g" % info["min_nonzero_margin"], "min index frac %.3g" % info["min_index_frac"],
              "RECM branches", info["branch"], "float32-vs-float64 labels differing", int((labels32 != labels_clean).sum()))

        if name == "shuffled":
            out["shuffled_perm_of_kitti"] = perm.astype(np.int32)
        else:
            out[f"{name}_pcl"] = pts
        out[f"{name}_params"] = np.array([prm["range_img_width"], prm["range_img_height"], prm["sensor_height"], prm["delta_R"]], np.float64)
        out[f"{name}_labels"] = labels
        out[f"{name}_cloud_index"] = cap["cloud_index"].astype(np.int32)
        out[f"{name}_region_minz"] = cap["region_minz"]
        out[f"{name}_candidates"] = cap["candidates"].astype(np.int32)
        out[f"{name}_min_margin"] = np.array(info["min_nonzero_margin"])
        out[f"{name}_min_index_frac"] = np.array(info["min_index_frac"])
        out[f"{name}_f32_label_diff"] = np.array(int((labels32 != labels_clean).sum()))
    path = os.path.join(HERE, "ground_seg_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    edges(ref, jcp_host)


def edges(ref, jcp_host):
    sys.path.insert(0, os.path.dirname(HERE))
    import ground_stage_cases as C

    out = {"names": np.array(C.GOLDEN_CASES)}
    for name in C.GOLDEN_CASES:
        pts32, prm = C.cloud(name)
        ok = ~np.isnan(pts32).any(-1)
        labels = np.zeros(pts32.shape[0], bool)
        with np.errstate(all="ignore"):
            labels[ok] = ref.JPCGroundRemove(pcl=pts32[ok].astype(np.float64), **prm)
        cap = {k: v.copy() for k, v in CAPTURE.items()}
        mine, info = jcp_host(pts32, debug=True, **prm)
        same = (np.array_equal(mine, labels), np.array_equal(info["cloud_index"], cap["cloud_index"]),
                np.array_equal(info["region_minz"], cap["region_minz"]), np.array_equal(info["candidates"], cap["candidates"].reshape(-1, 2)))
        print(name, "points", pts32.shape[0], "ground", int(labels.sum()), "candidates", cap["candidates"].shape[0],
              "host path equal (labels, cloud_index, region_minz, candidates):", same)
        assert all(same), name
        out[f"{name}_pcl"] = np.asarray(pts32)
        out[f"{name}_params"] = np.array([prm["range_img_width"], prm["range_img_height"], prm["sensor_height"], prm["delta_R"]], np.float64)
        out[f"{name}_labels"] = labels
        out[f"{name}_cloud_index"] = cap["cloud_index"].astype(np.int32)
        out[f"{name}_region_minz"] = cap["region_minz"]
        out[f"{name}_candidates"] = cap["candidates"].astype(np.int32)
    path = os.path.join(HERE, "ground_seg_edges_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
