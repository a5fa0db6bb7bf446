"""CPU: the clouds of tests/ground_stage_cases.py do what tests/test_gpu_ground_stages.py relies on -- asserted on the numpy host
path alone -- and the host path equals the reference's records at the new shapes (tests/golden/ground_seg_edges_reference.npz,
made by tests/golden/make_ground_seg_golden.py)."""
import os
import re

import numpy as np
import pytest

import ground_stage_cases as C

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EDGES = os.path.join(ROOT, "tests", "golden", "ground_seg_edges_reference.npz")


def _figures(name):
    _, info = C.host(name)
    cand = info["candidates"]
    _, prm = C.cloud(name)
    pixels = prm["range_img_width"] * prm["range_img_height"]
    lab4, wts = info["labels_candidates"], info["weights"]
    return dict(info=info, cand=cand, share=cand.shape[0] / pixels, dependent=float(C.has_earlier_candidate(lab4, cand).mean()),
                raster=C.resolve_raster(lab4, cand, wts), at_once=C.resolve_wavefront(lab4, cand, wts, None),
                skew3=C.resolve_wavefront(lab4, cand, wts, 3), skew2=C.resolve_wavefront(lab4, cand, wts, 2))


@pytest.mark.parametrize("name", list(C.CASES))
def test_near_tie_condition_holds(name):
    """what host_labels_checked of tests/test_gpu_ground_seg.py asks of a cloud before device labels must equal the host's"""
    p, _ = C.cloud(name)
    _, info = C.host(name)
    skip = []
    if name.startswith("degenerate"):
        # exact by construction, the same IEEE operations on both sides: sqrt(42^2 + 56^2) = sqrt(70^2) = 70 gives the region
        # value 67.0, and asin(0) = 0 between asin(-1) and asin(1) gives the row value H / 2
        names = C.degenerate(name == "degenerate")[1]
        valid = np.flatnonzero(~np.isnan(p).any(-1))
        skip = [int(np.searchsorted(valid, names[k])) for k in ("r70_inner", "r70_last", "x_inf") if k in names]
        assert (info["index_frac"][skip] == 0.0).all()
    bad, margin, frac = C.near_tie_figures(info, skip)
    print(f"{name}: candidates {info['candidates'].shape[0]}, bad ties {bad}, min nonzero margin {margin:.3g}, min index distance {frac:.3g}")
    assert bad == 0
    assert margin >= 1e-9 and frac >= 1e-9


@pytest.mark.parametrize("name", C.ORDER_CASES + (C.BIG,))
def test_rough_cases_depend_on_the_visiting_order(name):
    f = _figures(name)
    print(f"{name}: candidates {f['cand'].shape[0]} = {f['share']:.3f} of the pixels, {f['dependent']:.3f} with an earlier candidate in the "
          f"window, at once differs in {int((f['at_once'] != f['raster']).sum())}, skew 2 in {int((f['skew2'] != f['raster']).sum())}")
    min_share, min_dependent = (0.03, 0.60) if name == C.BIG else (0.15, 0.90)
    assert f["share"] >= min_share and f["dependent"] >= min_dependent
    assert np.array_equal(f["raster"], f["info"]["labels"])  # the restatement is the host path's pass
    assert not np.array_equal(f["at_once"], f["raster"])  # else the case does not test the order
    assert np.array_equal(f["skew3"], f["raster"])  # the device's wavefront order
    assert not np.array_equal(f["skew2"], f["raster"])  # one column less of skew reads a row above too early: the check bites


def test_every_recm_branch_fires_and_region_edges_run_no_loop():
    total = {}
    for name in C.CASES:
        _, info = C.host(name)
        for k, v in info["branch"].items():
            total[k] = total.get(k, 0) + v
    assert set(total) == {"hole_before_first", "hole_after_first", "smoothed", "second_scan_lowered"} and all(v > 0 for v in total.values()), total
    for name, length in C.REGIONS.items():
        _, prm = C.cloud(name)
        _, info = C.host(name)
        assert int(67.0 / prm["delta_R"]) == length and info["region_minz"].shape[0] == prm["range_img_width"] * length
        assert info["candidates"].shape[0] > 1000, name
    b1, b2 = C.host("rough_L1")[1]["branch"], C.host("rough_L2")[1]["branch"]
    assert all(v == 0 for v in b1.values()), b1  # length 1: neither scan has a position to visit
    assert b2["hole_before_first"] == b2["hole_after_first"] == b2["smoothed"] == 0, b2  # length 2: the first scan has none
    assert all(v > 0 for v in C.host("rough_L255")[1]["branch"].values())


def test_shapes_straddle_the_resolve_paths():
    hdr = open(os.path.join(ROOT, "include", "liso_ground.h")).read()
    lds = eval(re.search(r"#define LISO_GROUND_LDS_BYTES \(([0-9 *]+)\)", hdr).group(1))
    max_h = int(re.search(r"#define LISO_GROUND_MAX_HEIGHT (\d+)", hdr).group(1))
    stride = lambda name: (C.CASES[name][1] * C.CASES[name][2] + 15) // 16 * 16  # noqa: E731
    assert stride("rough_1024x64") == 64 * 1024 and stride("rough_1025x64") > 64 * 1024  # the LDS opt-in
    assert stride("rough_512x320") == lds and stride("rough_513x320") > lds  # LDS and global resolve, 5 waves
    assert C.CASES[C.BIG][2] == max_h and stride(C.BIG) > lds and C.cloud(C.BIG)[0].shape[0] <= 600000
    assert C.CASES["rough_64x64"][2] == 64 and C.CASES["rough_70x65"][2] == 65  # one full wave, a second wave with one lane
    for name, (_, W, H, _) in C.CASES.items():
        assert (H - 1) * H + W - 1 < W * H, name


def test_degenerate_rows_land_where_intended():
    W, H, length = 64, 16, 67
    p, names = C.degenerate()
    assert np.array_equal(p, C.cloud("degenerate")[0], equal_nan=True)
    labels, info = C.host("degenerate")
    is_nan = np.isnan(p).any(-1)
    assert np.array_equal(np.flatnonzero(is_nan), names["nan_rows"]) and 0 < names["nan_rows"][0] < names["nan_rows"][-1] < p.shape[0] - 1
    assert not labels[is_nan].any()
    valid = np.flatnonzero(~is_nan)
    v = {k: int(np.searchsorted(valid, r)) for k, r in names.items() if k != "nan_rows"}  # valid-row numbers
    row, col, kept, widx = info["row"], info["col"], set(info["kept"].tolist()), info["cloud_index"]
    raw = info["region_minz_raw"].reshape(W, length)

    # y == -0.0: x < 0 gives the negative column, left out of the projection, its label read at W + col; x > 0 gives column 0
    i = v["neg_zero_y_neg_x"]
    assert np.signbit(p[names["neg_zero_y_neg_x"], 1]) and col[i] == -31 and i not in kept and i not in widx
    assert labels[names["neg_zero_y_neg_x"]] and info["labels"][row[i], W - 31] == C.GROUND  # "labelled 0" would differ
    assert col[v["neg_zero_y_pos_x"]] == 0 and v["neg_zero_y_pos_x"] in kept
    # r_xy == 70: the inner column spills into the next column's region 0; the last column leaves the table alone
    i = v["r70_inner"]
    assert i in kept and 0 < col[i] < W - 1 and raw[col[i] + 1, 0] == -2.5 and (raw == -2.5).sum() == 1
    i = v["r70_last"]
    assert i in kept and col[i] == W - 1 and not (raw == -2.75).any() and widx[col[i] * H + row[i]] == i
    # r_xy == 3 and the ego box
    i = v["r3"]
    assert i in kept and raw[col[i], 0] <= p[names["r3"], 2]
    assert {k for k in ("ego_x3", "ego_inside", "ego_xm2", "ego_xm2_near", "ego_yp", "ego_ym") if v[k] in kept} == {"ego_x3", "ego_xm2", "ego_yp", "ego_ym"}
    # the elevation extremes
    assert info["min_ele"] == -np.pi / 2 and row[v["below"]] == 0 and v["below"] not in kept
    assert info["max_ele"] == np.pi / 2 and row[v["z_inf"]] == H - 1 and widx[col[v["z_inf"]] * H + H - 1] == v["z_inf"]
    assert info["labels_recm"][H - 1, col[v["z_inf"]]] == C.OBSTACLE
    assert v["x_inf"] not in kept and row[v["x_inf"]] == H // 2
    assert v["xz_inf"] not in kept and row[v["xz_inf"]] == 0
    # last writer wins in both orders
    for a, b in (("pair_a_first", "pair_a_last"), ("pair_b_first", "pair_b_last")):
        assert (row[v[a]], col[v[a]]) == (row[v[b]], col[v[b]]) and widx[col[v[b]] * H + row[v[b]]] == v[b]
    assert p[names["pair_a_first"], 2] > p[names["pair_a_last"], 2] and p[names["pair_b_first"], 2] < p[names["pair_b_last"], 2]
    # two equal z in one region
    a, b = v["equal_z_a"], v["equal_z_b"]
    ra, rb = (int(np.hypot(*p[names[k], :2].astype(np.float64)) - 3.0) for k in ("equal_z_a", "equal_z_b"))
    assert col[a] == col[b] and ra == rb and raw[col[a], ra] == -2.0 and (raw == -2.0).sum() == 1
    # one elevation, one point
    _, one = C.host("one_elevation")
    assert one["min_ele"] == one["max_ele"] and (one["row"] == 0).all() and len(set(one["col"].tolist())) > 10
    lab1, info1 = C.host("one_point")
    assert info1["row"][0] == 0 and info1["cloud_index"].max() == 0 and lab1.shape == (1,)


@pytest.mark.parametrize("name", C.GOLDEN_CASES)
def test_host_path_equals_the_reference_at_the_edges(name):
    d = np.load(EDGES)
    assert set(C.GOLDEN_CASES) == {str(n) for n in d["names"]}
    p, prm = C.cloud(name)
    assert np.array_equal(d[f"{name}_pcl"], p, equal_nan=True) and d[f"{name}_pcl"].dtype == np.float32
    assert np.array_equal(d[f"{name}_params"], [prm["range_img_width"], prm["range_img_height"], prm["sensor_height"], prm["delta_R"]])
    labels, info = C.host(name)
    assert np.array_equal(info["cloud_index"], d[f"{name}_cloud_index"])
    assert np.array_equal(info["region_minz"], d[f"{name}_region_minz"])
    assert np.array_equal(info["candidates"], d[f"{name}_candidates"].reshape(-1, 2))
    assert np.array_equal(labels, d[f"{name}_labels"])


def test_edge_records_are_small_and_hold_the_negative_column():
    assert os.path.getsize(EDGES) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "ground_seg_reference.npz"))
    p, names = C.degenerate(False)
    assert "r70_last" not in names  # the stubbed reference raises on that row
    _, info = C.host("degenerate_no_r70_last")
    assert (info["col"] < 0).sum() == 1


@pytest.mark.parametrize("N", C.REMOVAL_N)
def test_removal_clouds_meet_the_near_tie_condition_and_keep_some(N):
    batch, counts = C.removal_batch(N, 5)
    assert batch.shape == (3, N, 5) and np.array_equal(batch[..., :3], C.removal_batch(N, 3)[0], equal_nan=True)
    assert (counts <= N).all() and (N == 1 or (counts < N).any())
    if N > 1:
        assert np.isnan(batch[0, 1:-1, :3]).any() and np.isnan(batch[1, 1: counts[1] - 1, 1]).any() and not np.isnan(batch[2]).any()
        assert np.isfinite(batch[1, counts[1]:]).all()  # finite rows behind the count
    for b in range(3):
        if counts[b] == 0:
            continue
        labels, info = C.removal_host(N, b)
        bad, margin, frac = C.near_tie_figures(info)
        assert bad == 0 and margin >= 1e-9 and frac >= 1e-9, (N, b, margin, frac)
        ground = labels | C.cone_labels(batch[b, : counts[b], :3], -1.70, 0.8)
        valid = ~np.isnan(batch[b, : counts[b], :3]).any(-1)
        assert N == 1 or 0 < (valid & ~ground).sum() < valid.sum()
