"""GPU: every stage of JCP ground removal (liso_amd/csrc/ground_jcp.hip) against the intermediates of the numpy host path, on the
clouds of tests/ground_stage_cases.py: images smaller than the 5x5 window, one and several waves in the resolve workgroup, both
sides of the LDS opt-in and of the LDS / global-memory resolve, one, two and 255 regions, and hand-placed rows at the edges of the
projection.  tests/test_ground_stage_cases.py asserts on the CPU that these clouds meet the near-tie condition (so that fp64
device arithmetic a few ulp from the host's decides nothing) and that the dense ones depend on the visiting order.

Bounds.  Elevation extremes and weights: 1e-12 absolute -- three orders under the 1e-9 decision margin (24 weights sum to
under it), three above an ulp of pi/2.  Everything else is integer, a minimum, or +, /2 and comparisons in fp64 without
contraction on a `step` the host computes: identical.  The resolve pass is also checked against the plain raster-order loop on
the device's own stage-4 tables, where no near-tie proviso applies: the same weights, the same order of additions."""
import os

import numpy as np
import pytest
import torch

import ground_stage_cases as C
from liso_amd.jcp.jcp import JPCGroundRemove, jcp_device, jcp_tables, unkey_f32, unkey_f64

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EDGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ground_seg_edges_reference.npz")
GUARDED = ("rough_5x5", "rough_70x65", "rough_131x127")  # W * H no multiple of 16: the label images end inside their padding


def dev_cloud(name):
    p, prm = C.cloud(name)
    return torch.from_numpy(np.array(p)).to(DEV), prm


def run(t, prm, begin, end, state=None, counts=None):
    """-> (state, its tables as named tensor views)"""
    state = jcp_device(t, counts=counts, stages=(begin, end), state=state, **prm)
    return state, jcp_tables(state, t, **prm)


def host_tables(name):
    """the host path's intermediates in the device's layout and raw row numbers"""
    p, prm = C.cloud(name)
    W, H = prm["range_img_width"], prm["range_img_height"]
    labels, info = C.host(name)
    valid = np.flatnonzero(~np.isnan(p).any(-1))
    pix = np.full(p.shape[0], -1, np.int64)
    pix[valid] = (info["col"] % W) * H + info["row"]  # a negative column reads its label at W + col
    ci = info["cloud_index"]
    cand = info["candidates"]
    return dict(labels=labels, pix=pix, widx=np.where(ci >= 0, valid[np.maximum(ci, 0)], -1), minz_raw=info["region_minz_raw"],
                minz=info["region_minz"], lab0=info["labels_recm"], lab4=info["labels_candidates"], lab5=info["labels"], cand=cand,
                row_cnt=np.bincount(cand[:, 0], minlength=H), wts=info["weights"], min_ele=info["min_ele"], max_ele=info["max_ele"])


def candidate_lists(tb, b=0):
    """the device's stage-4 lists of cloud b -> (cand [K,2] in raster order, wts [K,24]) as numpy"""
    row_cnt, cols, wts = tb["row_cnt"][b], tb["cols"][b], tb["wts"][b]
    H, W = cols.shape
    assert int(row_cnt.min()) >= 0 and int(row_cnt.max()) <= W
    used = torch.arange(W, device=cols.device)[None, :] < row_cnt[:, None]
    rows = torch.arange(H, device=cols.device)[:, None].expand(H, W)[used]
    return torch.stack([rows, cols[used].long()], -1).cpu().numpy(), wts[used].cpu().numpy()


def np_(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("name", list(C.CASES))
def test_each_stage_equals_the_host_path(name):
    t, prm = dev_cloud(name)
    want = host_tables(name)
    N = t.shape[0]

    # stage 1: elevation extremes
    _, tb = run(t, prm, 0, 2)
    ele = unkey_f64(np_(tb["ele_key"])[0])
    err = max(abs(ele[0] - want["min_ele"]), abs(ele[1] - want["max_ele"]))
    print(f"{name}: min / max elevation {ele[0]!r} / {ele[1]!r}, off the host's by {err:.3g}")
    assert err <= 1e-12

    # stage 2: projection
    _, tb = run(t, prm, 0, 3)
    assert np.array_equal(np_(tb["pix"])[0], want["pix"])
    assert np.array_equal(np_(tb["widx"])[0], want["widx"])
    assert np.array_equal(unkey_f32(np_(tb["minz_key"])[0]).astype(np.float64), want["minz_raw"])

    # stage 3: RECM, bit for bit, and the per-pixel labels
    _, tb = run(t, prm, 0, 4)
    assert np.array_equal(np_(tb["minz"])[0].view(np.int64), want["minz"].view(np.int64))
    assert np.array_equal(np_(tb["lab0"])[0], want["lab0"])

    # stage 4: candidates, their lists and weights
    state4, tb = run(t, prm, 0, 5)
    lab4 = np_(tb["lab1"])[0]
    assert np.array_equal(lab4, want["lab4"])
    assert np.array_equal(np_(tb["row_cnt"])[0], want["row_cnt"])
    cand, wts = candidate_lists(tb)
    assert np.array_equal(cand, want["cand"])
    werr = float(np.abs(wts - want["wts"]).max()) if wts.size else 0.0
    print(f"{name}: {cand.shape[0]} candidates, weights off the host's by {werr:.3g}")
    assert werr <= 1e-12

    # stage 5 on the same workspace: the wavefront against the plain raster loop on the device's own tables
    _, tb = run(t, prm, 5, 6, state=state4)
    lab5 = np_(tb["lab1"])[0]
    raster = C.resolve_raster(lab4, cand, wts)
    print(f"{name}: resolved image differs from the raster loop on the device's tables in {int((lab5 != raster).sum())} pixels, "
          f"from the host's image in {int((lab5 != want['lab5']).sum())}")
    assert np.array_equal(lab5, raster)
    assert np.array_equal(lab5, want["lab5"])
    _, tb = run(t, prm, 0, 6)
    assert np.array_equal(np_(tb["lab1"])[0], want["lab5"])

    # stage 6: per-point labels, 0 on invalid rows
    _, tb = run(t, prm, 0, 7)
    labels = np_(tb["labels"])[0]
    assert labels.shape == (N,) and set(np.unique(labels).tolist()) <= {0, 1}
    assert np.array_equal(labels.astype(bool), want["labels"])
    assert not labels[np.isnan(C.cloud(name)[0]).any(-1)].any()


TABLES = ("ele_key", "pix", "widx", "minz_key", "minz", "lab0", "lab1", "row_cnt", "labels")


def snapshot(tb):
    out = {k: np_(tb[k]).copy() for k in TABLES}
    out["ele"] = np_(tb["ele"]).copy()
    for b in range(tb["cols"].shape[0]):
        out[f"cand{b}"], out[f"wts{b}"] = candidate_lists(tb, b)
    return out


def same_bits(x, y):
    if x.dtype == np.float64:
        x, y = np.ascontiguousarray(x).view(np.int64), np.ascontiguousarray(y).view(np.int64)
    return np.array_equal(x, y)


def assert_same_tables(a, b, what, valid_rows):
    for k in a:
        x, y = a[k], b[k]
        if k == "ele":  # the elevation of an invalid row is never written
            x, y = x[valid_rows], y[valid_rows]
        assert same_bits(x, y), (what, k)


@pytest.mark.parametrize("name", list(C.CASES))
def test_split_runs_and_a_second_run_equal_the_one_call(name):
    t, prm = dev_cloud(name)
    valid = ~np.isnan(C.cloud(name)[0]).any(-1)[None]
    state, tb = run(t, prm, 0, 7)
    whole = snapshot(tb)
    assert np.array_equal(whole["labels"][0].astype(bool), np_(JPCGroundRemove(pcl=t, **prm)))
    for s in range(1, 7):
        st, _ = run(t, prm, 0, s)
        _, tb = run(t, prm, s, 7, state=st)
        assert_same_tables(snapshot(tb), whole, f"stages (0, {s}) then ({s}, 7)", valid)
    _, tb = run(t, prm, 0, 7, state=state)  # the same workspace again: stage 0 resets what the stages accumulate into
    assert_same_tables(snapshot(tb), whole, "second run on the same workspace", valid)


@pytest.mark.parametrize("shape", [(70, 65), (513, 320)])
def test_batch_equals_the_single_calls_table_by_table(shape):
    """three different clouds with a zero-length cloud and an all-NaN cloud between them, finite junk behind the counts"""
    W, H = shape
    prm = C.params(W, H)
    clouds = [C.rough(W, H, 31), C.scene(W, H, 32), C.rough(W, H, 33, 0.8)]
    lengths = [clouds[0].shape[0], 0, clouds[1].shape[0], 50, clouds[2].shape[0]]
    n_max = max(lengths) + 7
    batch = np.full((5, n_max, 3), 7.5, np.float32)
    for b, c in zip((0, 2, 4), clouds):
        batch[b, : c.shape[0]] = c
    batch[3, :50] = np.nan
    t = torch.from_numpy(batch).to(DEV)
    counts = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    _, tb = run(t, prm, 0, 7, counts=counts)
    got = snapshot(tb)
    for b, n in enumerate(lengths):
        assert (got["pix"][b, n:] == -1).all() and not got["labels"][b, n:].any(), b  # rows beyond the count
    for b in (1, 3):  # no valid row: nothing projected, nothing labelled
        assert (got["pix"][b] == -1).all() and (got["widx"][b] == -1).all() and not got["labels"][b].any()
        assert not got["lab0"][b].any() and not got["lab1"][b].any() and not got["row_cnt"][b].any() and got[f"cand{b}"].shape[0] == 0
        assert got["ele_key"][b].view(np.uint64).tolist() == [2**64 - 1, 0]
    for b, c in zip((0, 2, 4), clouds):
        _, one = run(torch.from_numpy(c).to(DEV), prm, 0, 7)
        one = snapshot(one)
        n = c.shape[0]
        assert got[f"cand{b}"].shape[0] > 50
        for k in ("ele_key", "widx", "minz_key", "minz", "lab0", "lab1", "row_cnt"):
            assert same_bits(got[k][b], one[k][0]), (b, k)
        for k in ("pix", "labels", "ele"):
            assert same_bits(got[k][b, :n], one[k][0]), (b, k)
        assert np.array_equal(got[f"cand{b}"], one["cand0"]) and same_bits(got[f"wts{b}"], one["wts0"]), b


@pytest.mark.parametrize("name", GUARDED)
def test_guard_bands_stay_intact_at_odd_sizes(name):
    from guarded_alloc import guarded

    t, prm = dev_cloud(name)
    assert (prm["range_img_width"] * prm["range_img_height"]) % 16 != 0
    with guarded() as g:
        state, tb = run(t, prm, 0, 7)
        assert g.check() >= 2  # labels, workspace
        got = JPCGroundRemove(pcl=t, **prm)
        assert g.check() >= 2
    assert np.array_equal(np_(got), C.host(name)[0])
    assert np.array_equal(np_(tb["labels"])[0].astype(bool), C.host(name)[0])


@pytest.mark.parametrize("name", C.GOLDEN_CASES)
def test_device_equals_the_reference_at_the_edges(name):
    d = np.load(EDGES)
    t, prm = dev_cloud(name)
    got = np_(JPCGroundRemove(pcl=t, **prm))
    print(name, "labels differing:", int((got != d[f"{name}_labels"]).sum()), "of", got.size)
    assert np.array_equal(got, d[f"{name}_labels"])
