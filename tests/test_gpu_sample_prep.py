"""GPU: the sample preparation kernels (include/liso_sample_prep.h) against an fp64 numpy evaluation in the stated order, against
the reference fixture tests/golden/sample_prep_reference.npz, and as one captured chain behind ground removal.

Measured on an MI355X (printed by the tests): 6 of the fixture's 16 800 transformed coordinates and flow components are not
bit-identical to the reference's einsum, all within 1 ulp; the flow mean is at most 0.42 x 2^-23 max|v| from the exact mean and at
most 0.18 x count x 2^-23 max|v| from the reference's fp32 running sum."""
import os

import numpy as np
import pytest
import torch

from liso_amd.datasets import sample_prep as S
from liso_amd.kabsch.shape_utils import Shape

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "sample_prep_reference.npz"))
THRESHOLD_DT = 0.5 * 0.1
SIZES = (0, 1, 255, 256, 257, 4099)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def ulp_distance(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
    key = lambda v: np.where(v.view(np.int32) < 0, np.int64(-2147483648) - v.view(np.int32).astype(np.int64), v.view(np.int32).astype(np.int64))  # noqa: E731
    return np.where(np.isnan(a), 0, np.abs(key(a) - key(b)))


def transform_fp64(pcl, T, linear_only=False):
    """the header's expression, written out: left to right in fp64, rounded once"""
    x, y, z = (pcl[..., c].astype(np.float64) for c in range(3))
    with np.errstate(invalid="ignore"):
        rows = [((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + (0.0 if linear_only else T[r, 3]) for r in range(3)]
    return np.stack(rows, -1).astype(np.float32)


def random_cloud(g, n, stride, nan_rows=True):
    p = np.concatenate([g.uniform(-30, 30, (n, 2)), g.uniform(-3, 2, (n, 1)), g.uniform(0, 1, (n, stride - 3))], -1).astype(np.float32)
    if nan_rows and n > 8:
        p[n // 2] = np.nan
        p[n // 3, 1] = np.nan
    return p


# ---- transform --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("B", (1, 2))
def test_transform_bitwise_against_fp64(n, B):
    g = np.random.default_rng(100 + n + B)
    stride = 3 + n % 3
    T = np.stack([G["tf_gen_off_T"], G["tf_gen_scale_T"]])[:B]
    pcl = np.stack([random_cloud(g, n, stride) for _ in range(B)])
    flow = g.normal(size=(B, n, 3)).astype(np.float32)
    out, out_flow = S.transform_cloud_device(dev(pcl), dev(T), flow=dev(flow))
    bad = np.isnan(pcl[..., :3]).any(-1)
    for b in range(B):
        want, want_flow = transform_fp64(pcl[b], T[b]), transform_fp64(flow[b], T[b], True)
        want[bad[b]], want_flow[bad[b]] = np.nan, np.nan
        got = host(out[b])
        assert np.array_equal(got[:, :3].view(np.uint32), want.view(np.uint32))
        assert np.array_equal(got[:, 3:], pcl[b][:, 3:], equal_nan=True)
        assert np.array_equal(host(out_flow[b]).view(np.uint32), want_flow.view(np.uint32))
    # in place equals out of place
    p2, f2 = dev(pcl), dev(flow)
    S.transform_cloud_device(p2, dev(T), flow=f2, out=p2, out_flow=f2)
    assert np.array_equal(host(p2), host(out), equal_nan=True) and np.array_equal(host(f2), host(out_flow), equal_nan=True)


def test_transform_fixture():
    different = total = 0
    for tag in G["tf_tags"]:
        pcl, T, flow = G[f"tf_{tag}_pcl"], G[f"tf_{tag}_T"], G[f"tf_{tag}_flow"]
        out, out_flow = S.transform_cloud_device(dev(pcl), T, flow=dev(flow))
        d1, d2 = ulp_distance(host(out)[:, :3], G[f"tf_{tag}_out_pcl"][:, :3]), ulp_distance(host(out_flow), G[f"tf_{tag}_out_flow"])
        assert d1.max() <= 1 and d2.max() <= 1, tag
        assert np.array_equal(host(out)[:, 3:], pcl[:, 3:])
        assert np.array_equal(host(S.transform_flow(dev(flow), T)), host(out_flow))
        different += int((d1 > 0).sum() + (d2 > 0).sum())
        total += d1.size + d2.size
    print(f"transform vs reference einsum: {different} of {total} elements not bit-identical (all within 1 ulp)")


def test_transform_counts_and_junk_behind_them():
    g = np.random.default_rng(5)
    n, lens = 300, (257, 40)
    pcl = np.stack([random_cloud(g, n, 4), random_cloud(g, n, 4)])  # finite junk behind the counts
    flow = g.normal(size=(2, n, 3)).astype(np.float32)
    T = np.stack([G["tf_gen_off_T"], G["tf_m90_off_T"]])
    out, out_flow = S.transform_cloud_device(dev(pcl), dev(T), flow=dev(flow), counts=dev(np.array(lens, np.int32)))
    for b, m in enumerate(lens):
        one, one_flow = S.transform_cloud_device(dev(pcl[b, :m]), T[b], flow=dev(flow[b, :m]))
        assert np.array_equal(host(out[b, :m]), host(one), equal_nan=True) and np.array_equal(host(out_flow[b, :m]), host(one_flow), equal_nan=True)
        assert np.isnan(host(out[b, m:])).all() and np.isnan(host(out_flow[b, m:])).all()


# ---- poses ------------------------------------------------------------------------------------------------------------------------
def _tree(prefix):
    tree = {}
    for k in G.files:
        if k.startswith(prefix):
            node, parts = tree, k[len(prefix):].split("/")
            for part in parts[:-1]:
                node = node.setdefault(part, {})
            node[parts[-1]] = G[k]
    return tree


def _is_shape(d):
    return isinstance(d, dict) and set(d) == {"pos", "rot", "dims", "valid"}


def _to_device_sample(d):
    if _is_shape(d):
        return Shape(pos=dev(d["pos"]), dims=dev(d["dims"]), rot=dev(d["rot"]), probs=torch.ones_like(dev(d["rot"])), valid=dev(d["valid"]))
    return {k: _to_device_sample(v) for k, v in d.items()} if isinstance(d, dict) else dev(d)


class _Cfg(dict):
    __getattr__ = dict.__getitem__


CFG = _Cfg(data=_Cfg(odom_source="kiss_icp", flow_source="slim_flow", bev_range_m=(40.0, 40.0), img_grid_size=(64, 64),
                     limit_pillar_height=False, non_rigid_flow_threshold_mps=0.5,
                     augmentation=_Cfg(rotation=_Cfg(max_rot_deg=90.0), translation=_Cfg(max_sensor_pos_offset_m=5.0))))


def _check_augmented(got, want, given, T):
    for k, w in want.items():
        if isinstance(w, dict) and "poses" in w:
            np.testing.assert_allclose(host(got[k]["poses"]), w["poses"], rtol=0, atol=1e-12)
        elif _is_shape(w):
            v = w["valid"].astype(bool)
            gp, gr, src = host(got[k].pos), host(got[k].rot), given[k]
            assert gp.dtype == src["pos"].dtype and gr.dtype == src["rot"].dtype
            if gp.dtype == np.float64:
                assert (np.abs(gp[v] - w["pos"][v]) <= np.spacing(np.abs(w["pos"][v]))).all()  # 1 ulp of the storage dtype
                assert np.abs(gr[v] - w["rot"][v]).max() <= 1e-12
            else:
                assert ulp_distance(gp[v], w["pos"][v].astype(np.float32)).max() <= 1
                # yaw within 1e-12 before it is stored as fp32: at most one rounding of a value within 1e-12 of the reference's
                assert (np.abs(gr[v].astype(np.float64) - w["rot"][v]) <= 0.5 * np.spacing(np.abs(w["rot"][v]).astype(np.float32)) + 1e-12).all()
            assert np.array_equal(gp[~v], src["pos"][~v]) and np.array_equal(gr[~v], src["rot"][~v])  # invalid boxes untouched
        elif isinstance(w, dict):
            _check_augmented(got[k], w, given.get(k, {}), T)
        elif k.startswith("odom"):
            ours = host(got[k])
            if k in given:
                O = given[k]
                bound = 16 * 2.0 ** -52 * np.linalg.cond(T) * np.linalg.cond(O) * max(np.abs(T).max(), np.abs(O).max(), np.abs(w).max())
                assert np.abs(ours - w).max() <= bound, (k, np.abs(ours - w).max(), bound)
                rev = k.split("_")
                inv = host(got["_".join([rev[0], rev[2], rev[1]])])
                assert np.abs(ours @ inv - np.eye(4)).max() <= bound
        elif k.startswith("pcl") or k.startswith("flow"):
            assert ulp_distance(host(got[k])[:, :3], w[:, :3]).max() <= 1, k
            assert np.array_equal(host(got[k])[:, 3:], w[:, 3:])


@pytest.mark.parametrize("tag,dataset", [("aw", "waymo"), ("ak", "kitti_object")])
def test_augment_sample_content_device(tag, dataset):
    given, want = _tree(f"{tag}_in/"), _tree(f"{tag}_out/")
    got = _to_device_sample(given)
    np.random.seed(int(G[f"{tag}_seed"]))
    T = S.augment_sample_content(got, "t0", "t1", dataset, cfg=CFG)
    np.testing.assert_allclose(T, G[f"{tag}_T"], rtol=0, atol=1e-13)
    _check_augmented(got, want, given, T)
    for sub, k in ((got["gt"], "odom_t1_t0"), (got["gt"], "odom_tx_t0"), (got["kiss_icp"], "odom_t1_t0")):
        assert k in sub


def test_poses_batched_with_per_sample_transforms():
    g = np.random.default_rng(9)
    B, K = 2, 300  # more than one block of boxes
    T = np.stack([G["tf_gen_off_T"], G["tf_gen_scale_T"]])
    pos, rot = g.uniform(-20, 20, (B, K, 3)), g.uniform(-np.pi, np.pi, (B, K, 1))
    valid = g.uniform(size=(B, K)) > 0.25
    odom = np.stack([G["aw_in/gt/odom_t0_t1"], G["ak_in/gt/odom_t0_t1"]])
    s = Shape(pos=dev(pos), dims=torch.ones(B, K, 3, device=DEV, dtype=torch.float64), rot=dev(rot),
              probs=torch.ones(B, K, 1, device=DEV, dtype=torch.float64), valid=dev(valid))
    out = S.transform_boxes(s, dev(T))
    new, inv = S.transform_odometry(dev(odom), dev(T))
    for b in range(B):
        wp, wr = S.transform_boxes_host(pos[b], rot[b], valid[b], T[b])
        # two fp64 evaluations of a four-term sum (the device's fused chain, the host's unfused one): each within
        # 4 * 2^-53 * sum |term| of the exact value
        terms = np.abs(pos[b]) @ np.abs(T[b][:3, :3]).T + np.abs(T[b][:3, 3])
        assert (np.abs(host(out.pos[b]) - wp) <= 8 * 2.0 ** -53 * terms).all() and np.abs(host(out.rot[b]) - wr).max() <= 1e-12
        assert np.array_equal(host(out.pos[b])[~valid[b]], pos[b][~valid[b]])
        want = T[b] @ odom[b] @ np.linalg.inv(T[b])
        bound = 16 * 2.0 ** -52 * np.linalg.cond(T[b]) * np.linalg.cond(odom[b]) * max(np.abs(T[b]).max(), np.abs(odom[b]).max(), np.abs(want).max())
        assert np.abs(host(new[b]) - want).max() <= bound and np.abs(host(new[b]) @ host(inv[b]) - np.eye(4)).max() <= bound
    assert np.array_equal(host(s.pos), pos)  # the input Shape is not changed


# ---- crop -------------------------------------------------------------------------------------------------------------------------
def crop_kwargs(tag):
    m = G[f"{tag}_meta"]
    return dict(bev_range_m=m[2:4], img_grid_size=m[0:2].astype(np.int64), height_range_m=m[4:6])


def check_crop(got, b, prefix, n_max):
    """cloud b of the device result against the fixture arrays under `prefix`, paddings included"""
    m = G[f"{prefix}_pcl"].shape[0]
    assert int(got["counts"][b]) == m
    for k, ref, pad in (("pcl", "pcl", np.nan), ("pillar_coors", "coors", -1), ("flow", "flow", np.nan), ("lidar_rows", "rows", 0),
                        ("attr", "is_ground", 0)):
        a = host(got[k][b])
        assert a.shape[0] == n_max
        assert np.array_equal(a[:m], G[f"{prefix}_{ref}"], equal_nan=True), (prefix, k)
        assert np.isnan(a[m:]).all() if np.isnan(pad) else (a[m:] == pad).all(), (prefix, k, "padding")


@pytest.mark.parametrize("tag", [str(t) for t in G["crop_tags"]])
def test_crop_fixture(tag):
    pcl, flow, rows, ground = G[f"{tag}_pcl"], G[f"{tag}_flow"], G[f"{tag}_rows"], G[f"{tag}_is_ground"]
    n = pcl.shape[0]
    for prefix, drop in ((f"{tag}_crop", None), (f"{tag}_removed", ground)):
        got = S.pillarize_bev(dev(pcl)[None], flow=dev(flow)[None], lidar_rows=dev(rows)[None], attr=dev(ground)[None],
                              drop=None if drop is None else dev(drop)[None], **crop_kwargs(tag))
        check_crop(got, 0, prefix, n)


def test_crop_batch_of_two_lengths_and_negative_edge_band():
    na, nb = G["ca_pcl"].shape[0], G["cb_pcl"].shape[0]
    g = np.random.default_rng(3)

    def padded(ka, kb, tail, dtype):
        out = g.uniform(-5, 5, (2, na) + tail).astype(dtype)  # finite junk behind the shorter cloud
        out[0], out[1, :nb] = G[ka], G[kb]
        return dev(out)

    got = S.pillarize_bev(padded("ca_pcl", "cb_pcl", (4,), np.float32), dev(np.array([na, nb], np.int32)),
                          flow=padded("ca_flow", "cb_flow", (3,), np.float32), lidar_rows=padded("ca_rows", "cb_rows", (), np.int32),
                          attr=padded("ca_is_ground", "cb_is_ground", (), np.uint8).bool(), **crop_kwargs("ca"))
    check_crop(got, 0, "ca_crop", na)
    check_crop(got, 1, "cb_crop", na)
    pcl = G["ca_pcl"]
    band = (pcl[:, 0] < -20.0) & (pcl[:, 0] > -20.0 - 40.0 / 64) & (np.abs(pcl[:, 1]) < 19.0) & ~np.isnan(pcl).any(-1)
    kept = host(got["pcl"][0, : int(got["counts"][0])])
    co = host(got["pillar_coors"][0, : int(got["counts"][0])])
    in_band = (kept[:, 0] < -20.0) & (np.abs(kept[:, 1]) < 19.0)
    assert band.sum() >= 10 and in_band.sum() == band.sum() and (co[in_band, 0] == 0).all()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("B", (1, 2))
def test_crop_drop_masks_across_block_boundaries(n, B):
    g = np.random.default_rng(200 + n)
    kw = dict(bev_range_m=(40.0, 40.0), img_grid_size=(64, 64))
    pcl = np.stack([random_cloud(g, n, 3 + n % 3) for _ in range(B)])
    flow = g.normal(size=(B, n, 3)).astype(np.float32)
    rows = g.integers(0, 64, (B, n)).astype(np.int32)
    for name, drop in (("keep-all", np.zeros((B, n), bool)), ("keep-none", np.ones((B, n), bool)), ("alternating", (np.arange(B * n).reshape(B, n) % 2) == 1)):
        got = S.pillarize_bev(dev(pcl), flow=dev(flow), lidar_rows=dev(rows), drop=dev(drop), **kw)
        for b in range(B):
            want = S.bev_crop_host(pcl[b], flow=flow[b], lidar_rows=rows[b], drop=drop[b], **kw)
            m = want["count"]
            assert int(got["counts"][b]) == m, name
            if name == "keep-none":
                assert m == 0
            assert np.array_equal(host(got["pcl"][b, :m]), want["pcl"]) and np.isnan(host(got["pcl"][b, m:])).all(), name
            assert np.array_equal(host(got["pillar_coors"][b, :m]), want["pillar_coors"]) and (host(got["pillar_coors"][b, m:]) == -1).all()
            assert np.array_equal(host(got["flow"][b, :m]), want["flow"]) and np.isnan(host(got["flow"][b, m:])).all()
            assert np.array_equal(host(got["lidar_rows"][b, :m]), want["lidar_rows"]) and (host(got["lidar_rows"][b, m:]) == 0).all()


def test_guard_bands_stay_intact():
    from guarded_alloc import guarded

    pcl, flow, rows, ground = G["ca_pcl"], G["ca_flow"], G["ca_rows"], G["ca_is_ground"]
    batch = np.stack([pcl, pcl[::-1]])
    with guarded() as g:
        t = S.transform_cloud_device(dev(batch), G["tf_gen_off_T"])
        got = S.pillarize_bev(t, flow=dev(np.stack([flow, flow[::-1]])), lidar_rows=dev(np.stack([rows, rows[::-1]])),
                              attr=dev(np.stack([ground, ground[::-1]])), drop=dev(np.stack([ground, ground[::-1]])), **crop_kwargs("ca"))
        maps = S.bev_point_maps(got["pillar_coors"], got["counts"], (64, 64), pcl=got["pcl"], flow=got["flow"], flow2=got["flow"],
                                odom_tb_ta=dev(np.stack([G["ca_odom_t1_t0"]] * 2)), threshold_dt=THRESHOLD_DT)
        assert g.check() >= 10  # outputs, counts, workspaces
    assert set(maps) == {"occupancy_f32", "flow_bev", "flow_bev2", "moving_mask"}


# ---- maps -------------------------------------------------------------------------------------------------------------------------
def cell_statistics(coors, flow, H, W):
    cnt, top, exact = np.zeros((H, W)), np.zeros((H, W, 3)), np.zeros((H, W, 3))
    np.add.at(cnt, tuple(coors.T), 1)
    np.maximum.at(top, tuple(coors.T), np.abs(flow.astype(np.float64)))
    np.add.at(exact, tuple(coors.T), flow.astype(np.float64))
    return cnt, top, exact / np.maximum(cnt, 1)[..., None]


@pytest.mark.parametrize("tag", [str(t) for t in G["crop_tags"]])
def test_maps_fixture(tag):
    kw = crop_kwargs(tag)
    H, W = (int(v) for v in kw["img_grid_size"])
    for prefix in (f"{tag}_crop", f"{tag}_removed"):
        pcl, coors, flow = G[f"{prefix}_pcl"], G[f"{prefix}_coors"], G[f"{prefix}_flow"]
        n = pcl.shape[0]
        args = dict(pcl=dev(pcl)[None], flow=dev(flow)[None], odom_tb_ta=dev(G[f"{tag}_odom_t1_t0"])[None], threshold_dt=THRESHOLD_DT)
        got = S.bev_point_maps(dev(coors)[None], None, (H, W), flow2=dev(flow * np.float32(-3.0))[None], **args)
        assert np.array_equal(host(got["occupancy_f32"][0]), G[f"{prefix}_occupancy"])
        assert np.array_equal(host(got["moving_mask"][0]), G[f"{prefix}_moving"])
        bev = host(got["flow_bev"][0])
        cnt, top, exact = cell_statistics(coors, flow, H, W)
        err, ref_err = np.abs(bev - exact), np.abs(bev.astype(np.float64) - G[f"{prefix}_flow_bev"])
        print(f"{prefix}: flow_bev max error / (2^-23 max|v|) = {np.max(err / np.maximum(2.0 ** -23 * top, 1e-300)):.3f}, "
              f"against the reference / (count 2^-23 max|v|) = {np.max(ref_err / np.maximum(cnt[..., None] * 2.0 ** -23 * top, 1e-300)):.3f}")
        assert (err <= 2.0 ** -23 * top).all()
        assert (ref_err <= cnt[..., None] * 2.0 ** -23 * top).all()
        assert (bev[cnt == 0] == 0).all()
        _, top2, exact2 = cell_statistics(coors, flow * np.float32(-3.0), H, W)
        assert (np.abs(host(got["flow_bev2"][0]) - exact2) <= 2.0 ** -23 * top2).all()
        # two runs are bitwise equal, and so is a run on the rows permuted
        again = S.bev_point_maps(dev(coors)[None], None, (H, W), flow2=dev(flow * np.float32(-3.0))[None], **args)
        assert np.array_equal(host(again["flow_bev"]).view(np.uint32), host(got["flow_bev"]).view(np.uint32))
        perm = np.random.default_rng(n).permutation(n)
        shuffled = S.bev_point_maps(dev(coors[perm])[None], None, (H, W), flow=dev(flow[perm])[None])
        assert np.array_equal(host(shuffled["flow_bev"]).view(np.uint32), host(got["flow_bev"]).view(np.uint32))
        assert np.array_equal(host(shuffled["occupancy_f32"]), host(got["occupancy_f32"]))
        # rows behind the count take no part and have no mask
        m = n // 2
        half = S.bev_point_maps(dev(coors)[None], dev(np.array([m], np.int32)), (H, W), **args)
        assert np.array_equal(host(half["occupancy_f32"][0, 0]), cell_statistics(coors[:m], flow[:m], H, W)[0] > 0)
        assert not host(half["moving_mask"][0, m:]).any() and np.array_equal(host(half["moving_mask"][0, :m]), G[f"{prefix}_moving"][:m])
        assert np.array_equal(host(S.moving_mask(dev(pcl), dev(flow), dev(G[f"{tag}_odom_t1_t0"]), THRESHOLD_DT)), G[f"{prefix}_moving"])
        assert np.array_equal(host(S.add_bev_flow(dev(coors), dev(flow), (H, W))), bev)
        assert np.array_equal(host(S.add_bev_ground_height_occupancy_maps(dev(coors), (H, W))), G[f"{prefix}_occupancy"])


# ---- the chain ------------------------------------------------------------------------------------------------------------------
def test_chain_is_captured_once_and_replayed_with_a_second_sample():
    from liso_amd.datasets.torch_dataset_commons import remove_ground_points
    from liso_amd.utils import graph_capture

    ground = dict(range_img_width=512, range_img_height=32, sensor_height=1.73, delta_R=1)
    odom = dev(np.stack([G["ca_odom_t1_t0"]]))
    samples = [(dev(G[f"chain{s}_pcl"])[None], dev(G[f"chain{s}_flow"])[None], dev(G[f"chain{s}_T"])[None]) for s in (0, 1)]

    def chain(pcl, flow, T):
        _, _, is_ground = remove_ground_points(pcl, **ground)
        sample = {"pcl_t0": pcl, "pcl_t1": pcl, "gt": {"flow_t0_t1": flow, "odom_t0_t1": odom}}
        S.augment_sample_content(sample, "t0", "t1", "waymo", cfg=CFG, T=T)
        out = S.assemble_bev_sample(sample["pcl_t0"], None, flow=sample["gt"]["flow_t0_t1"], drop=is_ground,
                                    odom_tb_ta=sample["gt"]["odom_t1_t0"], dt=0.1, cfg=CFG)
        return [out["pcl_ta"]["pcl"], out["pcl_ta"]["pcl_is_valid"], out["pcl_ta"]["pillar_coors"], out["counts"], out["occupancy_f32"],
                out["flow_ta_tb"], out["flow_bev_ta_tb"], out["moving_mask"], is_ground]

    eager = [[host(t) for t in chain(*s)] for s in samples]
    # without ground removal the chain reproduces the reference's transform -> crop -> maps
    for s, (pcl, flow, T) in enumerate(samples):
        sample = {"pcl_t0": pcl, "pcl_t1": pcl, "gt": {"flow_t0_t1": flow}}
        S.augment_sample_content(sample, "t0", "t1", "waymo", cfg=CFG, T=T)
        out = S.assemble_bev_sample(sample["pcl_t0"], None, flow=sample["gt"]["flow_t0_t1"], cfg=CFG)
        m = int(out["counts"][0])
        assert m == G[f"chain{s}_out_pcl"].shape[0]
        assert np.array_equal(host(out["pcl_ta"]["pillar_coors"][0, :m]), G[f"chain{s}_out_coors"])
        assert np.array_equal(host(out["occupancy_f32"][0]), G[f"chain{s}_out_occupancy"])
        assert ulp_distance(host(out["pcl_ta"]["pcl"][0, :m, :3]), G[f"chain{s}_out_pcl"][:, :3]).max() <= 1
        assert host(out["pcl_ta"]["pcl_is_valid"][0]).sum() == m
    static = [t.clone() for t in samples[0]]
    stream = torch.cuda.Stream()
    graph, outs = graph_capture.capture(lambda: chain(*static), stream, warm_ups=2)
    for s in (0, 1):
        for dst, src in zip(static, samples[s]):
            dst.copy_(src)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs, eager[s]):
            assert np.array_equal(host(got), want, equal_nan=True)
    n = samples[0][0].shape[1]
    assert 0 < eager[0][3][0] < n and 0 < eager[0][8].sum() < n  # some points were kept and some ground was removed
