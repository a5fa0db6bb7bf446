"""Box-snippet augmentation of a batch with device draws (include/liso_augment.h, liso_amd/datasets/batch_augmentation.py) against its
numpy restatement bit for bit, against the per-sweep kernels it shares its bodies with, per sample, through `BatchBoxAugmenter`, and
captured in a hipGraph.  Shapes: tests/batch_augment_cases.py (two 0.5 m grids, radius 4; three sweeps of up to 2048 rows; nine
snippets of 1 .. 1100 points)."""
import functools
import gc

import numpy as np
import pytest
import torch

from tests import batch_augment_cases as cases

pytestmark = pytest.mark.gpu

AMPLE = 15 * max(cases.SNIPPET_SIZES)
MODES = ("dropout", "raydrop", "all")


@pytest.fixture(scope="module", autouse=True)
def private_memory_pool():
    """Everything this module allocates on the device comes from a memory pool of its own, which goes back to the driver, zeroed, when
    the module is done: the caching allocator's shared free lists stay exactly as the module found them.  The outputs of this path
    are NaN behind their counts by contract and a freed block keeps its bytes; a later test that reads memory it never wrote
    (tests/test_gpu_conv_roles.py checks `isfinite` over the padding columns of a `torch.empty` statistics buffer, which the f32x3
    kernel leaves alone for 32 filters) depends on what lies in those lists, and on their layout."""
    if not torch.cuda.is_available():
        yield
        return
    pool = torch.cuda.MemPool()
    ctx = torch.cuda.use_mem_pool(pool)
    ctx.__enter__()
    try:
        yield
    finally:
        host_case.cache_clear()
        device_db.cache_clear()
        gc.collect()
        torch.cuda.synchronize()
        held = []
        for shift in range(26, 8, -1):  # 64 MiB ... 512 B: the allocator splits what is larger and rounds to 512 B
            for _ in range(4096):
                reserved = torch.cuda.memory_reserved()
                block = torch.zeros(1 << shift, dtype=torch.uint8, device="cuda")
                if torch.cuda.memory_reserved() > reserved:  # no free block of the pool was left for this size: it grew
                    break
                held.append(block)
        torch.cuda.synchronize()
        del held, block
        ctx.__exit__(None, None, None)
        del pool


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


@functools.lru_cache(maxsize=None)
def host_case(grid, mode, capacity, third="lattice", seed=None, calls=0):
    """the numpy restatement of one scenario, computed once and shared (read only).  `seed=None` with the small capacity: the first
    seed, found here on the CPU, at which some object is dropped whole and some object is pasted."""
    from liso_amd.datasets import batch_augmentation as BA

    grid_hw, range_xy = cases.GRIDS[grid]
    batch = cases.make_batch(grid_hw, range_xy, third)
    cfg = cases.make_cfg(grid_hw, range_xy, mode)
    db = cases.make_db("cpu")
    for s in ([seed] if seed is not None else range(40)):
        out = BA.paste_snippets_batch_host(db, batch["coors"], batch["counts"], cfg=cfg, seed=s, calls=calls, extra_capacity=capacity)
        state = out["draws"][..., 15]
        if seed is not None or capacity >= AMPLE or ((state == BA.SLOT_OVERFLOW).any() and (state == BA.SLOT_PASTED).any()):
            break
    else:
        raise AssertionError("no seed with an overflow and a pasted object")
    for v in out.values():
        v.setflags(write=False)
    return out, s


@functools.lru_cache(maxsize=None)
def device_db():
    return cases.make_db("cuda")


def device_batch(grid, third="lattice"):
    grid_hw, range_xy = cases.GRIDS[grid]
    b = cases.make_batch(grid_hw, range_xy, third)
    return {k: torch.from_numpy(v).cuda() for k, v in b.items()}, cases.make_cfg(grid_hw, range_xy, "dropout")


def run_device(grid, mode, capacity, seed, third="lattice", calls=0, samples=None):
    from liso_amd.datasets import batch_augmentation as BA

    grid_hw, range_xy = cases.GRIDS[grid]
    batch, _ = device_batch(grid, third)
    cfg = cases.make_cfg(grid_hw, range_xy, mode)
    draws = BA.DeviceDraws(seed, "cuda").reset(calls)
    sel = slice(None) if samples is None else samples
    ids = None if samples is None else torch.tensor(samples, dtype=torch.int64).cuda()
    out = BA.paste_snippets_batch(device_db(), batch["pcl"][sel], batch["counts"][sel], batch["coors"][sel], cfg=cfg, draws=draws,
                                  sample_ids=ids, extra_capacity=capacity)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, draws


def assert_equals_host(got, want, where=""):
    """every output of the call, bit for bit (`kept_rows` and nothing else is compared only up to each sample's count)"""
    for key in ("draws", "object_offsets", "extra_counts", "overflow", "box_valid", "box_pos", "box_dims", "box_rot", "box_velo",
                "extra_points", "extra_flow"):
        assert np.array_equal(bits(got[key]), bits(want[key])), (where, key)
    for b, n in enumerate(want["extra_counts"]):
        assert np.array_equal(got["kept_rows"][b, :n], want["kept_rows"][b, :n]), (where, "kept_rows", b)


@pytest.mark.parametrize("capacity", [AMPLE, 300])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("grid", ["square", "oblong"])
def test_device_equals_the_host_restatement(grid, mode, capacity):
    from liso_amd.datasets import batch_augmentation as BA

    want, seed = host_case(grid, mode, capacity)
    state = want["draws"][..., 15]
    assert (state == BA.SLOT_PASTED).any() and not want["box_valid"][2].any()  # (the lattice sweep has no free cell)
    if capacity == 300:
        assert (state == BA.SLOT_OVERFLOW).any() and want["overflow"].sum() > 0
    else:
        assert want["overflow"].sum() == 0 and want["extra_counts"].max() > 300
    got, draws = run_device(grid, mode, capacity, seed)
    assert_equals_host(got, want, (grid, mode, capacity, seed))
    assert draws.state.cpu().tolist() == [seed, 1]


@pytest.mark.parametrize("mode", ["dropout", "raydrop"])
def test_two_free_cells_on_the_device(mode):
    want, seed = host_case("square", mode, AMPLE, third="hole", seed=1)
    got, _ = run_device("square", mode, AMPLE, seed, third="hole")
    assert_equals_host(got, want, mode)
    k = int((want["draws"][2, :, 15] != 0).sum())
    assert int(got["box_valid"][2].sum()) == min(k, 2)


def test_samples_do_not_depend_on_their_batch():
    """sample b of the batch of three == the same cloud alone with sample_ids = [b] and the same state"""
    full, _ = run_device("oblong", "dropout", AMPLE, seed=5, calls=7)
    assert len({int(c) for c in full["extra_counts"]}) > 1
    for b in range(3):
        alone, _ = run_device("oblong", "dropout", AMPLE, seed=5, calls=7, samples=[b])
        for key, v in alone.items():
            n = full["extra_counts"][b] if key == "kept_rows" else None
            assert np.array_equal(bits(np.atleast_1d(v[0])[:n]), bits(np.atleast_1d(full[key][b])[:n])), (b, key)


@pytest.mark.parametrize("grid", ["square", "oblong"])
def test_batched_free_mask_equals_the_per_sweep_mask(grid):
    from liso_amd.datasets.batch_augmentation import free_location_mask_batch, free_mask_host
    from liso_amd.datasets.box_augmentation import free_location_mask

    grid_hw, _ = cases.GRIDS[grid]
    for third in ("lattice", "hole"):
        batch, _ = device_batch(grid, third)
        free, prefix = free_location_mask_batch(batch["coors"], batch["counts"], grid_hw, 4)
        for b in range(3):
            n = int(batch["counts"][b])
            f1, p1 = free_location_mask(batch["coors"][b, :n], grid_hw, 4)
            assert torch.equal(free[b], f1) and torch.equal(prefix[b], p1)
            assert np.array_equal(free[b].cpu().numpy().astype(bool), free_mask_host(batch["coors"][b, :n].cpu().numpy(), grid_hw, 4))
        assert int(prefix[1, -1]) == grid_hw[0] * grid_hw[1] and int(prefix[2, -1]) == (0 if third == "lattice" else 2)


@pytest.mark.parametrize("mode", MODES)
def test_drawn_parameters_through_the_per_sweep_kernels(mode):
    """cells, poses, source rows and flow draws of the batched call fed to `select_free_cells` / `paste_snippets`: the same cells, and
    bit-equal points, flow and box speeds (one set of bodies, box_augment_bodies.h)"""
    from liso_amd.datasets import batch_augmentation as BA
    from liso_amd.datasets.box_augmentation import free_location_mask, paste_snippets, select_free_cells

    grid = "oblong"
    grid_hw, range_xy = cases.GRIDS[grid]
    want, seed = host_case(grid, mode, AMPLE)
    got, _ = run_device(grid, mode, AMPLE, seed)
    batch, _ = device_batch(grid)
    db = device_db()
    p = BA.augment_params(cases.make_cfg(grid_hw, range_xy, mode))
    for b in range(2):
        pasted = np.flatnonzero(got["box_valid"][b])
        assert pasted.size
        n = int(batch["counts"][b])
        free, prefix = free_location_mask(batch["coors"][b, :n], grid_hw, 4)
        cells = got["draws"][b, pasted, 0].astype(np.int64)
        compact = np.searchsorted(np.flatnonzero(free.cpu().numpy().reshape(-1)), cells)  # the index among the free cells
        assert np.array_equal(select_free_cells(free, prefix, compact).cpu().numpy(), cells)
        offs = got["object_offsets"][b]
        total = int(got["extra_counts"][b])
        rows = got["kept_rows"][b, :total]
        flow_u = np.zeros((total, 3))
        for slot in pasted:
            lo, hi = offs[slot], offs[slot + 1]
            local = rows[lo:hi] - db.offsets[int(got["draws"][b, slot, 1])]
            flow_u[lo:hi] = np.stack([BA.draw_uniform(seed, 0, b, BA.P_FLOW, slot, 3 * local + c) for c in range(3)], -1)
        pts, flow, velo = paste_snippets(db, rows, offs[np.concatenate([pasted, [pasted[-1] + 1]])].astype(np.int64), want["pose"][b, pasted],
                                         flow_u, p["vmin"], p["vmax"])
        assert np.array_equal(bits(pts.cpu().numpy()), bits(got["extra_points"][b, :total]))
        assert np.array_equal(bits(flow.cpu().numpy()), bits(got["extra_flow"][b, :total]))
        assert np.array_equal(bits(velo.cpu().numpy()), bits(got["box_velo"][b, pasted]))


def test_append_clouds_puts_the_pasted_rows_behind_each_count():
    from liso_amd.datasets.batch_augmentation import append_clouds

    rs = np.random.default_rng(0)
    for cols in (4, 3):
        cloud = torch.from_numpy(rs.normal(size=(3, 70, cols)).astype(np.float32)).cuda()
        extra = torch.from_numpy(rs.normal(size=(3, 300, cols)).astype(np.float32)).cuda()
        counts = torch.tensor([70, 0, 13], dtype=torch.int32).cuda()
        extra_counts = torch.tensor([300, 257, 0], dtype=torch.int32).cuda()
        out, out_counts = append_clouds(cloud, counts, extra, extra_counts)
        assert out.shape == (3, 370, cols) and out_counts.tolist() == [370, 257, 13]
        for b, (n, e) in enumerate(zip(counts.tolist(), extra_counts.tolist())):
            assert torch.equal(out[b, :n], cloud[b, :n]) and torch.equal(out[b, n:n + e], extra[b, :e]) and out[b, n + e:].isnan().all()


def _augmenter_inputs(grid, third="lattice"):
    from liso_amd.datasets.sample_prep import assemble_bev_sample

    batch, cfg = device_batch(grid, third)
    rs = np.random.default_rng(3)
    flow = torch.from_numpy(rs.normal(size=(3, cases.N_MAX, 3)).astype(np.float32)).cuda()
    sample = assemble_bev_sample(batch["pcl"], batch["counts"], flow=flow, cfg=cfg)
    assert torch.equal(sample["counts"], batch["counts"])  # (every point of the scenario lies inside the grid)
    n = batch["counts"]
    sample["pcl_full_w_ground_ta"] = {"pcl": torch.cat([batch["pcl"], batch["pcl"][:, :40]], 1).contiguous(), "counts": n}
    sample["pcl_full_no_ground_ta"] = {"pcl": batch["pcl"].clone(), "counts": n}
    return sample, cfg, batch


def test_batch_box_augmenter_returns_the_reference_dictionary():
    from liso_amd.datasets import batch_augmentation as BA
    from liso_amd.datasets.label_prep import draw_heat_regression_maps
    from liso_amd.datasets.sample_prep import pillarize_bev
    from liso_amd.kabsch.shape_utils import Shape

    sample, cfg, batch = _augmenter_inputs("oblong")
    aug = BA.BatchBoxAugmenter(cfg, device_db(), need_flow=True, seed=4)
    aug.extra_capacity = 4000
    P = 2
    pre = Shape(pos=torch.rand(3, P, 3).cuda(), dims=torch.rand(3, P, 3).cuda() + 1, rot=torch.rand(3, P, 1).cuda(),
                probs=torch.ones(3, P, 1).cuda(), velo=torch.rand(3, P, 1).cuda(), valid=torch.tensor([[1, 1], [1, 0], [0, 0]]).bool().cuda())
    res = aug(sample, prediscovered_boxes=pre)
    want = BA.paste_snippets_batch_host(cases.make_db("cpu"), sample["pcl_ta"]["pillar_coors"].cpu().numpy(), batch["counts"].cpu().numpy(),
                                        cfg=cfg, seed=4, calls=0, extra_capacity=4000)
    e = want["extra_counts"]
    assert e[0] > 0 and e[1] > 0 and e[2] == 0 and np.array_equal(res["overflow"].cpu().numpy(), want["overflow"])
    # the three clouds: behind each count exactly the pasted rows
    n = batch["counts"].cpu().numpy()
    for key, src in (("pcl_full_w_ground_ta", sample["pcl_full_w_ground_ta"]["pcl"]), ("pcl_full_no_ground_ta", batch["pcl"])):
        out, cnt = res[key]["pcl"].cpu().numpy(), res[key]["counts"].cpu().numpy()
        assert np.array_equal(cnt, n + e)
        for b in range(3):
            assert np.array_equal(bits(out[b, :n[b]]), bits(src[b, :n[b]].cpu().numpy()))
            assert np.array_equal(bits(out[b, n[b]:cnt[b]]), bits(want["extra_points"][b, :e[b]])) and np.isnan(out[b, cnt[b]:]).all()
    # pcl_ta = pillarize_bev of the concatenation, the flow riding along
    cat = torch.full((3, cases.N_MAX + 4000, 4), float("nan")).cuda()
    cat_flow = torch.full((3, cases.N_MAX + 4000, 3), float("nan")).cuda()
    for b in range(3):
        cat[b, :n[b]], cat[b, n[b]:n[b] + e[b]] = batch["pcl"][b, :n[b]], torch.from_numpy(want["extra_points"][b, :e[b]]).cuda()
        cat_flow[b, :n[b]], cat_flow[b, n[b]:n[b] + e[b]] = sample["flow_ta_tb"][b, :n[b]], torch.from_numpy(want["extra_flow"][b, :e[b]]).cuda()
    crop = pillarize_bev(cat, torch.from_numpy(n + e).cuda(), bev_range_m=cfg.data.bev_range_m, img_grid_size=cfg.data.img_grid_size, flow=cat_flow)
    assert torch.equal(res["counts"], crop["counts"]) and torch.equal(res["pcl_ta"]["pillar_coors"], crop["pillar_coors"])
    for b in range(3):
        c = int(crop["counts"][b])
        assert torch.equal(res["pcl_ta"]["pcl"][b, :c], crop["pcl"][b, :c]) and torch.equal(res["slim_flow"]["flow_ta_tb"][b, :c], crop["flow"][b, :c])
    # boxes: K pasted slots, then the prediscovered ones
    boxes = res["gt"]["boxes"]
    K = 15
    assert boxes.valid.shape == (3, K + P) and res["mined"]["boxes"] is boxes
    assert np.array_equal(boxes.valid[:, :K].cpu().numpy(), want["box_valid"].astype(bool)) and torch.equal(boxes.valid[:, K:], pre.valid)
    assert np.array_equal(bits(boxes.pos[:, :K].cpu().numpy()), bits(want["box_pos"])) and torch.equal(boxes.pos[:, K:], pre.pos)
    assert np.array_equal(bits(boxes.velo[:, :K, 0].cpu().numpy()), bits(want["box_velo"])) and torch.equal(boxes.velo[:, K:], pre.velo)
    assert np.array_equal(bits(boxes.rot[:, :K, 0].cpu().numpy()), bits(want["box_rot"])) and bool((boxes.probs == 1).all())
    assert res["mined"]["prediscovered_boxes"] is pre
    maps = draw_heat_regression_maps(boxes, aug.centermaps_output_grid_size, np.array(cfg.data.bev_range_m, np.float32), cfg.box_prediction)
    for k, v in maps.items():
        assert torch.equal(res["mined"][f"centermaps_{k}"], v), k
    assert bool(res["mined"]["centermaps_center_bool_mask"].any())


def _kernel_launches(fn):
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return len([e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower()])


def test_captured_call_draws_afresh_on_every_replay():
    from liso_amd.datasets import batch_augmentation as BA
    from liso_amd.utils import graph_capture

    grid, mode, seed = "square", "dropout", 21
    grid_hw, range_xy = cases.GRIDS[grid]
    cfg = cases.make_cfg(grid_hw, range_xy, mode)
    batch, _ = device_batch(grid)
    draws = BA.DeviceDraws(seed, "cuda")
    ids = torch.arange(3, dtype=torch.int64).cuda()
    body = lambda: BA.paste_snippets_batch(device_db(), batch["pcl"], batch["counts"], batch["coors"], cfg=cfg, draws=draws,  # noqa: E731
                                           sample_ids=ids, extra_capacity=AMPLE)
    stream = torch.cuda.Stream()
    graph, out = graph_capture.capture(body, stream, warm_ups=2)
    torch.cuda.synchronize()
    draws.reset()
    replays = []
    with torch.cuda.stream(stream):
        for _ in range(2):
            graph.replay()
            stream.synchronize()
            replays.append({k: v.cpu().numpy() for k, v in out.items()})
    for call, got in enumerate(replays):
        assert_equals_host(got, host_case(grid, mode, AMPLE, seed=seed, calls=call)[0], f"replay {call}")
    assert not np.array_equal(replays[0]["draws"], replays[1]["draws"])
    assert draws.state.cpu().tolist() == [seed, 2]
    # the launch count does not depend on the batch size
    one = lambda: BA.paste_snippets_batch(device_db(), batch["pcl"][:1], batch["counts"][:1], batch["coors"][:1], cfg=cfg, draws=draws,  # noqa: E731
                                          sample_ids=ids[:1], extra_capacity=AMPLE)
    one()
    n3, n1 = _kernel_launches(body), _kernel_launches(one)
    assert n3 == n1 == 6, (n3, n1)


def test_adopted_database_keeps_its_device_rows():
    """`BoxSnippetDb.from_device` with the LiDAR rows on the device: `device_tables` hands the same rows on (no second upload), and
    the ray-drop call through the adopted database equals the one through the uploaded database"""
    from liso_amd.datasets.box_augmentation import BoxSnippetDb

    db = device_db()
    rows = torch.from_numpy(np.concatenate(db.lidar_rows).astype(np.int32)).cuda()
    adopted = BoxSnippetDb.from_device(db.points, db.offsets, db.boxes, lidar_rows=rows)
    tables = adopted.device_tables()
    assert tables["lidar_rows"].data_ptr() == rows.data_ptr() and adopted.device_tables() is tables
    assert torch.equal(tables["offsets"], db.device_tables()["offsets"]) and torch.equal(tables["pos_z"], db.device_tables()["pos_z"])
    want, seed = host_case("square", "raydrop", AMPLE)
    from liso_amd.datasets import batch_augmentation as BA

    batch, _ = device_batch("square")
    cfg = cases.make_cfg(*cases.GRIDS["square"], "raydrop")
    got = BA.paste_snippets_batch(adopted, batch["pcl"], batch["counts"], batch["coors"], cfg=cfg, draws=BA.DeviceDraws(seed, "cuda"),
                                  extra_capacity=AMPLE)
    assert_equals_host({k: v.cpu().numpy() for k, v in got.items()}, want, "adopted")
