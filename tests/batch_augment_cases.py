"""Scenarios shared by the host and the GPU tests of the batched box-snippet augmentation (no tests in here): the configuration,
the nine-snippet database and the three-sweep batch with its lattice variants."""
import numpy as np
import torch

SNIPPET_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1100)
GRIDS = {"square": ((64, 64), (32.0, 32.0)), "oblong": ((48, 80), (24.0, 40.0))}  # both: 0.5 m cells, dilation radius 4
N_MAX = 2048


def make_cfg(grid_hw, range_xy, mode, max_num_objs=15, network="centerpoint"):
    """mode: "dropout" (the reference's shipped block), "raydrop" or "all" """
    from liso_amd.utils.config import default_cfg, to_attr

    cfg = default_cfg()
    cfg.data.bev_range_m, cfg.data.img_grid_size = tuple(range_xy), tuple(grid_hw)
    cfg.data.limit_pillar_height = False
    cfg.data.flow_source, cfg.data.train_on_box_source = "slim_flow", "mined"
    cfg.network.name = network
    cfg.data.augmentation = to_attr({"boxes": {
        "active": True, "max_num_objs": max_num_objs, "min_artificial_obj_velo": 1.0, "max_artificial_obj_velo": 3.0,
        "max_scale_delta": 0.2, "max_points_dropout": 0.25 if mode == "dropout" else 0.0, "use_raydrop_augm": mode == "raydrop"}})
    return cfg


def make_db(device, sizes=SNIPPET_SIZES, seed=11):
    from liso_amd.datasets.box_augmentation import BoxSnippetDb
    from liso_amd.kabsch.shape_utils import Shape

    rs = np.random.default_rng(seed)
    M = len(sizes)
    pcls = [np.concatenate([rs.uniform(-2, 2, (n, 3)), rs.uniform(0, 1, (n, 1))], -1).astype(np.float32) for n in sizes]
    rows = [rs.integers(0, 64, n).astype(np.int32) for n in sizes]
    boxes = Shape(pos=torch.from_numpy(rs.uniform(-1.5, -0.5, (M, 3)).astype(np.float32)),
                  dims=torch.from_numpy(rs.uniform(1.0, 4.0, (M, 3)).astype(np.float32)), rot=torch.zeros(M, 1), probs=torch.ones(M, 1))
    return BoxSnippetDb({"pcl_in_box_cosy": pcls, "boxes": boxes, "lidar_rows": rows}, device)


def _lattice(grid_hw):
    H, W = grid_hw
    return np.stack(np.meshgrid(np.arange(1, H, 4), np.arange(1, W, 4), indexing="ij"), -1).reshape(-1, 2)


def lattice_with_two_free_cells(grid_hw, radius=4):
    """the spacing-4 lattice (which leaves no free cell at radius 4) with a 2 x 2 block of its points taken out, and as many single
    occupied cells put back around the hole as it takes to leave exactly the two cells `keep` free"""
    H, W = grid_hw
    i0, j0 = 1 + 4 * (H // 8), 1 + 4 * (W // 8)
    cells = [tuple(c) for c in _lattice(grid_hw) if not (c[0] in (i0, i0 + 4) and c[1] in (j0, j0 + 4))]
    keep = [(i0 + 2, j0 + 2), (i0 + 2, j0 + 3)]

    def free_now():
        from liso_amd.datasets.batch_augmentation import free_mask_host

        return [tuple(c) for c in np.argwhere(free_mask_host(np.array(cells), grid_hw, radius))]

    r2 = radius * radius
    for _ in range(64):
        others = [f for f in free_now() if f not in keep]
        if not others:
            break
        best, best_n = None, 0
        for ci in range(i0 - 8, i0 + 13):
            for cj in range(j0 - 8, j0 + 13):
                if not (0 <= ci < H and 0 <= cj < W) or any((ci - a) ** 2 + (cj - b) ** 2 <= r2 for a, b in keep):
                    continue
                n = sum((ci - a) ** 2 + (cj - b) ** 2 <= r2 for a, b in others)
                if n > best_n:
                    best, best_n = (ci, cj), n
        assert best is not None, others
        cells.append(best)
    assert sorted(free_now()) == sorted(keep), free_now()
    return np.array(cells), keep


def cell_points(cells, grid_hw, range_xy, rs, jitter=0.3):
    """one point in each given cell: centre + a jitter well inside the cell; z and intensity random"""
    cells = np.asarray(cells).reshape(-1, 2)
    size = np.array(range_xy) / np.array(grid_hw)
    xy = (cells + 0.5 + rs.uniform(-jitter, jitter, cells.shape)) * size - 0.5 * np.array(range_xy)
    return np.concatenate([xy, rs.uniform(-1.5, 0.5, (cells.shape[0], 1)), rs.uniform(0, 1, (cells.shape[0], 1))], -1).astype(np.float32)


def make_batch(grid_hw, range_xy, third="lattice", seed=5):
    """-> dict(pcl float32 [3, N_MAX, 4] (NaN behind the count), coors int32 [3, N_MAX, 2] (-1 behind the count), counts int32 [3]):
    ~1500 points in one quadrant; an empty sweep; the spacing-4 lattice from cell 1 (`third="lattice"`: no free cell at radius 4)
    or that lattice with a hole that leaves exactly two free cells (`third="hole"`)"""
    H, W = grid_hw
    rs = np.random.default_rng(seed)
    quadrant = np.stack([rs.integers(0, H // 2, 1500), rs.integers(W // 2, W, 1500)], -1)
    lattice = _lattice(grid_hw) if third == "lattice" else lattice_with_two_free_cells(grid_hw)[0]
    pcl = np.full((3, N_MAX, 4), np.nan, np.float32)
    coors = np.full((3, N_MAX, 2), -1, np.int32)
    counts = np.zeros(3, np.int32)
    for b, cells in ((0, quadrant), (2, lattice)):
        counts[b] = cells.shape[0]
        pcl[b, :counts[b]] = cell_points(cells, grid_hw, range_xy, rs)
        coors[b, :counts[b]] = cells
    return {"pcl": pcl, "coors": coors, "counts": counts}
