"""LisoLoopTrainer(share_voxelisation=True): every sweep is voxelised once -- stage A's inference puts both sweeps of its pairs through
one pillar-encoder call and the detector step reads its clouds' rows out of that voxelisation.  Losses, mined boxes and the detector's
parameters are those of the switch turned off, bit for bit; where the conditions for sharing do not hold the step voxelises for
itself as before."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GRID, RANGE_M, STEPS = 256, 50.0, 5
_CACHE = {}


def _pairs():
    if "pairs" not in _CACHE:
        from liso_amd.datasets.synthetic import slim_pair

        _CACHE["pairs"] = [slim_pair(31 + i, torch.device("cuda"), n_points=40000, grid=GRID, bev_range_m=RANGE_M) for i in range(6)]
    return _CACHE["pairs"]


def _run(share, ground=False, announce=True):
    """5 steps of batch 2 around a ring of 6 pairs (the settings of test_gpu_liso_loop's batched pipeline test) -> losses, mined boxes,
    the detector's state and the trainer's counters; one run per setting, kept for the tests that compare against it"""
    key = (share, ground, announce)
    if key in _CACHE:
        return _CACHE[key]
    from liso_amd.trainer import LisoLoopTrainer
    from liso_amd.utils.config import apply_slim_simple_knn_training, default_cfg

    dev, pairs = torch.device("cuda"), _pairs()
    cfg = apply_slim_simple_knn_training(default_cfg(grid=GRID, bev_range_m=RANGE_M))
    cfg.data.use_ground_for_network = ground
    torch.manual_seed(0)
    tr = LisoLoopTrainer(cfg, dev, compute_dtype=torch.bfloat16, total_steps=20, use_graph=True, overlap=True, infer_batch=2, flow_ahead=1,
                         share_voxelisation=share)
    assert tr.share_voxelisation is share
    losses, boxes = [], []
    for i in range(STEPS):
        cur = [pairs[(2 * i + k) % 6] for k in range(2)]
        up = [pairs[(2 * i + k) % 6] for k in range(2, 6)] if announce else ()
        losses.append(float(tr.step_batch(cur, upcoming=up)))
        for b in tr.last_boxes_batch:
            allb = torch.cat([b.pos.float(), b.dims.float(), b.rot.float(), b.velo.float()], dim=-1)
            boxes.append(allb[b.valid].cpu())
    torch.cuda.synchronize()
    _CACHE[key] = {"losses": losses, "boxes": boxes, "state": {k: v.detach().clone() for k, v in tr.detector.net.state_dict().items()},
                   "replays": tr.stage_a_replays, "voxelisations": tr.stage_a_voxelisations, "shared_steps": tr.shared_prep_steps}
    return _CACHE[key]


def _assert_same_training(a, b):
    assert a["losses"] == b["losses"], (a["losses"], b["losses"])
    assert len(a["boxes"]) == len(b["boxes"]) == 2 * STEPS
    for x, y in zip(a["boxes"], b["boxes"]):
        assert x.shape == y.shape and torch.equal(x, y)
    assert a["state"].keys() == b["state"].keys()
    for k, v in a["state"].items():
        assert torch.equal(v, b["state"][k]), k
    assert a["losses"][-1] != a["losses"][0] and sum(x.shape[0] for x in a["boxes"]) > 0  # (it trained, on boxes)


def test_shared_voxelisation_trains_exactly_as_separate_voxelisations():
    off, on = _run(share=False), _run(share=True)
    _assert_same_training(on, off)
    # switch off: two encoder calls per inference, the detector never reads them
    assert off["replays"] > 0 and off["voxelisations"] == 2 * off["replays"] and off["shared_steps"] == 0
    # switch on: ONE voxelisation per inference replay; the first step is not announced and infers for itself, the second finds the
    # rows that were prepared for it before any inference had run -- from the third on the pipeline is full and every step shares
    assert on["replays"] == off["replays"] and on["voxelisations"] == on["replays"]
    assert on["shared_steps"] == STEPS - 2


def test_unannounced_pairs_fall_back_to_their_own_voxelisation():
    off, alone = _run(share=False), _run(share=True, announce=False)
    _assert_same_training(alone, off)
    assert alone["shared_steps"] == 0 and alone["replays"] == 0  # (nothing ran ahead: every step infers and voxelises in line)


def test_network_clouds_with_ground_are_never_shared():
    """data.use_ground_for_network: SLIM reads `pcl_full_w_ground_ta`, the detector `pcl_full_no_ground_ta` -- other clouds, so the
    detector voxelises its own; SLIM's two sweeps still go through one call"""
    off, on = _run(share=False, ground=True), _run(share=True, ground=True)
    _assert_same_training(on, off)
    assert on["shared_steps"] == 0 and off["shared_steps"] == 0
    assert on["replays"] == off["replays"] > 0 and on["voxelisations"] == on["replays"] and off["voxelisations"] == 2 * off["replays"]
