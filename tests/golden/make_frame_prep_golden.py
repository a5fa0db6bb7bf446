"""Generates tests/golden/frame_prep_reference.npz: the per-frame body of track_boxes_on_data_sequence between NMS and the tracker's
update (liso/tracker/tracking.py:745-1017) run frame by frame on the CPU with the reference's own functions, on the sequences of
tests/frame_prep_cases.py under each of its configurations:
  liso.kabsch.shape_utils.is_boxes_clearly_in_bev_range                      (:549-560)
  liso.datasets.torch_dataset_commons.get_points_in_boxes_mask               (:1902-1935)
  liso.eval.eval_ours.count_box_points_in_kitti_annotated_fov                (:96-116)
  liso.networks.flow_cluster_detector.flow_cluster_detector.fit_bev_box_z_and_height_using_points_in_box (:339-384)
  liso.tracker.tracking.propagate_boxes_forward_using_flow                   (:2168-2211)
  liso.kabsch.shape_utils.soft_align_box_flip_orientation_with_motion_trafo  (:608-644), extract_motion_in_pred_box_coordinates (:563-580)
  liso.kabsch.shape_utils.Shape.get_points_in_box_bool_mask                  (:488-538, the count behind the flow mean)
shape_utils and torch_dataset_commons are imported with their absent third-party imports stubbed (make_targets_golden.import_with_stubs);
tracking.py, eval_ours.py and flow_cluster_detector.py cannot be imported here, so the three functions needed from them are compiled at
generation time from the files' own text (make_tracking_golden.function_from_reference_file).  The reference's code is executed where it
lies; only arrays are stored.  The order of the steps and the conditions around them (:745-748, :769, :817-835, :942-979) are restated
in `run_frame` below.  The generator asserts the conditions under which the reference alone decides every case
(frame_prep_cases.MARGINS, through the host restatement's margins).
Run in the build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_frame_prep_golden.py
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_targets_golden import import_with_stubs  # noqa: E402  (also puts the reference on sys.path)
from make_tracking_golden import function_from_reference_file  # noqa: E402

import frame_prep_cases as FC  # noqa: E402

REF = "/root/reference/liso/"
FLOAT_KEYS = ("boxes", "rot", "conf", "velo", "into_prev", "into_next", "mean_flow")


def reference_functions():
    def _imp():
        from liso.datasets.torch_dataset_commons import get_points_in_boxes_mask
        from liso.kabsch import shape_utils
        from liso.utils.torch_transformation import homogenize_pcl
        return get_points_in_boxes_mask, shape_utils, homogenize_pcl

    get_points_in_boxes_mask, su, homogenize_pcl = import_with_stubs(_imp)
    propagate = function_from_reference_file(REF + "tracker/tracking.py", "propagate_boxes_forward_using_flow",
                                             {"torch": torch, "Shape": su.Shape, "extract_box_motion_transform_without_sensor_odometry":
                                              su.extract_box_motion_transform_without_sensor_odometry})
    fit_z = function_from_reference_file(REF + "networks/flow_cluster_detector/flow_cluster_detector.py",
                                         "fit_bev_box_z_and_height_using_points_in_box", {"torch": torch, "np": np, "Shape": su.Shape})
    count_fov = function_from_reference_file(REF + "eval/eval_ours.py", "count_box_points_in_kitti_annotated_fov",
                                             {"torch": torch, "np": np, "Shape": su.Shape, "fit_bev_box_z_and_height_using_points_in_box": fit_z})
    return dict(mask=get_points_in_boxes_mask, su=su, homog=homogenize_pcl, propagate=propagate, count_fov=count_fov)


def run_frame(R, sc, t, cfg):
    """one frame as tracking.py:745-1017 treats it -> dict of per-box arrays of the boxes that reach the tracker, plus the drop counts"""
    su = R["su"]
    nb, n, m = int(sc["n_box"][t]), int(sc["counts"][t]), int(sc["fov_counts"][t])
    b = torch.from_numpy(sc["boxes"][t, :nb].copy())
    pred = su.Shape(pos=b[:, :3], dims=b[:, 3:6], rot=b[:, 6:7], probs=torch.from_numpy(sc["conf"][t, :nb].copy())[:, None])
    src = torch.arange(nb)
    pcl = torch.from_numpy(sc["clouds"][t, :n].copy())
    dropped_bev = dropped_points = 0
    if pred.shape[0] > 0 and cfg["drop_boxes_on_bev_boundaries"]:  # :745-767
        ok = su.is_boxes_clearly_in_bev_range(pred, bev_range_m=torch.tensor(cfg["bev_range_m"]))
        pred.valid, src, dropped_bev = ok, src[ok], int((~ok).sum())
        pred = pred.drop_padding_boxes()
    if pred.shape[0] > 0 and cfg["min_points_in_box"] > 0:  # :769-815
        num = R["mask"](pred.clone(), R["homog"](pcl[:, :3])).sum(dim=0)
        ok = num >= cfg["min_points_in_box"]
        pred.valid, src, dropped_points = ok, src[ok], int((~ok).sum())
        pred = pred.drop_padding_boxes()
    k = pred.shape[0]
    out = {"src": src.numpy().astype(np.int32), "dropped_bev": dropped_bev, "dropped_points": dropped_points,
           "conf": pred.probs[:, 0].numpy().copy()}
    if k == 0:
        return out
    fov_min = cfg.get("fov_min_points", cfg["min_points_in_box"])
    in_fov = R["count_fov"](pred.clone(), torch.from_numpy(sc["fov_clouds"][t, :m].copy())) >= fov_min  # :825-831
    out["in_fov"] = in_fov.numpy().astype(np.uint8)
    out["raw_yaw"] = pred.rot[:, 0].numpy().copy()
    pred = pred[None]
    odom = torch.from_numpy(sc["odom"][t].copy())
    cloud, valid = pcl[None, :, :3], torch.from_numpy(sc["point_valid"][t, :n].copy())[None].bool()
    flow = torch.from_numpy(sc["flow"][t, :n].copy())[None]
    fg, _, bg, _, into_next = R["propagate"](pred, cloud, valid, pointwise_flow_ta_tb=flow, odom_t0_t1=odom, device="cpu")  # :942-955
    _, _, _, _, into_prev = R["propagate"](pred, cloud, valid, pointwise_flow_ta_tb=-1.0 * flow, odom_t0_t1=torch.linalg.inv(odom),
                                           device="cpu")  # :957-970
    out["n_points"] = pred.get_points_in_box_bool_mask(cloud).sum(dim=1)[0].numpy().astype(np.int32)
    out["mean_flow"] = fg[0, :, :3, 3].numpy().astype(np.float32)  # (the fp32 mean, widened by the reference: the cast is exact)
    assert (out["mean_flow"].astype(np.float64) == fg[0, :, :3, 3].numpy()).all()
    if cfg["align_predicted_boxes_using_flow"] and not cfg.get("is_flow_cluster_detector", False):  # :972-979
        trans, _ = su.extract_motion_in_pred_box_coordinates(pred, fg, bg)
        out["box_translation"] = trans[0].numpy().copy()
        pred = su.soft_align_box_flip_orientation_with_motion_trafo(boxes=pred, fg_kabsch_trafos=fg, bg_kabsch_trafo=bg)
    pred = pred[0]
    out["rot"] = pred.rot[:, 0].numpy().astype(np.float64)
    velo = pred.velo.numpy().astype(np.float64)
    out["velo"] = velo if velo.shape[-1] == 3 else np.zeros((k, 3))  # (a Shape's default velo is one zero per box)
    out["boxes"] = np.concatenate([pred.pos.numpy(), pred.dims.numpy(), out["rot"][:, None].astype(np.float32)], -1)
    out["into_next"], out["into_prev"] = into_next[0].numpy(), into_prev[0].numpy()
    return out


def run_scene(R, name, cfg_name):
    """-> the tables of `TrackerFrames` for one sequence with cap = its P, as the reference fills them"""
    from liso_amd.tracker.frame_prep import prepare_tracker_frames_host

    sc, cfg = FC.scene(name), FC.config(cfg_name)
    t_max, p = FC.SHAPES[name]
    single = {k: v[None] for k, v in sc.items() if k != "n_frames"}
    single["n_frames"] = np.array([sc["n_frames"]], np.int32)
    host = prepare_tracker_frames_host(*FC.args_of(single), cap=p, **cfg, **FC.MARGINS)  # raises unless the reference decides every case
    res = {k: np.zeros_like(v[0]) for k, v in host.items() if k != "overflow"}
    res["src"][:] = -1
    res["raw_yaw"], res["box_translation"] = np.zeros((t_max, p), np.float32), np.zeros((t_max, p, 3))
    for t in range(sc["n_frames"]):
        fr = run_frame(R, sc, t, cfg)
        k = len(fr["src"])
        res["n_det"][t], res["dropped_bev"][t], res["dropped_points"][t] = k, fr["dropped_bev"], fr["dropped_points"]
        for key, v in fr.items():
            if key not in ("dropped_bev", "dropped_points"):
                res[key][t, :k] = v
    for key in ("n_det", "src", "in_fov", "n_points", "dropped_bev", "dropped_points"):  # the restatement and the reference agree
        assert (res[key] == host[key][0]).all(), (name, cfg_name, key)
    return res


def main():
    R = reference_functions()
    out = {}
    for name in ("A", "B", "W"):
        out[f"{name}_checksum"] = np.float64(FC.checksum(name))
        for cfg_name in FC.CONFIGS:
            for key, v in run_scene(R, name, cfg_name).items():
                out[f"{name}_{cfg_name}_{key}"] = v
    path = os.path.join(HERE, "frame_prep_reference.npz")
    np.savez_compressed(path, **out)
    print({k: (v.shape, v.dtype) for k, v in out.items() if k.startswith("A_filter")})
    print(os.path.getsize(path) / 1e3, "kB")


if __name__ == "__main__":
    main()
