"""The mined-box database on disk: `load_mined_boxes_db` (mirror of liso/tracker/mined_box_db_utils.py) and `save_mined_box_db`
(mirror of liso/tracker/tracking.py:1927-1962).  The database is what `MinedTracks.to_dict` (liso_amd/tracker/track_mining.py)
returns: {sample name: {"lidar_T_box": float64 [n,4,4], "raw_box": the `__dict__` of a numpy Shape [n], "track_id": int64 [n]}} and
{sample name: {"max_confidence": float, "num_boxes": int}}."""
from pathlib import Path

import numpy as np
import yaml


def load_mined_boxes_db(path_to_mined_boxes_db):
    """a `.npy` file holds the pickled dict itself, anything else (`tracked.npz`) holds it as `arr_0`"""
    print(f"Loading mined_boxes_db from {path_to_mined_boxes_db}")
    if Path(path_to_mined_boxes_db).as_posix().endswith(".npy"):
        mined_boxes_db = np.load(path_to_mined_boxes_db, allow_pickle=True).item()
    else:
        mined_boxes_db = np.load(path_to_mined_boxes_db, allow_pickle=True)["arr_0"].item()
    total = sum(el["raw_box"]["pos"].shape[0] for el in mined_boxes_db.values())
    print(f"Loaded {total} mined boxes for {len(mined_boxes_db)} point clouds from db at {path_to_mined_boxes_db}")
    return mined_boxes_db


def _plain(value):
    """configuration entries as yaml's safe dumper takes them: dicts (attribute dicts included), lists, plain scalars"""
    if isinstance(value, dict):
        return {str(k): _plain(v) for k, v in value.items()}
    if isinstance(value, (list, tuple)):
        return [_plain(v) for v in value]
    if isinstance(value, np.generic):
        return value.item()
    if isinstance(value, Path):
        return value.as_posix()
    return value


def save_mined_box_db(tracking_cfg, export_raw_tracked_detections_to, tracked_boxes_conf_stats, tracked_boxes_db, mined_objects_target_paths):
    """writes `tracking_cfg.yaml`, `tracked_box_stats.yaml` and `tracked.npz` into the directory and puts the path of the last into
    mined_objects_target_paths["tracked"]"""
    target = Path(export_raw_tracked_detections_to)
    target.mkdir(exist_ok=True, parents=True)
    with open(target / "tracking_cfg.yaml", "w") as outfile:
        yaml.safe_dump(_plain(tracking_cfg), outfile)
    with open(target / "tracked_box_stats.yaml", "w") as outfile:
        yaml.safe_dump(_plain(tracked_boxes_conf_stats), outfile)
    db_target_pth = target / "tracked"
    save_str = "Overwrote" if db_target_pth.with_suffix(".npz").exists() else "Saving"
    np.savez_compressed(db_target_pth, tracked_boxes_db)
    mined_objects_target_paths["tracked"] = db_target_pth.with_suffix(".npz")
    print(f"{save_str} box db with {len(tracked_boxes_db)} entries to {db_target_pth}!")
