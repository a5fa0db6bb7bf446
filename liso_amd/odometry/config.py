"""`KISSConfig`: the parameters of the odometry under the names and defaults of kiss_icp's configuration object, so that
`kiss_config = KISSConfig(); kiss_config.mapping.voxel_size = 0.01 * kiss_config.data.max_range` (create_kitti_raw.py:74-76) works
unchanged."""
import dataclasses
from typing import Optional


@dataclasses.dataclass
class DataConfig:
    max_range: float = 100.0
    min_range: float = 5.0
    deskew: bool = False  # only False is supported


@dataclasses.dataclass
class MappingConfig:
    voxel_size: Optional[float] = None  # None -> 0.01 * max_range
    max_points_per_voxel: int = 20


@dataclasses.dataclass
class AdaptiveThresholdConfig:
    initial_threshold: float = 2.0
    min_motion_th: float = 0.1


@dataclasses.dataclass
class RegistrationConfig:
    max_num_iterations: int = 500
    convergence_criterion: float = 1e-4


@dataclasses.dataclass
class KISSConfig:
    data: DataConfig = dataclasses.field(default_factory=DataConfig)
    mapping: MappingConfig = dataclasses.field(default_factory=MappingConfig)
    adaptive_threshold: AdaptiveThresholdConfig = dataclasses.field(default_factory=AdaptiveThresholdConfig)
    registration: RegistrationConfig = dataclasses.field(default_factory=RegistrationConfig)

    def params(self):
        """the flat keyword arguments `lidar_odometry` and `lidar_odometry_host` take"""
        return dict(max_range=self.data.max_range, min_range=self.data.min_range, deskew=self.data.deskew,
                    voxel_size=self.mapping.voxel_size, max_points_per_voxel=self.mapping.max_points_per_voxel,
                    initial_threshold=self.adaptive_threshold.initial_threshold, min_motion_th=self.adaptive_threshold.min_motion_th,
                    max_num_iterations=self.registration.max_num_iterations,
                    convergence_criterion=self.registration.convergence_criterion)


DEFAULTS = KISSConfig().params()


def resolve_params(**params):
    """the parameters with their defaults filled in and `voxel_size=None` resolved to 0.01 * max_range; an unknown name, `deskew=True`
    or a value outside its range raises"""
    unknown = set(params) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown odometry parameters {sorted(unknown)}; known: {sorted(DEFAULTS)}")
    p = dict(DEFAULTS, **params)
    if p.pop("deskew"):
        raise NotImplementedError("deskew=True is not supported: the sweeps carry no per-point timestamps here")
    p["max_range"], p["min_range"] = float(p["max_range"]), float(p["min_range"])
    p["voxel_size"] = 0.01 * p["max_range"] if p["voxel_size"] is None else float(p["voxel_size"])
    p["max_points_per_voxel"], p["max_num_iterations"] = int(p["max_points_per_voxel"]), int(p["max_num_iterations"])
    for k in ("initial_threshold", "min_motion_th", "convergence_criterion"):
        p[k] = float(p[k])
    if not (p["max_range"] > p["min_range"] >= 0.0 and p["voxel_size"] > 0.0 and 1 <= p["max_points_per_voxel"] <= 20
            and p["max_num_iterations"] >= 1 and p["initial_threshold"] > 0.0 and p["min_motion_th"] >= 0.0
            and p["convergence_criterion"] > 0.0):
        raise ValueError(f"odometry parameters out of range: {p}")
    return p
