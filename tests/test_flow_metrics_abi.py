"""CPU: the scene-flow metrics modules import (also under the reference's names), and their argument checks refuse bad inputs
before anything is launched (include/liso_flow_metrics.h)."""
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _lib():
    from liso_amd import _lib as L

    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return L


def test_modules_import():
    m = importlib.import_module("liso_amd.slim.utils.metrics")
    f = importlib.import_module("liso_amd.eval.flow_metrics")
    v = importlib.import_module("liso_amd.slim.validation")
    for name in ("get_ratio_for_thresh", "get_inlier_outlier_ratios", "compute_scene_flow_metrics_for_points_in_this_mask",
                 "aggregate_metrics"):
        assert callable(getattr(m, name))
    assert callable(f.FlowMetrics) and callable(v.run_eval_on_this_dataset)
    from liso_amd.slim.model.slim import SLIM
    from liso_amd.trainer import SlimTrainer

    assert callable(SLIM.infer_eval_flows) and callable(SlimTrainer.eval_model)
    from liso_amd.datasets.synthetic import slim_val_batch

    assert callable(slim_val_batch)


def test_reference_names_resolve_under_install_as():
    code = ("import liso_amd; liso_amd.install_as('liso')\n"
            "import liso.slim.utils.metrics as m, liso.eval.flow_metrics as f\n"
            "import liso_amd.slim.utils.metrics as m2, liso_amd.eval.flow_metrics as f2\n"
            "assert m is m2 and f is f2 and f.FlowMetrics is f2.FlowMetrics\n"
            "from liso.slim.utils.metrics import aggregate_metrics, compute_scene_flow_metrics_for_points_in_this_mask\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


def test_result_layout_matches_the_header():
    L = _lib()
    from liso_amd.eval.flow_metrics import RESULT_DTYPE

    lib = L.lib()
    assert lib.liso_flow_metrics_result_bytes() == RESULT_DTYPE.itemsize == 4000
    assert lib.liso_flow_metrics_state_bytes() >= RESULT_DTYPE.itemsize


def test_c_abi_refuses_bad_arguments_before_launching():
    L = _lib()
    lib = L.lib()
    buf = ctypes.create_string_buffer(64 + 16)
    addr = ctypes.addressof(buf)
    st = ctypes.c_void_p((addr + 15) // 16 * 16)  # (an aligned address; every call below returns before touching it)
    dummy = st
    edges33 = (ctypes.c_double * 34)(*range(34))
    edges3 = (ctypes.c_double * 3)(0.0, 1.0, 2.0)

    def upd(state=st, rows=10, pts=dummy, pst=4, gt=dummy, gst=3, nf=1, p0=dummy, s0=3, valid=dummy, mov=dummy, edges=edges3, nb=2):
        return lib.liso_flow_metrics_update(state, rows, pts, pst, gt, gst, nf, p0, s0, None, 0, None, 0, valid, mov, None,
                                            ctypes.cast(edges, ctypes.c_void_p) if edges is not None else None, nb, None, None)

    assert upd(nb=33, edges=edges33) == -1           # more than 32 bins
    assert upd(nb=-1) == -1
    assert upd(edges=None) == -1                     # bins without edges
    assert upd(state=None) == -1
    assert upd(state=ctypes.c_void_p(st.value + 4)) == -1  # misaligned state
    assert upd(rows=-1) == -1
    assert upd(nf=0) == -1 and upd(nf=4) == -1
    assert upd(nf=2) == -1                           # second flow missing
    assert upd(gt=None) == -1 and upd(p0=None) == -1 and upd(valid=None) == -1 and upd(mov=None) == -1
    assert upd(gst=2) == -1 and upd(s0=2) == -1 and upd(pst=2) == -1
    assert upd(pts=None) == -1                       # range bins need the points
    bad = (ctypes.c_double * 3)(0.0, 2.0, 1.0)
    assert upd(edges=bad) == -1                      # decreasing edges
    nan = (ctypes.c_double * 3)(0.0, float("nan"), 1.0)
    assert upd(edges=nan) == -1
    assert lib.liso_flow_metrics_reset(None, None) == -1
    assert lib.liso_flow_metrics_read(st, None, None) == -1


def _args(B=2, N=7):
    return dict(points=torch.zeros(B, N, 4), gt=torch.zeros(B, N, 3), pred=torch.zeros(B, N, 3),
                valid=torch.ones(B, N, dtype=torch.bool), moving=torch.zeros(B, N, dtype=torch.bool))


@pytest.mark.parametrize("bad", ["gt_dtype", "pred_shape", "pred_last", "mask_dtype", "mask_shape", "points_last", "bins"])
def test_python_argument_checks_raise_before_launching(bad):
    _lib()
    from liso_amd.eval.flow_metrics import FlowMetrics, FlowMetricsState

    a = _args()
    exc = ValueError
    if bad == "gt_dtype":
        a["gt"], exc = a["gt"].double(), TypeError
    elif bad == "pred_shape":
        a["pred"] = torch.zeros(2, 6, 3)
    elif bad == "pred_last":
        a["pred"] = torch.zeros(2, 7, 2)
    elif bad == "mask_dtype":
        a["valid"], exc = a["valid"].to(torch.uint8), TypeError
    elif bad == "mask_shape":
        a["valid"] = torch.ones(2, 8, dtype=torch.bool)
    elif bad == "points_last":
        a["points"] = torch.zeros(2, 7, 2)
    state = FlowMetricsState.__new__(FlowMetricsState)  # (no device buffer: the checks come first)
    state.device = torch.device("cuda:0")
    bins = np.arange(35, dtype=np.float64) if bad == "bins" else np.linspace(0, 100, 11)
    with pytest.raises(exc):
        state.update(a["points"], a["gt"], [a["pred"]], a["valid"], a["moving"], None, bins)
    if bad == "bins":
        with pytest.raises(ValueError):
            FlowMetrics(range_bins=np.arange(34))


def test_cpu_tensors_are_refused():
    L = _lib()
    from liso_amd.eval.flow_metrics import FlowMetrics

    a = _args()
    with pytest.raises(L.LisoHipError):
        FlowMetrics().update(a["points"], a["pred"], a["gt"], a["moving"], a["valid"])


def test_log_metrics_curves_refuses_plots():
    from liso_amd.eval.flow_metrics import FlowMetrics

    with pytest.raises(NotImplementedError):
        FlowMetrics().log_metrics_curves(0, summary_writer=object())
    with pytest.raises(NotImplementedError):
        FlowMetrics().log_metrics_curves(0, path="/nonexistent")
    # never updated: the reference's initial values
    fm = FlowMetrics(range_bins=(0.0, 25.0, 50.0))
    assert fm.log_metrics_curves(3, writer_prefix="raw/") == {"raw/AEE/still": 0.0, "raw/AEE/moving": 0.0, "raw/AEE/overall": 0.0}
    assert fm.num_points_in_range_bin["overall"].tolist() == [0, 0] and fm.total_num_pts == {"still": 0, "moving": 0, "overall": 0}


def test_aggregate_metrics_is_the_reference_weighting():
    from liso_amd.slim.utils.metrics import aggregate_metrics

    a = {"AEE": 0.5, "AVG_FLOW_VECTOR": np.array([1.0, 0.0, 2.0]), "num_pts_used": 10}
    b = {"AEE": 1.0, "AVG_FLOW_VECTOR": np.array([0.0, 3.0, 2.0]), "num_pts_used": 30}
    r = aggregate_metrics([a, b])
    assert r["num_pts_used"] == 40 and r["AEE"] == (0.5 * 10 + 1.0 * 30) / 40
    assert np.array_equal(r["AVG_FLOW_VECTOR"], np.array([10.0, 90.0, 80.0]) / 40)
