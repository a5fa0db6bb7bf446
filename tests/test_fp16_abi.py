"""CPU: the fp16 storage type of the detector path and its loss scale are declared in the C ABI, exported by the library and bound
in Python with the same codes; dtypes no kernel takes are refused before anything is launched.
Every test asserts on the host that fp16 is supported before it calls into the library, and no test here calls an entry point that can
launch a kernel (the element-code checks of the launching entry points are exercised with real device buffers in
tests/test_gpu_fp16_detector.py)."""
import os
import re

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _header_defines():
    out = {}
    for name in ("liso_conv.h", "liso_optim.h"):
        txt = open(os.path.join(ROOT, "include", name)).read()
        for k, v in re.findall(r"#define\s+(LISO_[A-Z0-9_]+)\s+(-?\d+)\b", txt):
            out[k] = int(v)
    return out


def _lib():
    from liso_amd import _lib

    # host-side check first: without fp16 support nothing below may reach the library
    assert hasattr(_lib, "CONV_F16") and hasattr(_lib, "ELEM_F16") and hasattr(_lib, "elem_code"), "fp16 storage is not built"
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib


def test_fp16_codes_agree_between_headers_and_python():
    L = _lib()
    d = _header_defines()
    assert d["LISO_CONV_F16"] == L.CONV_F16
    assert len({d["LISO_CONV_BF16"], d["LISO_CONV_F32X3"], d["LISO_CONV_F32"], d["LISO_CONV_F16"]}) == 4
    assert (d["LISO_ELEM_F32"], d["LISO_ELEM_BF16"], d["LISO_ELEM_F16"]) == (L.ELEM_F32, L.ELEM_BF16, L.ELEM_F16) == (0, 1, 2)
    assert L.elem_code(torch.float32) == 0 and L.elem_code(torch.bfloat16) == 1 and L.elem_code(torch.float16) == 2


def test_loss_scale_entry_points_are_declared_exported_and_bound():
    L = _lib()
    lib = L.lib()
    for s in ("liso_grad_nonfinite_f32", "liso_adamw_step_amp_f32", "liso_loss_scale_update"):
        assert s in L.SIGNATURES and hasattr(lib, s), s
    txt = open(os.path.join(ROOT, "include", "liso_optim.h")).read()
    body = re.search(r"typedef struct \{(.*?)\} liso_loss_scale_state;", txt, re.S).group(1)
    fields = re.findall(r"\b(?:float|int)\s+([a-z_]+)(\[\d+\])?;", body)
    assert [f for f, _ in fields] == ["scale", "found_inf", "growth_tracker", "step", "skipped", "reserved"]
    assert L.LOSS_SCALE_STATE_BYTES == 4 * (5 + 3)


@pytest.mark.parametrize("dtype", [torch.float64, torch.int32, torch.int64, torch.uint8, torch.bool])
def test_dtype_helper_rejects_types_no_kernel_takes(dtype):
    L = _lib()
    with pytest.raises(TypeError):
        L.elem_code(dtype)
    with pytest.raises(TypeError):
        L.is_half(dtype)


def test_packed_panel_sizes_know_the_fp16_mode():
    """(a pure size query, nothing is launched) one fp16 plane = the bytes of the bf16 plane; an unknown mode has no size"""
    L = _lib()
    lib = L.lib()
    assert lib.liso_conv_packed_bytes(64, 64, 9, L.CONV_F16) == lib.liso_conv_packed_bytes(64, 64, 9, L.CONV_BF16) > 0
    assert lib.liso_conv_packed_bytes(64, 64, 9, 7) == 0


def test_fp16_convolutions_plan_like_bf16():
    """LISO_CONV_F16 reuses the BF16 kernels and plans: the same kernel kind, tiles, slabs and statistics rows for every geometry"""
    import ctypes

    L = _lib()
    from liso_amd.utils import mfma_conv as MC

    lib = L.lib()
    for (B, ci, co, H, W, k, s, p, tr) in [(2, 64, 64, 64, 64, 3, 1, 1, False), (1, 64, 128, 40, 72, 3, 2, 1, False),
                                           (2, 256, 128, 16, 16, 2, 2, 0, True), (2, 128, 128, 32, 32, 1, 1, 0, False)]:
        spec = MC.ConvSpec(k, k, s, p, tr)
        ho, wo = spec.out_hw(H, W)
        infos = []
        for mode in (L.CONV_BF16, L.CONV_F16):
            d = (MC.scatter_desc if tr else MC.gather_desc)(spec, B, H, W, ci, ci, ho, wo, co, co, 0, mode)
            info = (ctypes.c_int * 8)()
            assert lib.liso_conv_plan_info(ctypes.byref(d), info) == 0
            infos.append((list(info), lib.liso_conv_stats_rows(ctypes.byref(d)), lib.liso_conv_wgrad_workspace_bytes(ctypes.byref(d))))
        assert infos[0] == infos[1], infos


def test_pillar_wrapper_refuses_an_unsupported_canvas_dtype_before_any_launch():
    """the canvas rows are allocated in out_dtype and the kernel writes one element code's layout: a dtype without a code must raise,
    not reach the kernel (CPU tensors here: the check comes first, so no device is needed)"""
    _lib()
    from liso_amd.networks.pcl_to_feature_grid.pcl_to_feature_grid import PointsPillarFeatureNetWrapper
    from liso_amd.utils.config import default_cfg

    m = PointsPillarFeatureNetWrapper(default_cfg(grid=64, bev_range_m=40.0))
    pts = [torch.zeros(100, 3)]
    for bad in (torch.float64, torch.int32):
        m.out_dtype = bad
        with pytest.raises(TypeError):
            m(pts)


def test_set_compute_dtype_and_trainer_loss_scale_arguments():
    _lib()
    from liso_amd.networks.simple_net.simple_net import BoxLearner
    from liso_amd.trainer import DetectorTrainer
    from liso_amd.utils.config import default_cfg

    cfg = default_cfg(grid=64, bev_range_m=40.0)
    net = BoxLearner(cfg)
    net.model.set_compute_dtype(torch.float16)
    assert net.model.pfn.out_dtype == torch.float16
    with pytest.raises(TypeError):
        net.model.set_compute_dtype(torch.float64)
    # bf16 / fp32 trainers take no loss scale; fp16 needs the device
    with pytest.raises(ValueError):
        DetectorTrainer(cfg, torch.device("cpu"), compute_dtype=torch.bfloat16, loss_scale="dynamic")
    with pytest.raises(ValueError):
        DetectorTrainer(cfg, torch.device("cpu"), compute_dtype=torch.float16)
    tr = DetectorTrainer(cfg, torch.device("cpu"), compute_dtype=torch.float32)
    assert tr.loss_scaler is None and tr.loss_scale_stats() is None


def test_loss_scale_state_round_trips_through_a_checkpoint():
    """scale, growth tracker, applied / skipped steps are saved and restored (a restored fp16 run does not restart at init_scale)"""
    _lib()
    from liso_amd.utils.loss_scale import DeviceLossScale

    a = DeviceLossScale(torch.device("cpu"))
    a.state[2], a.state[3], a.state[4] = 17, 123, 4  # growth tracker, applied, skipped
    a.set_scale(2.0 ** 13)
    sd = a.state_dict()
    b = DeviceLossScale(torch.device("cpu"))
    b.load_state_dict(sd)
    assert b.stats() == a.stats() == {"scale": 2.0 ** 13, "applied_steps": 123, "skipped_steps": 4, "growth_tracker": 17}
    assert int(b.state[1]) == 0  # (the found-inf flag is per step: never restored)
