"""ctypes loader for liso_amd/libliso_hip.so (C ABI: include/*.h).

The HIP library is the product.  There is no CPU fallback: if the shared object is
missing, or a device op is called without a GPU, we raise.  PyTorch is only used
for device memory and streams (``tensor.data_ptr()``, ``torch.cuda.current_stream()``).
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libliso_hip.so")

_lib = None


class LisoHipError(RuntimeError):
    pass


_ERRORS = {-1: "LISO_EINVAL (bad pointer/size)", -2: "LISO_EWORKSPACE (workspace too small)",
           -3: "LISO_ELAUNCH (HIP launch failed)", -4: "LISO_GROUND_ELENGTH (int(67 / delta_R) > 255)"}


def _preload_torch_hip_runtime():
    # torch bundles its own libamdhip64 (SONAME libamdhip64.so.7).  Our library needs the same SONAME; make
    # sure torch's copy is the one already mapped so that both share one HIP runtime (one context, one
    # allocator view of device pointers and streams).
    tl = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(tl):
        ctypes.CDLL(tl, mode=ctypes.RTLD_GLOBAL)


def lib():
    """Return the loaded library; raise loudly if it was never built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LisoHipError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C liso_amd/csrc`.  liso_amd has no CPU fallback for device ops.")
        _preload_torch_hip_runtime()
        _lib = ctypes.CDLL(LIB_PATH)
        _declare(_lib)
    return _lib


def check(code, what):
    if code != 0:
        raise LisoHipError(f"{what} failed: {_ERRORS.get(code, code)}")


def stream_ptr(device=None):
    """Current PyTorch HIP stream as a void* for the C ABI."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def multi_copy(pairs):
    """dst.copy_(src) for every (dst, src) of `pairs`, the device-resident, contiguous, same-dtype ones of one device as ONE launch
    (include/liso_optim.h: liso_multi_copy) on the current stream; everything else (host sources, dtype changes, strided views) by
    `copy_(non_blocking=True)`."""
    import torch

    fast = []
    for d, s_ in pairs:
        if (d.is_cuda and s_.is_cuda and d.device == s_.device and d.dtype == s_.dtype and d.shape == s_.shape and d.is_contiguous()
                and s_.is_contiguous() and (not fast or fast[0][0].device == d.device)):
            if d.numel() and d.data_ptr() != s_.data_ptr():
                fast.append((d, s_))
        else:
            d.copy_(s_, non_blocking=True)
    if len(fast) == 1:
        fast[0][0].copy_(fast[0][1], non_blocking=True)
    elif fast:
        n = len(fast)
        dst = (ctypes.c_void_p * n)(*[d.data_ptr() for d, _ in fast])
        src = (ctypes.c_void_p * n)(*[s_.data_ptr() for _, s_ in fast])
        nb = (ctypes.c_size_t * n)(*[d.numel() * d.element_size() for d, _ in fast])
        with torch.cuda.device(fast[0][0].device):
            check(lib().liso_multi_copy(n, dst, src, nb, stream_ptr()), "multi_copy")


def copy_blocks(jobs):
    """`jobs`: (dst, src) pairs of fp32 tensors that are 2-D "rows" views -- dst[i] <- src[i] where both index the same logical block
    [rows, cols...] with the trailing dimensions contiguous and one stride between rows (a filter block inside a merged filter, a
    column range of a matrix, a whole contiguous tensor) -- as ONE launch (include/liso_optim.h: liso_multi_copy_rows)."""
    import torch

    n = len(jobs)
    if n == 0:
        return
    dst = (ctypes.c_void_p * n)()
    src = (ctypes.c_void_p * n)()
    rows = (ctypes.c_uint * n)()
    rb = (ctypes.c_uint * n)()
    ds = (ctypes.c_size_t * n)()
    ss = (ctypes.c_size_t * n)()

    def rows_view(t):
        # -> (rows, elements per row, row stride in elements): dim 0 = rows, the rest one contiguous run
        assert t.dtype == torch.float32 and t.is_cuda
        if t.dim() == 1:
            assert t.stride(0) == 1 or t.numel() <= 1
            return 1, t.numel(), t.numel()
        inner = 1
        for k in range(t.dim() - 1, 0, -1):
            assert t.shape[k] == 1 or t.stride(k) == inner, (tuple(t.shape), t.stride())
            inner *= t.shape[k]
        return t.shape[0], inner, (t.stride(0) if t.shape[0] > 1 else inner)

    for i, (d, s_) in enumerate(jobs):
        assert tuple(d.shape) == tuple(s_.shape), (tuple(d.shape), tuple(s_.shape))
        r, c, dstr = rows_view(d)
        r2, c2, sstr = rows_view(s_)
        assert (r, c) == (r2, c2)
        dst[i], src[i], rows[i], rb[i], ds[i], ss[i] = d.data_ptr(), s_.data_ptr(), r, 4 * c, 4 * dstr, 4 * sstr
    with torch.cuda.device(jobs[0][0].device):
        check(lib().liso_multi_copy_rows(n, dst, src, rows, rb, ds, ss, stream_ptr()), "multi_copy_rows")


def require_cuda(*tensors):
    for t in tensors:
        if not t.is_cuda:
            raise LisoHipError("device op called with a CPU tensor; liso_amd has no CPU fallback")


_vp, _i, _f, _sz, _lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_long
_d = ctypes.c_double

# symbol -> (restype, argtypes); mirrors include/*.h exactly (tests/test_abi.py parses the headers and checks)
SIGNATURES = {
    # include/liso_iou3d.h
    "liso_iou3d_overlap_bev_f32": (_i, [_vp, _i, _vp, _i, _vp, _vp]),
    "liso_iou3d_iou_bev_f32": (_i, [_vp, _i, _vp, _i, _vp, _vp]),
    "liso_iou3d_nms_workspace_bytes": (_sz, [_i]),
    "liso_iou3d_nms_f32": (_i, [_vp, _i, _f, _vp, _vp, _vp, _sz, _vp]),
    "liso_iou3d_nms_normal_f32": (_i, [_vp, _i, _f, _vp, _vp, _vp, _sz, _vp]),
    "liso_iou3d_iou_bev_cpu_f32": (_i, [_vp, _i, _vp, _i, _vp]),
    # include/liso_pillars.h
    "liso_pillars_voxelize_workspace_bytes": (_sz, [_vp, _i, _i]),
    "liso_pillars_voxelize_f32": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "liso_pfn_partials_bytes": (_sz, []),
    "liso_pfn_decorate_workspace_bytes": (_sz, [_i, _i]),
    "liso_pfn_decorate_f32": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "liso_pfn_bn_prepare_f32": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _i, _vp, _vp, _vp, _vp]),
    "liso_pfn_forward_scatter": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "liso_pfn_forward_rows": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "liso_pfn_backward": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "liso_pfn_bn_prepare_sub_f32": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _i, _vp, _vp, _vp, _vp]),
    "liso_pfn_forward_scatter_sub": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "liso_pfn_forward_rows_sub": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "liso_pfn_backward_sub": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    # include/liso_kabsch.h
    "liso_kabsch_workspace_bytes": (_sz, [_vp]),
    "liso_kabsch_trafos_counted_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "liso_symm_ortho_fwd_f64": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "liso_symm_ortho_bwd_f64": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "liso_weighted_moments_workspace_bytes": (_sz, [_i]),
    "liso_weighted_moments_fwd_f32": (_i, [_vp, _vp, _vp, _i, ctypes.c_long, _vp, _vp, _sz, _vp]),
    "liso_weighted_moments_bwd_f32": (_i, [_vp, _vp, _vp, _i, ctypes.c_long, _vp, _vp, _vp, _vp, _vp]),
    # include/liso_flow_cluster.h
    "liso_bev_dynamic_flow_workspace_bytes": (_sz, [_i, _i, _i]),
    "liso_bev_dynamic_flow_f32": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "liso_odom_inverse_minus_eye_f64": (_i, [_vp, _i, _vp, _vp]),
    "liso_fit_box_z_workspace_bytes": (_sz, [_i, _i]),
    "liso_fit_box_z_f32": (_i, [_vp, _i, _i, _vp, _i, _vp, _i, _vp, _i, _f, _vp, _vp, _vp, _vp, _sz, _vp]),
    "liso_dbscan_workspace_bytes": (_sz, [_vp]),
    "liso_dbscan_components": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "liso_dbscan_labels": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "liso_region_props_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "liso_region_props": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    # include/liso_slim.h
    "liso_corr_lookup_fwd_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "liso_corr_lookup_fwd_tiled_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "liso_corr_lookup_bwd_dvol_f32": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "liso_corr_pyramid_fwd_f32": (_i, [_vp, _vp, _vp, _vp]),
    "liso_corr_pyramid_bwd_f32": (_i, [_vp, _vp, _vp, _vp]),
    "liso_corr_bwd_features_workspace_bytes": (_sz, [_vp]),
    "liso_corr_bwd_features_f32": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "liso_rows_combine_f32": (_i, [_lg, _i, _vp, _lg, _vp, _lg, _vp, _lg, _vp, _lg, _vp, _lg, _i, _vp]),
    "liso_gru_out_rows_train_f32": (_i, [_lg, _i, _vp, _lg, _vp, _vp, _lg, _vp, _lg, _vp]),
    "liso_gru_out_rows_bwd_f32": (_i, [_lg, _i, _vp, _lg, _vp, _vp, _lg, _vp, _lg, _vp, _lg, _vp, _vp, _vp]),
    "liso_gru_in_rows_bwd_f32": (_i, [_lg, _i, _vp, _lg, _vp, _lg, _vp, _vp, _vp, _lg, _vp, _lg, _vp, _vp]),
    "liso_raft_state_step_train_f32": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "liso_raft_pack_output_grads_f32": (_i, [_lg, _i, _vp, _vp, _vp, _vp]),
    "liso_nearest_point_loss_fwd_f32": (_i, [_vp] * 8),
    "liso_nearest_point_loss_bwd_f32": (_i, [_vp] * 9),
    # include/liso_slim_decode.h
    "liso_slim_decode_weights_fwd": (_i, [_vp] * 6 + [_i] + [_vp] * 4),
    "liso_slim_decode_weights_bwd": (_i, [_vp] * 9),
    "liso_slim_decode_points_fwd": (_i, [_vp] * 9),
    "liso_slim_decode_points_bwd": (_i, [_vp] * 11),
    "liso_slim_loss_workspace_bytes": (_sz, []),
    "liso_slim_static_points_loss_fwd": (_i, [_i, ctypes.c_long, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "liso_slim_static_points_loss_bwd": (_i, [_i, ctypes.c_long, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "liso_slim_knn_queries": (_i, [_i, _i, ctypes.c_long, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "liso_slim_nearest_point_loss_fwd": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "liso_slim_nearest_point_loss_bwd": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "liso_bev_gather_fwd_f32": (_i, [_vp, _vp, ctypes.c_long, _i, ctypes.c_float, _vp, _vp]),
    "liso_bev_gather_bwd_f32": (_i, [_vp, _vp, _vp, _vp, ctypes.c_long, _i, _vp, _vp, _vp]),
    "liso_gru_in_fwd_f32": (_i, [_vp, _vp, _vp, ctypes.c_long, _vp, _vp, _vp, _vp, _vp]),
    "liso_gru_in_bwd_f32": (_i, [_vp, _vp, ctypes.c_long, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_long, _vp, _vp]),
    "liso_gru_out_fwd_f32": (_i, [ctypes.c_long, _vp, _vp, _vp, _vp, _vp]),
    "liso_gru_out_bwd_f32": (_i, [ctypes.c_long, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "liso_gru_in_rows_f32": (_i, [ctypes.c_long, _i, _vp, ctypes.c_long, _vp, ctypes.c_long, _vp, _vp, ctypes.c_long, _vp]),
    "liso_gru_out_rows_f32": (_i, [ctypes.c_long, _i, _vp, ctypes.c_long, _vp, _vp, ctypes.c_long, _vp]),
    "liso_multi_copy": (_i, [_i, _vp, _vp, _vp, _vp]),
    "liso_bev_lin_index": (_i, [_vp, _i, _vp, _i, ctypes.c_long, _i, _i, _vp, _vp]),
    "liso_channel_extrema_workspace_bytes": (_sz, []),
    "liso_channel_extrema_f32": (_i, [_vp, ctypes.c_long, _i, _i, _vp, _vp, _sz, _vp]),
    "liso_bev_plan_tile_lin": (_i, [_vp, _i, ctypes.c_long, _i, _i, _i, _i, _vp, _vp]),
    "liso_bev_plan_rank": (_i, [_vp, _vp, ctypes.c_long, _vp, _vp, _vp]),
    "liso_bev_plan_expand": (_i, [_vp, _vp, _vp, _i, ctypes.c_long, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "liso_raft_state_step_f32": (_i, [_i, _i, _vp, ctypes.c_long, _vp, _vp, _vp, _vp]),
    "liso_raft_upsample_scratch_bytes": (_sz, [_vp]),
    "liso_raft_upsample_outputs_fwd_f32": (_i, [_vp] * 5),
    "liso_raft_upsample_outputs_bwd_f32": (_i, [_vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    # include/liso_detector.h
    "liso_centerloss_workspace_bytes": (_sz, [_vp]),
    "liso_centerloss_fwd_f32": (_i, [_vp] * 17 + [_sz, _vp]),
    "liso_centerloss_bwd_f32": (_i, [_vp] * 21),
    "liso_render_center_targets_f32": (_i, [_vp] * 12),
    "liso_conv_pack_weights_batched": (_i, [_vp, _i, _vp]),
    "liso_conv_pack_weights_placed": (_i, [_vp, _i, _i, _vp]),
    "liso_conv_in_finalize": (_i, [_vp, _i, _i, _i, _i, ctypes.c_long, _vp, _vp, _f, _vp, _vp]),
    "liso_residual_affine_relu_f32": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _i, ctypes.c_long, _i, _vp]),
    # include/liso_box_mining.h
    "liso_scan_workspace_bytes": (_sz, [_i, ctypes.c_long]),
    "liso_scan_inclusive_i32": (_i, [_vp, _i, ctypes.c_long, _vp, _vp, _sz, _vp]),
    "liso_mine_boxes_from_regions": (_i, [_vp, _i, _i, _vp, _i, _vp, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "liso_mine_filter_compact": (_i, [_vp] * 21),
    "liso_mine_box_motion": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp]),
    "liso_mine_nms_workspace_bytes": (_sz, [_i, _i]),
    "liso_mine_nms_prepare": (_i, [_i, _i, _i] + [_vp] * 11 + [_sz, _vp]),
    "liso_mine_nms_finish": (_i, [_i, _i, _i] + [_vp] * 16),
    # include/liso_optim.h
    "liso_adamw_step_f32": (_i, [_vp, _vp, _vp, _vp, _sz] + [ctypes.c_double] * 5 + [ctypes.c_long, _vp]),
    "liso_adamw_step_scaled_f32": (_i, [_vp, _vp, _vp, _vp, _sz] + [ctypes.c_double] * 6 + [ctypes.c_long, _vp]),
    "liso_adamw_pack_table_plan": (_i, [_vp, _i, _sz, _vp, _vp]),
    "liso_adamw_pack_table_fill": (_i, [_vp, _i, _sz, _vp, _sz]),
    "liso_adamw_step_packed_f32": (_i, [_vp, _vp, _vp, _vp, _sz] + [ctypes.c_double] * 6 + [ctypes.c_long, _vp, _i, _vp]),
    "liso_grad_nonfinite_f32": (_i, [_vp, _sz, _vp, _vp]),
    "liso_adamw_step_amp_f32": (_i, [_vp, _vp, _vp, _vp, _sz] + [ctypes.c_double] * 6 + [_vp, _vp]),
    "liso_loss_scale_update": (_i, [_vp, ctypes.c_double, ctypes.c_double, _i, _vp]),
    "liso_rmsprop_step_f32": (_i, [_vp, _vp, _vp, _sz] + [ctypes.c_double] * 4 + [_vp]),
    "liso_multi_copy_rows": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "liso_gather_f32": (_i, [_i, _vp, _vp, _vp, _vp]),
    # include/liso_bn.h
    "liso_bn_workspace_bytes": (_sz, [_i]),
    "liso_bn_relu_fwd": (_i, [_vp, _i, ctypes.c_long, _i, _vp, _vp, _vp, _vp, _f, _f, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "liso_in_workspace_bytes": (_sz, [_i, _i]),
    "liso_in_relu_fwd": (_i, [_vp, _i, _i, ctypes.c_long, _i, _vp, _vp, _f, _i, _vp, _vp, _vp, _sz, _vp]),
    "liso_in_relu_bwd": (_i, [_vp, _vp, _i, _i, ctypes.c_long, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "liso_in_relu_bwd_sum": (_i, [_vp, _vp, _i, _i, ctypes.c_long, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "liso_bn_relu_bwd": (_i, [_vp, _vp, _i, ctypes.c_long, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "liso_bn_relu_bwd_strided": (_i, [_vp, ctypes.c_long, _vp, ctypes.c_long, _i, ctypes.c_long, _i, _vp, _vp, _i, _i, _vp, ctypes.c_long, _vp, _vp, _vp, _sz, _vp]),
    "liso_bn_relu_bwd_chained": (_i, [_vp, ctypes.c_long, _vp, ctypes.c_long, _i, ctypes.c_long, _i, _vp, _vp, _i, _i, _vp, ctypes.c_long, _vp, _vp, _vp, _sz, _vp, _vp]),
    "liso_bn_multi_workspace_bytes": (_sz, [_vp, _i, _i]),
    "liso_bn_relu_bwd_multi": (_i, [_vp, ctypes.c_long, _vp, ctypes.c_long, _vp, ctypes.c_long, _i, ctypes.c_long, _vp, _i, _i, _i, _vp, ctypes.c_long,
                                    _vp, _sz, _vp, _vp, _vp]),
    "liso_bn_relu_bwd_multi_check": (_i, [_vp, _i, _i, _i, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, _vp]),
    "liso_knn_workspace_bytes": (_sz, [_vp, _i]),
    "liso_knn_build_f32": (_i, [_vp, _vp, _i, _i, _vp, _sz, _vp]),
    "liso_knn_sorted_ids": (_i, [_vp, _vp, _i, _vp, _vp]),
    "liso_knn_query_f32": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _i, _vp]),
    # include/liso_conv.h
    "liso_conv_packed_bytes": (_sz, [_i, _i, _i, _i]),
    "liso_conv_pack_weights": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "liso_conv_stats_rows": (_i, [_vp]),
    "liso_conv_kernel_kind": (_i, [_vp]),
    "liso_conv_forward": (_i, [_vp] * 10),
    "liso_conv_set_option": (_i, [_i, _i]),
    "liso_conv_forward_sparse": (_i, [_vp] * 11),
    "liso_conv_plan_info": (_i, [_vp, _vp]),
    "liso_conv_wgrad_workspace_bytes": (_sz, [_vp]),
    "liso_conv_wgrad": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "liso_conv_wgrad_deferred": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _sz, _vp, _vp]),
    "liso_conv_wgrad_reduce": (_i, [_vp, _vp]),
    "liso_conv_wgrad_sparse_workspace_bytes": (_sz, [_vp]),
    "liso_conv_wgrad_sparse_f32": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _sz, _vp]),
    "liso_conv_wgrad_smallci_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "liso_conv_wgrad_smallci_f32": (_i, [_vp, ctypes.c_long, _vp, ctypes.c_long, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "liso_sparse_conv_stat_groups": (_i, [_i, _i, _i]),
    "liso_sparse_conv_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "liso_sparse_conv_forward": (_i, [_vp, ctypes.c_long, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "liso_sparse_conv_forward_rows": (_i, [_vp, ctypes.c_long, _i, _vp, ctypes.c_long, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp,
                                           _sz, _vp]),
    "liso_sparse_conv_dgrad": (_i, [_vp, ctypes.c_long, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, ctypes.c_long, _vp, _vp, _sz, _i, _vp]),
    "liso_conv_bn_finalize": (_i, [_vp, _i, _i, _i, ctypes.c_long, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp]),
    "liso_conv_bn_finalize_merged": (_i, [_vp, _i, _i, _i, ctypes.c_long, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _i, _i, _vp]),
    # include/liso_tracking.h
    "liso_points_in_boxes_workspace_bytes": (_sz, [_vp]),
    "liso_points_in_boxes_f32": (_i, [_vp] * 9 + [_sz, _vp]),
    "liso_match_greedy_f32": (_i, [_vp, ctypes.c_long, ctypes.c_long, _i, _i, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "liso_fit_boxes_closeness_workspace_bytes": (_sz, [ctypes.c_long, _i]),
    "liso_fit_boxes_closeness_f32": (_i, [_vp, ctypes.c_long, _i, _vp, _vp, _i, _f, _vp, _vp, _vp, _sz, _vp]),
    "liso_bike_rollout_fwd_f32": (_i, [_i, _i, _vp, _vp, _vp, _vp, _f, _f, _f, _vp, _vp]),
    "liso_bike_rollout_bwd_f32": (_i, [_i, _i, _vp, _vp, _vp, _f, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "liso_smooth_tracks_jerk_f32": (_i, [_vp, _vp, _i, _i, _i, _f, _f, _vp, _vp]),
    # include/liso_flow_metrics.h
    "liso_flow_metrics_state_bytes": (_sz, []),
    "liso_flow_metrics_result_bytes": (_sz, []),
    "liso_flow_metrics_reset": (_i, [_vp, _vp]),
    "liso_flow_metrics_update": (_i, [_vp, _lg, _vp, _lg, _vp, _lg, _i, _vp, _lg, _vp, _lg, _vp, _lg, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "liso_flow_metrics_read": (_i, [_vp, _vp, _vp]),
    # include/liso_det_nms.h
    "liso_det_nms_workspace_bytes": (_sz, [_i, _i]),
    "liso_det_nms_order": (_i, [_i, _i, _vp, _vp, _vp, _f, _vp, _vp, _vp, _sz, _vp]),
    "liso_det_nms_select": (_i, [_i, _i, _vp, _vp, _vp, _f, _i, _i, _vp, _vp, _vp]),
    "liso_det_nms_gather": (_i, [_i, _i, _i, _vp, _vp, _vp, _i, _vp]),
    # include/liso_det_val.h
    "liso_det_val_pairs_f32": (_i, [_i, _i, _i] + [_vp] * 8),
    "liso_det_val_pairs_cpu_f32": (_i, [_i, _i, _i] + [_vp] * 7),
    "liso_det_val_transfer_classes": (_i, [_i, _i, _i] + [_vp] * 5 + [_f, _vp, _vp, _vp]),
    "liso_det_val_match_f32": (_i, [_i, _i, _i] + [_vp] * 10 + [_i, _vp, _i, _vp, _i] + [_vp] * 6),
    "liso_det_val_assign_f32": (_i, [_i, _i, _i] + [_vp] * 8 + [_i, _vp, _i, _vp, _i] + [_vp] * 5),
    "liso_match_assign_f32": (_i, [_vp, ctypes.c_long, _i, _i, _f, _vp, _vp, _vp]),
    # include/liso_nusc_metrics.h
    "liso_det_val_nusc_f32": (_i, [_i, _i, _i] + [_vp] * 8 + [_i, _i, _vp, _i] + [_vp] * 6),
    # include/liso_ground.h
    "liso_ground_jcp_workspace_bytes": (_sz, [_vp]),
    "liso_ground_jcp_workspace_layout": (_i, [_vp, _vp]),
    "liso_ground_jcp_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "liso_ground_jcp_stages_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _vp]),
    "liso_ground_cone_f32": (_i, [_i, _i, _i, _vp, _vp, ctypes.c_double, ctypes.c_double, _vp, _vp, _vp]),
    "liso_ground_compact_workspace_bytes": (_sz, [_i, _i]),
    "liso_ground_compact_f32": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    # include/liso_augment.h
    "liso_bev_free_mask_workspace_bytes": (_sz, [_i, _i]),
    "liso_bev_free_mask": (_i, [_vp, ctypes.c_long, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "liso_bev_select_free_cells": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp]),
    "liso_snippet_paste": (_i, [_vp, ctypes.c_long, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, _i, _vp, _vp, _vp, _vp]),
    "liso_bev_free_mask_batch_workspace_bytes": (_sz, [_i, _i, _i]),
    "liso_bev_free_mask_batch": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "liso_snippet_augment_batch_workspace_bytes": (_sz, [_vp]),
    "liso_snippet_augment_batch": (_i, [_vp] * 23 + [_sz, _vp]),
    "liso_cloud_append_batch": (_i, [_vp] * 4 + [_i] * 4 + [_vp] * 3),
    # include/liso_sample_prep.h
    "liso_sample_transform_f32": (_i, [_i, _i, _i] + [_vp] * 7),
    "liso_sample_transform_poses_f64": (_i, [_i, _vp, _vp, _i, _vp, _i, _vp]),
    "liso_bev_crop_workspace_bytes": (_sz, [_i, _i]),
    "liso_bev_crop_f32": (_i, [_vp] * 14 + [_sz, _vp]),
    "liso_bev_point_maps_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "liso_bev_point_maps_f32": (_i, [_i] * 5 + [_vp] * 6 + [ctypes.c_double] + [_vp] * 5 + [_sz, _vp]),
    # include/liso_label_prep.h
    "liso_box_has_points_f32": (_i, [_i] * 4 + [_vp] * 7),
    "liso_filter_boxes": (_i, [_vp] * 6 + [_i] + [_vp] * 3),
    "liso_object_velocity_f64": (_i, [_i, _i] + [_vp] * 5),
    "liso_ignore_region_mask": (_i, [_i] * 4 + [ctypes.c_double] * 2 + [_vp] * 6),
    "liso_render_center_targets_ex_f32": (_i, [_vp] * 15),
    # include/liso_snippets.h
    "liso_snippet_cut_workspace_bytes": (_sz, [_i, _i, _i]),
    "liso_snippet_cut_f32": (_i, [_i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _lg] + [_vp] * 5 + [_sz, _vp]),
    # include/liso_tracking.h: the sequence tracker
    "liso_track_sequences_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "liso_track_sequences": (_i, [_i] * 4 + [_vp] * 7 + [ctypes.c_double] + [_vp] * 10 + [_sz, _vp]),
    # include/liso_track_mining.h
    "liso_track_mining_workspace_bytes": (_sz, [_i] * 5),
    "liso_select_tracks": (_i, [_i] * 5 + [_vp] * 7 + [_i, _f, _d, _d, _i, _d, _d, _i, _d] + [_vp] * 13 + [_vp, _sz, _vp]),
    "liso_refine_tracks_apply": (_i, [_i] * 3 + [_vp] * 12 + [_i, _i, _d] + [_vp] * 7 + [_vp]),
    "liso_export_tracks": (_i, [_i] * 6 + [_vp] * 11 + [_i] + [_vp] * 13 + [_vp, _sz, _vp]),
    # include/liso_frame_prep.h
    "liso_frame_prep_workspace_bytes": (_sz, [_vp]),
    "liso_prepare_tracker_frames": (_i, [_vp] * 27 + [_sz, _vp]),
    # include/liso_odometry.h
    "liso_odometry_workspace_bytes": (_sz, [_vp]),
    "liso_odometry_workspace_layout": (_i, [_vp, _vp]),
    "liso_odometry_preprocess": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "liso_odometry_register": (_i, [_vp, _i] + [_vp] * 8 + [_sz, _vp]),
    "liso_odometry_map_update": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "liso_odometry_sequences": (_i, [_vp] * 11 + [_sz, _vp]),
    "liso_odometry_relative_f64": (_i, [_i, _vp, _vp, _vp, _vp]),
    "liso_correct_kitti_scan_f64": (_i, [_lg, _vp, _vp, _vp]),
    # include/liso_flow_labels.h
    "liso_flow_labels_workspace_bytes": (_sz, [_i, _i]),
    "liso_flow_labels_f32": (_i, [_vp] * 18 + [_sz, _vp]),
    "liso_kitti_rows_cols_f32": (_i, [_i, _i, _i, _vp, _vp, _d, _i, _i, _vp, _vp, _vp]),
    # include/liso_visu.h
    "liso_visu_flow_wheel_f32": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
    "liso_visu_topdown_workspace_bytes": (_sz, [_i, _i, _i]),
    "liso_visu_topdown_f32": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "liso_visu_occupancy_f64": (_i, [_i, _i, _i, _i, _i, _d, _d, _vp, _vp, _vp, _vp]),
    "liso_visu_box_corners_bev": (_i, [_i, _i, _i, _i, _i, _vp, _i, _d, _d, _vp, _vp, _vp, _vp, _vp]),
    "liso_visu_box_colors": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "liso_visu_lines_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "liso_visu_draw_lines_f32": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
}


CONV_MAX_TAPS, CONV_MAX_CLASSES, CONV_BF16, CONV_F32X3, CONV_F32, CONV_F16 = 49, 4, 0, 1, 2, 3
# element codes of the `is_bf16` / `out_bf16` / `grad_bf16` arguments (include/liso_conv.h: LISO_ELEM_*)
ELEM_F32, ELEM_BF16, ELEM_F16 = 0, 1, 2
_ELEM_CODES = {torch.float32: ELEM_F32, torch.bfloat16: ELEM_BF16, torch.float16: ELEM_F16}
LOSS_SCALE_STATE_BYTES = 32  # sizeof(liso_loss_scale_state), include/liso_optim.h


def elem_code(dtype):
    """the element code of a detector-path tensor dtype: fp32 -> 0, bf16 -> 1, fp16 -> 2; anything else raises TypeError"""
    code = _ELEM_CODES.get(dtype)
    if code is None:
        raise TypeError(f"no device kernel takes {dtype} tensors (float32, bfloat16 or float16)")
    return code


def is_half(dtype):
    """a 16-bit storage type of the detector path (bf16 or fp16): 8 channels per lane, one MFMA per product"""
    return elem_code(dtype) != ELEM_F32


def lane_channels(dtype):
    """channels in a lane's 16-byte access of the channels-last passes: 8 in bf16 / fp16, 4 in fp32"""
    return 8 if is_half(dtype) else 4
CONV_OPT_SHARED_GPU = 1
CONV_OPT_ROLES_CUS = 2


class ConvDesc(ctypes.Structure):
    """mirror of liso_conv_desc (include/liso_conv.h)"""
    _fields_ = [("batch", _i), ("hi", _i), ("wi", _i), ("ci", _i), ("x_pix_stride", _i), ("ho", _i), ("wo", _i), ("co", _i),
                ("y_pix_stride", _i), ("y_ch_off", _i), ("hv", _i), ("wv", _i), ("isy", _i), ("isx", _i), ("osy", _i), ("osx", _i),
                ("n_classes", _i), ("class_tap_begin", _i * (CONV_MAX_CLASSES + 1)), ("class_ooy", _i * CONV_MAX_CLASSES),
                ("class_oox", _i * CONV_MAX_CLASSES), ("n_taps", _i), ("tap_dy", _i * CONV_MAX_TAPS), ("tap_dx", _i * CONV_MAX_TAPS),
                ("tap_w", _i * CONV_MAX_TAPS), ("w_taps", _i), ("mode", _i), ("out_f32", _i), ("in_relu", _i), ("out_relu", _i),
                ("in_affine_batch_stride", _i), ("wgrad_co", _i)]


class ConvPackPlacedJob(ctypes.Structure):
    """mirror of liso_conv_pack_placed_job (include/liso_conv.h)"""
    _fields_ = [("src", _vp), ("dst", _vp), ("d0", _i), ("d1", _i), ("kh", _i), ("kw", _i), ("transposed", _i), ("for_dgrad", _i),
                ("mode", _i), ("K", _i), ("N", _i), ("k_offset", _i), ("n_offset", _i)]


class AdamwPackDest(ctypes.Structure):
    """mirror of liso_adamw_pack_dest (include/liso_optim.h)"""
    _fields_ = [("dst", _vp), ("for_dgrad", _i), ("mode", _i), ("K", _i), ("N", _i), ("k_offset", _i), ("n_offset", _i)]


class AdamwPackItem(ctypes.Structure):
    """mirror of liso_adamw_pack_item (include/liso_optim.h)"""
    _fields_ = [("offset", _sz), ("d0", _i), ("d1", _i), ("kh", _i), ("kw", _i), ("transposed", _i), ("n_dest", _i),
                ("dest", AdamwPackDest * 2), ("mirror", _vp), ("mirror_row_stride", _sz)]


class ConvPackJob(ctypes.Structure):
    """mirror of liso_conv_pack_job (include/liso_conv.h)"""
    _fields_ = [("src", _vp), ("dst", _vp), ("d0", _i), ("d1", _i), ("kh", _i), ("kw", _i), ("transposed", _i), ("for_dgrad", _i),
                ("mode", _i)]


class WgradReduceJob(ctypes.Structure):
    """mirror of liso_wgrad_reduce_job (include/liso_conv.h)"""
    _fields_ = [("slab", _vp), ("bias_slab", _vp), ("dw", _vp), ("dbias", _vp), ("cip", ctypes.c_long), ("cop", ctypes.c_long),
                ("splits", _i), ("bias_rows", _i), ("taps", _i), ("ci", _i), ("co", _i), ("transposed", _i)]


BN_MAX_GROUPS = 4  # include/liso_bn.h: LISO_BN_MAX_GROUPS


class BnGroup(ctypes.Structure):
    """mirror of liso_bn_group (include/liso_bn.h)"""
    _fields_ = [("c_off", _i), ("c", _i), ("gamma", _vp), ("stats", _vp), ("grad_gamma", _vp), ("grad_beta", _vp)]


class KnnGrid(ctypes.Structure):
    """mirror of liso_knn_grid (include/liso_slim.h)"""
    _fields_ = [("x_min", _f), ("y_min", _f), ("cell", _f), ("nx", _i), ("ny", _i), ("z_min", _f), ("z_cell", _f), ("nz", _i)]


class CenterLossCfg(ctypes.Structure):
    """mirror of liso_centerloss_cfg (include/liso_detector.h)"""
    _fields_ = [("batch", _i), ("h", _i), ("w", _i), ("res_x", _f), ("res_y", _f), ("z_min", _f), ("z_max", _f),
                ("sup_weight", _f), ("rot_reg_weight", _f)]


class NpLossCfg(ctypes.Structure):
    """mirror of liso_nploss_cfg (include/liso_slim.h)"""
    _fields_ = [("batch", _i), ("n", ctypes.c_long), ("n_b", ctypes.c_long), ("ext", _f * 4), ("fov_mode", _i), ("delta", _f)]


class SlimDecodeCfg(ctypes.Structure):
    """mirror of liso_slim_decode_cfg (include/liso_slim_decode.h)"""
    _fields_ = [("samples", _i), ("n", ctypes.c_long), ("h", _i), ("w", _i), ("logit_mode", _i * 4), ("static_flow_zero", _i),
                ("dynamic_flow_zero", _i), ("overwrite_flow", _i), ("overwrite_logits", _i), ("non_rigid", _i), ("use_static_aggr", _i),
                ("dyn_grad_scale", _f), ("ext_lo", ctypes.c_double * 2), ("ext_span", ctypes.c_double * 2)]


class SlimDecodeOut(ctypes.Structure):
    """mirror of liso_slim_decode_out: 11 float pointers + the flags pointer (None = not wanted)"""
    FIELDS = ("dis_logit", "dis", "logits", "probs", "staticness", "dynamicness", "groundness", "dyn_flow", "stat_flow", "agg_flow", "saf_flow")
    _fields_ = [(k, _vp) for k in FIELDS] + [("flags", _vp)]


class SlimNpLossCfg(ctypes.Structure):
    """mirror of liso_slim_nploss_cfg"""
    _fields_ = [("samples", _i), ("clouds", _i), ("n", ctypes.c_long), ("n_b", ctypes.c_long), ("ext", _f * 4), ("fov_mode", _i), ("delta", _f)]


class BoxPtsCfg(ctypes.Structure):
    """mirror of liso_boxpts_cfg (include/liso_tracking.h)"""
    _fields_ = [("batch", _i), ("n", ctypes.c_long), ("k", _i), ("point_stride", _i), ("precision", _i), ("dims_bloat", _f)]


class AugmentBatchCfg(ctypes.Structure):
    """mirror of liso_augment_batch_cfg (include/liso_augment.h)"""
    _fields_ = [("batch", _i), ("n_max", _i), ("h", _i), ("w", _i), ("radius", _i), ("max_num_objs", _i), ("num_snippets", _i),
                ("db_rows", ctypes.c_long), ("extra_capacity", _i), ("selection", _i), ("range_x", _d), ("range_y", _d), ("cell_x", _d),
                ("cell_y", _d), ("max_scale_delta", _d), ("max_points_dropout", _d), ("vmin", _d), ("vmax", _d)]


class FramePrepCfg(ctypes.Structure):
    """mirror of liso_frame_prep_cfg (include/liso_frame_prep.h)"""
    _fields_ = [("n_seq", _i), ("max_frames", _i), ("max_box", _i), ("cap", _i), ("n_points", ctypes.c_long), ("point_stride", _i),
                ("n_fov_points", ctypes.c_long), ("fov_stride", _i), ("bev_range_x", _f), ("bev_range_y", _f), ("drop_on_bev_boundaries", _i),
                ("min_points_in_box", _i), ("fov_min_points", _i), ("align", _i), ("no_align_below_m", _d), ("full_align_above_m", _d)]


class OdometryCfg(ctypes.Structure):
    """mirror of liso_odometry_cfg (include/liso_odometry.h)"""
    _fields_ = [("n_seq", _i), ("max_frames", _i), ("n_max", _i), ("point_stride", _i), ("map_voxels", _i), ("max_points_per_voxel", _i),
                ("max_num_iterations", _i), ("max_range", _d), ("min_range", _d), ("voxel_size", _d), ("initial_threshold", _d),
                ("min_motion_th", _d), ("convergence_criterion", _d)]


class GruCfg(ctypes.Structure):
    """mirror of liso_gru_cfg (include/liso_slim.h)"""
    _fields_ = [("batch", _i), ("ch", _i), ("cx", _i), ("hw", ctypes.c_long)]


class UpsampleCfg(ctypes.Structure):
    """mirror of liso_upsample_cfg (include/liso_slim.h)"""
    _fields_ = [("n_it", _i), ("batch2", _i), ("dirs", _i), ("h", _i), ("w", _i), ("factor", _i), ("flow_scale", _f)]


class MineFilterCfg(ctypes.Structure):
    """mirror of liso_mine_filter_cfg (include/liso_box_mining.h)"""
    _fields_ = [("batch", _i), ("k", _i), ("min_points", _i), ("aspect_ratio_max", ctypes.c_double), ("max_box_len_m", ctypes.c_double),
                ("min_box_area_m2", ctypes.c_double), ("min_box_volume_m3", ctypes.c_double), ("park_invalid", _i)]


class DetGatherField(ctypes.Structure):
    """mirror of liso_det_gather_field (include/liso_det_nms.h)"""
    _fields_ = [("src", _vp), ("dst", _vp), ("row_elems", _i), ("elem_bytes", _i), ("pad_bits", ctypes.c_uint64)]


class GroundCfg(ctypes.Structure):
    """mirror of liso_ground_cfg (include/liso_ground.h)"""
    _fields_ = [("batch", _i), ("n_max", _i), ("point_stride", _i), ("width", _i), ("height", _i),
                ("sensor_height", ctypes.c_double), ("delta_r", ctypes.c_double)]


class TargetsCfg(ctypes.Structure):
    """mirror of liso_targets_cfg (include/liso_detector.h)"""
    _fields_ = [("batch", _i), ("n_boxes", _i), ("h", _i), ("w", _i), ("range_x", _f), ("range_y", _f)]


class DbscanCfg(ctypes.Structure):
    """mirror of liso_dbscan_cfg (include/liso_flow_cluster.h)"""
    _fields_ = [("batch", _i), ("gx", _i), ("gy", _i), ("window", _i), ("min_samples", _i), ("eps", _f), ("flow_weight", _f)]


class CorrCfg(ctypes.Structure):
    """mirror of liso_corr_cfg (include/liso_slim.h)"""
    _fields_ = [("batch", _i), ("h", _i), ("w", _i), ("dim", _i), ("levels", _i), ("radius", _i)]


class KabschCfg(ctypes.Structure):
    """mirror of liso_kabsch_cfg (include/liso_kabsch.h)"""
    _fields_ = [("batch", _i), ("n_points", _i), ("n_slots", _i), ("point_stride", _i), ("flow_stride", _i),
                ("slope", _f), ("scale_fg", _f), ("scale_bg", _f), ("softness", _i)]


class PillarCfg(ctypes.Structure):
    """mirror of liso_pillar_cfg (include/liso_pillars.h)"""
    _fields_ = [("x_min", _f), ("y_min", _f), ("z_min", _f), ("vx", _f), ("vy", _f), ("vz", _f), ("gx", _i),
                ("gy", _i), ("max_points", _i), ("max_voxels", _i), ("n_channels", _i)]


PILLARS_MAX_BATCH = 32  # LISO_PILLARS_MAX_BATCH (include/liso_pillars.h): samples of one voxelisation call


class _Everything:
    def __contains__(self, name):
        return True


class KernelTimer:
    """Optional HIP-event timing of individual C-ABI launches on the current PyTorch stream (used by bench.py for the
    `roofline` object).  Disabled unless bench.py turns it on; costs two event records per timed launch."""

    def __init__(self):
        self.enabled = set()
        self.events = {}
        self.units = {}
        self.bytes = {}
        self.weights = {}
        self.weight = 1.0

    def enable(self, name):
        self.enabled.add(name)
        self.events.setdefault(name, [])

    def enable_all(self):
        """time every `launch()` whatever its name (bench.py: find the kernel family with the largest share of a step)"""
        self.enabled = _Everything()

    def disable_all(self):
        self.enabled = set()

    def launch(self, name, fn, units=None, nbytes=None):
        """`units`: how many work items (queries, points, flops ...) this launch processes, for per-launch algorithmic bytes;
        `nbytes`: algorithmic HBM bytes of a launch whose `units` are flops (the partner of the PMC traffic figure)"""
        if name not in self.enabled:
            return fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        self.events.setdefault(name, []).append((a, b))
        self.weights.setdefault(name, []).append(float(self.weight))
        if units is not None:
            self.units.setdefault(name, []).append(units)
        if nbytes is not None:
            self.bytes.setdefault(name, []).append(nbytes)
        return r

    def mean_units(self, name):
        u = self.units.get(name, [])
        return sum(u) / len(u) if u else None

    def durations_ms(self, name):
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in self.events.get(name, [])]

    def weighted_total_ms(self, name):
        """sum of the launch durations x the weight that was set when each was recorded (`weight` = share of the launch that belongs
        to one unit of work: 1 / batch for launches that serve a batch of units)"""
        return sum(d * w for d, w in zip(self.durations_ms(name), self.weights.get(name, [])))

    def reset(self):
        for k in self.events:
            self.events[k] = []
        self.units = {}
        self.bytes = {}
        self.weights = {}


TIMER = KernelTimer()


def _declare(l):
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(l, name)  # AttributeError here == header/library mismatch, fail loudly
        fn.restype = res
        fn.argtypes = args
