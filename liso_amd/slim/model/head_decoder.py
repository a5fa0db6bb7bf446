"""HeadDecoder of SLIM: network output [B,H,W,8(+1)] -> per-point flow / class predictions.

Mirror of liso/slim/model/head_decoder.py (HeadDecoder.concat2network_output :37-65, apply_output_modification :67-298,
apply_flow_to_points :300-408, forward :410-496, artificial_network_output :517-717, artificial_{flow,logit}_network_output
:734-955, scale_gradient :720-726).  Same names, keyword arguments and returned keys; `Munch` is the attribute dict of
liso_amd.utils.config.  In-place writes of the reference that mutate caller tensors (`coords[~valid] = 0`,
`points_h[~mask] = 0`) are replaced by out-of-place `torch.where` with identical values.
"""
from typing import Dict

import numpy as np
import torch

from liso_amd.utils.graph_safety import channel_extrema, two_stage_amax, two_stage_amin
from torch import nn

from liso_amd.slim.slim_loss.numerical_stability import normalized_sigmoid_sum
from liso_amd.slim.slim_loss.static_aggregation import (
    BevGatherPlan,
    batched_grid_data_to_pointwise_data,
    compute_batched_bev_static_aggregated_flow,
    compute_pointwise_static_aggregated_flow,
)
from liso_amd.utils.bev_utils import get_voxel_center_coords_m
from liso_amd.utils.config import AttrDict as Munch


def homogenize_coors(coors):
    assert coors.shape[-1] == 3
    return torch.cat([coors, torch.ones(list(coors.shape[:-1]) + [1], dtype=coors.dtype, device=coors.device)], dim=-1)


def scale_gradient(tensor, scaling):
    """reference :720-726"""
    if scaling == 1.0:
        return tensor
    if scaling == 0.0:
        return tensor.detach()
    assert scaling > 0.0
    return tensor * scaling - tensor.detach() * (scaling - 1.0)


def castf(tensor):
    return tensor if tensor.dtype in {torch.float32, torch.float64} else tensor.float()


class HeadDecoder(nn.Module):
    def __init__(self, cfg, name, bev_extent, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.cfg, self.name, self.bev_extent = cfg, name, bev_extent
        self._centers = {}  # (grid size, device) -> ([H,W,2] fp64 cell centres, [H,W,4] homogeneous), uploaded once

    def _gt_static_flows(self, inv_odom, pc, homog):
        """reference :127-157 -- the odometry's static flow of every BEV cell and point, (inv_odom - I) applied as fp64
        broadcast multiply-adds.  (The reference's einsum is a [3x4]x[4xN] fp64 GEMM, which rocBLAS runs with a 128x128
        DGEMM tile: 28 ms per call at N = 120k, measured -- 70 % of the first SLIM step for a quantity forward() then
        discards.)  It depends on the sweep only, so the 6 RAFT iterations of a step share one evaluation."""
        # (the stream is part of the key: a hit hands out tensors that were produced on, and belong to the allocator pool of, the
        # stream that filled the cache -- another stream would read them without an event in between and keep using them after the
        # entry is replaced and its memory recycled; the loop's pipeline runs this decoder on two streams)
        stream_id = torch.cuda.current_stream(inv_odom.device).cuda_stream if inv_odom.is_cuda else 0
        key = (inv_odom, pc, inv_odom._version, pc._version, homog, stream_id)
        c = getattr(self, "_gt_cache", None)
        # (never while a hipGraph is being captured: a hit would leave the computation out of the graph and every replay
        # would keep the values of the capture-time inputs)
        capturing = inv_odom.is_cuda and torch.cuda.is_current_stream_capturing()
        if (not capturing and c is not None and all(a is b for a, b in zip(c[0], key) if torch.is_tensor(a))
                and c[0][2:4] == key[2:4] and c[0][5] == key[5]):
            return c[1]
        M = inv_odom.double() - torch.eye(4, dtype=torch.float64, device=inv_odom.device)[None]
        hb = homog if homog.dim() == 4 else homog[None]  # [B,N,1,4] (per point, pointwise decoding) or the shared [H,W,4]
        gt_static_flow = (M[:, None, None, :2, 0] * hb[..., 0:1] + M[:, None, None, :2, 1] * hb[..., 1:2]
                          + M[:, None, None, :2, 3]).to(torch.float32)  # cell centres have z = 0, w = 1
        p64 = pc[:, :, :3].to(torch.float64)
        gt_pointwise_static_flow = (M[:, None, :3, 0] * p64[..., 0:1] + M[:, None, :3, 1] * p64[..., 1:2]
                                    + M[:, None, :3, 2] * p64[..., 2:3] + M[:, None, :3, 3]).to(torch.float32)
        if capturing:
            return gt_static_flow, gt_pointwise_static_flow
        self._gt_cache = (key, (gt_static_flow, gt_pointwise_static_flow))
        return self._gt_cache[1]

    def _extent_vectors(self, device):
        key = str(device)
        c = getattr(self, "_extent_cache", None)
        if c is None or c[0] != key:
            e = np.asarray(self.bev_extent, dtype=np.float64)
            self._extent_cache = (key, torch.from_numpy(e[:2].copy()).to(device), torch.from_numpy((e[2:] - e[:2]).copy()).to(device))
        return self._extent_cache[1], self._extent_cache[2]

    def _cell_centers(self, final_grid_size, device):
        key = (tuple(int(v) for v in final_grid_size), str(device))
        if key not in self._centers:
            centers_np = get_voxel_center_coords_m(np.array(self.bev_extent), final_grid_size)
            homog = np.concatenate([centers_np, np.zeros_like(centers_np[..., :1]), np.ones_like(centers_np[..., :1])], axis=-1)
            self._centers[key] = (torch.from_numpy(centers_np).to(device), torch.from_numpy(homog).to(device))
        return self._centers[key]

    def concat2network_output(self, *, logits, static_flow, dynamic_flow, weight_logits_for_static_aggregation=None):
        assert logits.shape[1] == 4 and static_flow.shape[1] == 2 and dynamic_flow.shape[1] == 2
        assert (weight_logits_for_static_aggregation is None) == (not self.cfg.model.predict_weight_for_static_aggregation)
        parts = [logits, static_flow, dynamic_flow]
        if weight_logits_for_static_aggregation is not None:
            assert weight_logits_for_static_aggregation.shape[1] == 1
            parts.append(weight_logits_for_static_aggregation)
        return torch.cat(parts, dim=1).permute(0, 2, 3, 1)

    def apply_output_modification(self, network_output, dynamicness_threshold, *, pc, pointwise_voxel_coordinates_fs,
                                  pointwise_valid_mask, filled_pillar_mask, inv_odom, per_point_cluster_idxs_gt=None,
                                  gt_flow_bev=None, ohe_gt_stat_dyn_ground_label_bev_map=None,
                                  dynamic_flow_is_non_rigid_flow=False,
                                  overwrite_non_filled_pillars_with_default_flow: bool = True,
                                  overwrite_non_filled_pillars_with_default_logits: bool = True, gather_plan=None,
                                  pointwise=None):
        """`pointwise` (extension, see _forward_pointwise): the "maps" are per-point rows [B,N,1,C]; dict with the pillar
        centres of the points and the BEV-wide extrema of the raw logit channels."""
        dev = network_output.device
        flow_dim = 2
        assert 3 == len(filled_pillar_mask.shape) == len(network_output.shape) - 1
        assert filled_pillar_mask.shape[-2:] == network_output.shape[-3:-1]
        filled_pillar_mask = filled_pillar_mask[..., None]
        nod = {}
        if self.cfg.model.predict_weight_for_static_aggregation is not False:
            nod["weight_logits_for_static_aggregation"] = network_output[..., -1]
            network_output = network_output[..., :-1]
        assert network_output.shape[-1] == 4 + 2 * flow_dim
        nod.update({  # reference :104-113
            "disappearing_logit": network_output[..., 0:1], "static_logit": network_output[..., 1:2],
            "dynamic_logit": network_output[..., 2:3], "ground_logit": network_output[..., 3:4],
            "static_flow": network_output[..., 4:4 + flow_dim],
            "dynamic_flow": network_output[..., 4 + flow_dim:4 + 2 * flow_dim],
        })
        final_grid_size = network_output.shape[1:3]
        assert pointwise_voxel_coordinates_fs.shape[-1] == 2
        # ground-truth static flow of every BEV cell / point from the odometry (fp64 einsum, :127-157)
        if pointwise is not None:
            centers, homog = pointwise["centers"], pointwise["homog"]
            if pointwise.get("extremes") is not None:  # the True / False logit modes take extrema over the whole BEV map
                mx, mn = pointwise["extremes"]
                for ch, k in enumerate(("disappearing_logit", "static_logit", "dynamic_logit", "ground_logit")):
                    nod[k]._bev_extreme = (mx[ch], mn[ch])
        else:
            centers, homog = self._cell_centers(final_grid_size, inv_odom.device)
        gt_static_flow, gt_pointwise_static_flow = self._gt_static_flows(inv_odom, pc, homog)
        nod, static_aggr_trafo, not_enough_points = artificial_network_output(
            network_output_dict=nod, dynamicness_threshold=dynamicness_threshold, cfg=self.cfg,
            ohe_gt_stat_dyn_ground_label_bev_map=ohe_gt_stat_dyn_ground_label_bev_map, gt_flow_bev=gt_flow_bev,
            gt_static_flow=gt_static_flow, filled_pillar_mask=filled_pillar_mask, pc=pc,
            pointwise_voxel_coordinates_fs=pointwise_voxel_coordinates_fs.to(dev),
            pointwise_valid_mask=pointwise_valid_mask.to(dev), voxel_center_metric_coordinates=centers,
            overwrite_non_filled_pillars_with_default_flow=overwrite_non_filled_pillars_with_default_flow,
            overwrite_non_filled_pillars_with_default_logits=overwrite_non_filled_pillars_with_default_logits,
            gather_plan=gather_plan, pointwise=pointwise is not None)
        disappearing_logit = nod["disappearing_logit"][..., 0]
        is_static, groundness = nod["is_static"], nod["groundness"]
        masked_static_aggr_flow = nod["masked_static_aggr_flow"]
        static2 = masked_static_aggr_flow if self.cfg.model.use_static_aggr_flow_for_aggr_flow else nod["static_flow"]
        dyn2 = nod["dynamic_flow"] * (1.0 - groundness[..., None])
        if dynamic_flow_is_non_rigid_flow:  # reference :249-267
            dyn2 = static2 * (1.0 - groundness[..., None]) + dyn2
        aggregated2 = torch.where(is_static[..., None], static2, dyn2)
        # every map the per-point gather needs, packed once (2-D flows get their zero z column here; the 3-D flow maps
        # of the reference's Munch are views into this tensor):
        #   0 disappearing | 1 disappearing_logit | 2:5 class_probs | 5:8 class_logits | 8:11 dynamic_flow |
        #   11:14 static_flow | 14:17 aggregated_flow | 17:20 static_aggr_flow | 20:23 is_static, is_dynamic, is_ground
        z1 = torch.zeros_like(disappearing_logit)[..., None]
        flags = torch.stack([is_static, nod["is_dynamic"], nod["is_ground"]], dim=-1)
        packed = torch.cat([torch.sigmoid(nod["disappearing_logit"]), nod["disappearing_logit"], nod["class_probs"],
                            nod["class_logits"], nod["dynamic_flow"], z1, nod["static_flow"], z1, aggregated2, z1,
                            nod["static_aggr_flow"], z1, flags.to(z1.dtype)], dim=-1)
        modified = Munch(disappearing=packed[..., 0], disappearing_logit=disappearing_logit,
                         class_probs=nod["class_probs"], class_logits=nod["class_logits"], staticness=nod["staticness"],
                         dynamicness=nod["dynamicness"], groundness=groundness, is_static=is_static,
                         is_dynamic=nod["is_dynamic"], is_ground=nod["is_ground"], dynamic_flow=packed[..., 8:11],
                         static_flow=packed[..., 11:14], aggregated_flow=packed[..., 14:17],
                         static_aggr_flow=packed[..., 17:20], packed=packed)
        masked_static_aggr_flow3 = torch.cat([masked_static_aggr_flow, z1], dim=-1)
        return (modified, nod, gt_flow_bev, gt_static_flow, gt_pointwise_static_flow, nod["masked_gt_static_flow"],
                masked_static_aggr_flow3, nod.get("masked_weights_for_static_aggregation", None), static_aggr_trafo,
                not_enough_points)

    def apply_flow_to_points(self, *, modified_output_bev_img, pointwise_voxel_coordinates_fs, pointwise_valid_mask,
                             gather_plan=None):
        """reference :300-408 -- gather 3 bool + 20 distinct float channels per point (one 23-channel gather: the booleans
        ride along as 0/1 floats, default 0 == False)"""
        m = modified_output_bev_img
        if "packed" in m:
            flts = m.packed
        else:  # a caller-built Munch without the packed tensor: same channel layout
            flts = torch.cat([torch.stack([m.disappearing, m.disappearing_logit], dim=-1), m.class_probs, m.class_logits,
                              m.dynamic_flow, m.static_flow, m.aggregated_flow, m.static_aggr_flow,
                              torch.stack([m.is_static, m.is_dynamic, m.is_ground], dim=-1).to(m.staticness.dtype)], dim=-1)
        assert flts.shape[-1] == 23, flts.shape
        pf = batched_grid_data_to_pointwise_data(flts, pointwise_voxel_coordinates_fs, pointwise_valid_mask, default_value=0.0,
                                                 plan=gather_plan)
        dis, dis_l, probs, logits, dyn, stat, agg, saf, flg = torch.split(pf, [1, 1, 3, 3, 3, 3, 3, 3, 3], dim=-1)
        pb = flg.detach() > 0.5
        st, dy, gr = torch.unbind(probs, dim=-1)
        return Munch(disappearing_logit=dis_l[..., 0], disappearing=dis[..., 0], class_logits=logits, class_probs=probs,
                     staticness=st, dynamicness=dy, groundness=gr, is_static=pb[..., 0], is_dynamic=pb[..., 1],
                     is_ground=pb[..., 2], dynamic_flow=dyn, static_flow=stat, aggregated_flow=agg, static_aggr_flow=saf)

    def forward(self, network_output, dynamicness_threshold, *, pc, pointwise_voxel_coordinates, pointwise_valid_mask,
                filled_pillar_mask, odom, inv_odom, summaries, gt_flow_bev=None, per_point_cluster_idxs_gt=None,
                ohe_gt_stat_dyn_ground_label_bev_map=None, dynamic_flow_is_non_rigid_flow=False, gather_plan=None,
                pointwise_only=False, aggregated_flow_only=False, eval_flows_only=False):
        """reference :410-496.  `gather_plan` (extension): a BevGatherPlan of (pointwise_voxel_coordinates // final_scale,
        pointwise_valid_mask) to reuse across the RAFT iterations of one cloud; built here when absent.
        `pointwise_only` (extension, training): return the per-point predictions, `static_aggr_trafo`, `not_enough_points`
        and `dynamicness_threshold` only -- everything the losses read -- without `dense_maps` / `modified_network_output`.
        `aggregated_flow_only` (extension, inference; with `pointwise_only`): the caller reads nothing but `aggregated_flow`; when that
        does not depend on the static aggregation (model.use_static_aggr_flow_for_aggr_flow False) the Kabsch fit is skipped.
        `eval_flows_only` (extension, inference; with `pointwise_only`): the caller reads `static_flow`, `aggregated_flow` and
        `static_aggr_flow` only (the flows SLIM's validation evaluates): one decode of those three after the Kabsch fit."""
        coors_fs = torch.div(pointwise_voxel_coordinates, self.cfg.model.u_net.final_scale, rounding_mode="trunc")
        if gather_plan is None:
            gather_plan = BevGatherPlan(coors_fs, pointwise_valid_mask, network_output.shape[1:3])
        if (pointwise_only and network_output.is_cuda and gt_flow_bev is None and ohe_gt_stat_dyn_ground_label_bev_map is None
                and self.cfg.model.predict_weight_for_static_aggregation is False):
            return self._forward_pointwise(network_output, dynamicness_threshold, pc=pc, coors_fs=coors_fs,
                                           pointwise_valid_mask=pointwise_valid_mask, filled_pillar_mask=filled_pillar_mask,
                                           inv_odom=inv_odom, dynamic_flow_is_non_rigid_flow=dynamic_flow_is_non_rigid_flow,
                                           gather_plan=gather_plan, aggregated_flow_only=aggregated_flow_only,
                                           eval_flows_only=eval_flows_only)
        (modified, nod, gt_flow_bev, _, _, _, _, _, static_aggr_trafo, not_enough_points) = self.apply_output_modification(
            network_output, dynamicness_threshold, pc=pc, pointwise_voxel_coordinates_fs=coors_fs,
            pointwise_valid_mask=pointwise_valid_mask, filled_pillar_mask=filled_pillar_mask, inv_odom=inv_odom,
            gt_flow_bev=gt_flow_bev, ohe_gt_stat_dyn_ground_label_bev_map=ohe_gt_stat_dyn_ground_label_bev_map,
            dynamic_flow_is_non_rigid_flow=dynamic_flow_is_non_rigid_flow, per_point_cluster_idxs_gt=per_point_cluster_idxs_gt,
            gather_plan=gather_plan)
        pointwise = self.apply_flow_to_points(modified_output_bev_img=modified, pointwise_voxel_coordinates_fs=coors_fs,
                                              pointwise_valid_mask=pointwise_valid_mask, gather_plan=gather_plan)
        retval = Munch(**pointwise, dense_maps=Munch(aggregated_flow=modified.aggregated_flow, static_flow=modified.static_flow),
                       modified_network_output=Munch(nod))
        retval["static_aggr_trafo"] = static_aggr_trafo
        retval["dynamicness_threshold"] = dynamicness_threshold
        retval["not_enough_points"] = not_enough_points
        return retval


    def _forward_pointwise(self, network_output, dynamicness_threshold, *, pc, coors_fs, pointwise_valid_mask, filled_pillar_mask,
                           inv_odom, dynamic_flow_is_non_rigid_flow, gather_plan, aggregated_flow_only=False, eval_flows_only=False):
        """Gather first, decode second.  Every step of apply_output_modification (:67-298) is pointwise in the BEV cell --
        defaults at unfilled pillars, softmax, thresholds, flow selection -- except (a) the BEV-wide extrema of the
        True / False logit modes and (b) the static aggregation, which itself only reads the maps at the points' pillars and
        evaluates one rigid transform per sample at the pillar centres.  So the 8 raw channels are read at every point's
        pillar first (one 8-channel gather instead of a 3- and a 23-channel one) and the same code then runs on [B,N,1,C]
        rows: 2.2x fewer elements than 512^2 maps at 120k points, and the adjoint scatters 8 channels instead of 26."""
        S, N = pointwise_valid_mask.shape
        H, W = int(network_output.shape[1]), int(network_output.shape[2])
        om = self.cfg.model.output_modification
        raw = batched_grid_data_to_pointwise_data(network_output, coors_fs, pointwise_valid_mask, 0.0, plan=gather_plan)
        from liso_amd.slim.model import fused_decode as FD

        if getattr(self, "fused_decoding", True) and FD.decode_supported(self.cfg, network_output) and pc.dtype == torch.float32:
            # the whole per-point decode as two launches around the Kabsch fit (include/liso_slim_decode.h)
            extremes = None
            if any(v is True or v is False for v in (om.static_logit, om.dynamic_logit, om.ground_logit)):
                extremes = channel_extrema(network_output[..., :4].detach())
            meta = FD.DecodeMeta(self.cfg, self.bev_extent, gather_plan, filled_pillar_mask, extremes, dynamicness_threshold,
                                 pc.contiguous(), non_rigid=dynamic_flow_is_non_rigid_flow)
            if aggregated_flow_only and not self.cfg.model.use_static_aggr_flow_for_aggr_flow and not torch.is_grad_enabled():
                eye = _cached_eye(S, raw.device)
                return Munch(aggregated_flow=FD.decode_points(raw, eye, meta, want=("agg_flow",))["agg_flow"],
                             dynamicness_threshold=dynamicness_threshold)
            x, y, w = FD.decode_weights(raw, meta)
            from liso_amd.slim.slim_loss.weighted_pc_alignment import batched_weighted_pc_alignment

            static_aggr_trafo, not_enough_points = batched_weighted_pc_alignment(
                x, y, w, pointwise_valid_mask,
                use_epsilon_on_weights=self.cfg.losses.unsupervised.use_epsilon_for_weighted_pc_alignment)
            if eval_flows_only and not torch.is_grad_enabled():
                o = FD.decode_points(raw, static_aggr_trafo, meta, want=("stat_flow", "agg_flow", "saf_flow"))
                return Munch(static_flow=o["stat_flow"], aggregated_flow=o["agg_flow"], static_aggr_flow=o["saf_flow"],
                             static_aggr_trafo=static_aggr_trafo, dynamicness_threshold=dynamicness_threshold,
                             not_enough_points=not_enough_points)
            o = FD.decode_points(raw, static_aggr_trafo, meta)
            fl = o["flags"]
            return Munch(disappearing_logit=o["dis_logit"], disappearing=o["dis"], class_logits=o["logits"], class_probs=o["probs"],
                         staticness=o["staticness"], dynamicness=o["dynamicness"], groundness=o["groundness"], is_static=fl[..., 0],
                         is_dynamic=fl[..., 1], is_ground=fl[..., 2], dynamic_flow=o["dyn_flow"], static_flow=o["stat_flow"],
                         aggregated_flow=o["agg_flow"], static_aggr_flow=o["saf_flow"], static_aggr_trafo=static_aggr_trafo,
                         dynamicness_threshold=dynamicness_threshold, not_enough_points=not_enough_points)
        safe = gather_plan.lin64.clamp(min=0)
        filled_pt = (filled_pillar_mask.reshape(-1)[safe].view(S, N) & pointwise_valid_mask).view(S, N, 1)
        extremes = None
        if any(v is True or v is False for v in (om.static_logit, om.dynamic_logit, om.ground_logit)):
            lg = network_output[..., :4].detach()
            extremes = channel_extrema(lg)  # (staged: no inter-block semaphores, see liso_amd/utils/graph_safety.py)
        # metric centre of every point's pillar: get_voxel_center_coords_m's fp64 arithmetic (bev_utils.py:24-40) on the
        # point's own (row, col) -- bit-identical to reading the [H,W,2] centre map, without a 16-byte-row gather
        lo, span = self._extent_vectors(inv_odom.device)
        shape = _cached_vector((float(H), float(W)), inv_odom.device, torch.float64)
        centers_pt = (((coors_fs.to(torch.float64) + 0.5) / shape) * span + lo).view(S, N, 1, 2)
        homog_pt = torch.cat([centers_pt, torch.zeros_like(centers_pt[..., :1]), torch.ones_like(centers_pt[..., :1])], dim=-1)
        (modified, _, _, _, _, _, _, _, static_aggr_trafo, not_enough_points) = self.apply_output_modification(
            raw.view(S, N, 1, raw.shape[-1]), dynamicness_threshold, pc=pc, pointwise_voxel_coordinates_fs=coors_fs,
            pointwise_valid_mask=pointwise_valid_mask, filled_pillar_mask=filled_pt, inv_odom=inv_odom,
            dynamic_flow_is_non_rigid_flow=dynamic_flow_is_non_rigid_flow, gather_plan=gather_plan,
            pointwise=dict(centers=centers_pt, homog=homog_pt, extremes=extremes))
        # invalid rows: the BEV path gathers with default 0 (apply_flow_to_points); the rows decoded above from all-default
        # inputs hold the "unfilled pillar" values instead
        pf = torch.where(pointwise_valid_mask[..., None], modified.packed.view(S, N, 23), 0.0)
        dis, dis_l, probs, logits, dyn, stat, agg, saf, flg = torch.split(pf, [1, 1, 3, 3, 3, 3, 3, 3, 3], dim=-1)
        pb = flg.detach() > 0.5
        st, dy, gr = torch.unbind(probs, dim=-1)
        return Munch(disappearing_logit=dis_l[..., 0], disappearing=dis[..., 0], class_logits=logits, class_probs=probs,
                     staticness=st, dynamicness=dy, groundness=gr, is_static=pb[..., 0], is_dynamic=pb[..., 1],
                     is_ground=pb[..., 2], dynamic_flow=dyn, static_flow=stat, aggregated_flow=agg, static_aggr_flow=saf,
                     static_aggr_trafo=static_aggr_trafo, dynamicness_threshold=dynamicness_threshold,
                     not_enough_points=not_enough_points)


def artificial_network_output(*, network_output_dict: Dict[str, torch.Tensor], dynamicness_threshold, cfg,
                              ohe_gt_stat_dyn_ground_label_bev_map, gt_flow_bev, gt_static_flow, filled_pillar_mask, pc,
                              pointwise_voxel_coordinates_fs, pointwise_valid_mask, voxel_center_metric_coordinates,
                              overwrite_non_filled_pillars_with_default_flow: bool = False,
                              overwrite_non_filled_pillars_with_default_logits: bool = False, gather_plan=None,
                              pointwise: bool = False):
    """reference :517-717.  `pointwise`: the maps are per-point rows [B,N,1,C] (HeadDecoder._forward_pointwise)."""
    model_cfg = cfg.model
    om = model_cfg.output_modification
    nod = artificial_flow_network_output(network_output_dict=network_output_dict, model_cfg=model_cfg, gt_flow_bev=gt_flow_bev,
                                         gt_static_flow=gt_static_flow)
    nod = artificial_logit_network_output(network_output_dict=nod, model_cfg=model_cfg,
                                          ohe_gt_stat_dyn_ground_label_bev_map=ohe_gt_stat_dyn_ground_label_bev_map,
                                          gt_flow_bev=gt_flow_bev, gt_static_flow=gt_static_flow)
    defaults = {  # reference :566-574
        "disappearing_logit": -100.0, "static_logit": -100.0 if om.static_logit is False else 0.0,
        "dynamic_logit": 0.0 if om.dynamic_logit is True else -100.0, "ground_logit": 0.0 if om.ground_logit is True else -100.0,
        "static_flow": 0.0, "dynamic_flow": 0.0, "static_aggr_flow": 0.0,
    }
    taboo = []
    if not overwrite_non_filled_pillars_with_default_flow:
        taboo += ["static_flow", "dynamic_flow", "static_aggr_flow"]
    if not overwrite_non_filled_pillars_with_default_logits:
        taboo += ["disappearing_logit", "static_logit", "dynamic_logit", "ground_logit"]
    # one masked select over the 8 packed channels instead of one per key (reference :576-590)
    order = ["disappearing_logit", "static_logit", "dynamic_logit", "ground_logit", "static_flow", "dynamic_flow"]
    vals = torch.cat([nod[k] for k in order], dim=-1)
    dvec = []
    for k in order:
        dvec += [float("nan") if k in taboo else defaults[k]] * nod[k].shape[-1]
    dvec_t = _cached_vector(tuple(dvec), vals.device, vals.dtype)
    keep = filled_pillar_mask if not taboo else (filled_pillar_mask | torch.isnan(dvec_t))
    vals = torch.where(keep, vals, dvec_t)
    for k, piece in zip(order, torch.split(vals, [nod[k].shape[-1] for k in order], dim=-1)):
        nod[k] = piece  # one split: its backward is a single cat
    nod["class_logits"] = vals[..., 1:4]  # static | dynamic | ground: adjacent channels of the packed tensor
    nod["class_probs"] = torch.nn.functional.softmax(nod["class_logits"], dim=-1)
    nod["staticness"], nod["dynamicness"], nod["groundness"] = (nod["class_probs"][..., i] for i in range(3))
    nod["is_dynamic"] = nod["dynamicness"] >= dynamicness_threshold
    nod["is_static"] = (nod["staticness"] >= nod["groundness"]) & (~nod["is_dynamic"])
    nod["is_ground"] = ~(nod["is_static"] | nod["is_dynamic"])
    weight_map = nod["staticness"] * castf(filled_pillar_mask[..., 0])
    if model_cfg.predict_weight_for_static_aggregation is not False:  # reference :627-681
        mode = model_cfg.predict_weight_for_static_aggregation
        assert mode in {"sigmoid", "softmax"}
        wl = nod["weight_logits_for_static_aggregation"]
        if mode == "softmax":
            masked = torch.where(filled_pillar_mask[..., 0], wl, torch.ones_like(wl) * (torch.min(wl) - 1000.0))
            shp = masked.shape
            nod["masked_weights_for_static_aggregation"] = torch.reshape(
                torch.nn.functional.softmax(torch.reshape(masked, (-1, shp[-1] * shp[-2])), dim=-1), (-1, *shp[-2:]))
        else:
            gs = filled_pillar_mask.shape[-3:-1]
            nod["masked_weights_for_static_aggregation"] = torch.reshape(
                normalized_sigmoid_sum(logits=torch.reshape(wl, [-1, gs[0] * gs[1]]),
                                       mask=torch.reshape(filled_pillar_mask[..., 0], [-1, gs[0] * gs[1]])), [-1, *gs])
        weight_map = weight_map * nod["masked_weights_for_static_aggregation"]
    if pointwise:
        flows_pt, static_aggr_trafo, not_enough_points = compute_pointwise_static_aggregated_flow(
            pc, pointwise_valid_mask, nod["static_flow"][:, :, 0, :], weight_map[:, :, 0], voxel_center_metric_coordinates[:, :, 0, :],
            use_eps_for_weighted_pc_alignment=cfg.losses.unsupervised.use_epsilon_for_weighted_pc_alignment)
        nod["static_aggr_flow"] = flows_pt[:, :, None, :]
    else:
        nod["static_aggr_flow"], static_aggr_trafo, not_enough_points = compute_batched_bev_static_aggregated_flow(
            pc, pointwise_voxel_coordinates_fs, pointwise_valid_mask, nod["static_flow"], weight_map,
            voxel_center_metric_coordinates,
            use_eps_for_weighted_pc_alignment=cfg.losses.unsupervised.use_epsilon_for_weighted_pc_alignment, plan=gather_plan)
    nod["masked_static_aggr_flow"] = torch.where(filled_pillar_mask, nod["static_aggr_flow"], torch.zeros_like(nod["static_aggr_flow"]))
    nod["masked_gt_static_flow"] = torch.where(filled_pillar_mask, gt_static_flow, torch.zeros_like(nod["masked_static_aggr_flow"]))
    return nod, static_aggr_trafo, not_enough_points


_VECTOR_CACHE = {}


def _cached_eye(n, device):
    key = ("eye", n, str(device))
    if key not in _VECTOR_CACHE:
        _VECTOR_CACHE[key] = torch.eye(4, dtype=torch.float64, device=device)[None].repeat(n, 1, 1).contiguous()
    return _VECTOR_CACHE[key]


def _cached_vector(values, device, dtype):
    """small constant vectors (per-channel defaults) uploaded once per (values, device)"""
    key = (values, str(device), dtype)
    if key not in _VECTOR_CACHE:
        _VECTOR_CACHE[key] = torch.tensor(values, dtype=dtype, device=device)
    return _VECTOR_CACHE[key]


def artificial_flow_network_output(*, network_output_dict, model_cfg, gt_flow_bev, gt_static_flow):
    """reference :734-776"""
    om = model_cfg.output_modification
    nod = network_output_dict
    if om.static_flow == "gt":
        nod["static_flow"] = gt_static_flow
    elif om.static_flow == "zero":
        nod["static_flow"] = _const_like(nod["static_flow"], 0.0)
    elif om.static_flow != "net":
        raise ValueError("unknown output mode: %s" % str(om.static_flow))
    if om.dynamic_flow == "gt":
        nod["dynamic_flow"] = gt_flow_bev
        if model_cfg.dynamic_flow_is_non_rigid_flow:
            nod["dynamic_flow"] = nod["dynamic_flow"] - nod["static_flow"]
    elif om.dynamic_flow == "zero":
        nod["dynamic_flow"] = _const_like(nod["dynamic_flow"], 0.0)
    elif om.dynamic_flow != "net":
        raise ValueError("unknown output mode: %s" % str(om.dynamic_flow))
    nod["dynamic_flow"] = scale_gradient(nod["dynamic_flow"], om.dynamic_flow_grad_scale)
    return nod


def _extreme(a, b, fn):
    """global max / min over two maps (reference: fn(torch.cat([a, b], 0)).detach()).  Pointwise decoding tags the raw
    per-point logit channels with the extrema of the BEV maps they were read from (`_bev_extreme`)."""
    def one(t):
        tag = getattr(t, "_bev_extreme", None)
        if tag is not None:
            return tag[0] if fn is torch.max else tag[1]
        return two_stage_amax(t) if fn is torch.max else two_stage_amin(t)
    return torch.maximum(one(a), one(b)) if fn is torch.max else torch.minimum(one(a), one(b))


def _const_like(ref, value):
    """`value * ones_like(ref)` as an expanded view (value: python scalar or 0-d tensor)"""
    if torch.is_tensor(value):
        return value.to(ref.dtype).expand(ref.shape)
    return ref.new_full((), value).expand(ref.shape)


def artificial_logit_network_output(*, network_output_dict, model_cfg, ohe_gt_stat_dyn_ground_label_bev_map, gt_flow_bev,
                                    gt_static_flow):
    """reference :779-955 (the `net` / on / off modes; the gt_label_based / gt_flow_based modes need dataset labels and
    are reproduced as well)."""
    om = model_cfg.output_modification
    nod = network_output_dict
    ref = nod["static_logit"]
    ohe = ohe_gt_stat_dyn_ground_label_bev_map
    if om.disappearing_logit is True:
        nod["disappearing_logit"] = _const_like(ref, 0.0)
    elif om.disappearing_logit is False:
        nod["disappearing_logit"] = _const_like(ref, -100.0)
    elif om.disappearing_logit != "net":
        raise ValueError("unknown output mode: %s" % str(om.disappearing_logit))
    # static
    if om.static_logit == "gt_label_based":
        assert om.dynamic_logit == "gt_label_based"
        if om.ground_logit is False:
            nod["static_logit"] = 100.0 * (castf(ohe[..., 0:1] | ohe[..., 2:3]) - 1.0)
        else:
            assert om.ground_logit == "gt_label_based"
            nod["static_logit"] = 100.0 * (castf(ohe[..., 0:1]) - 1.0)
    elif om.static_logit == "gt_flow_based":
        assert om.dynamic_logit == "gt_flow_based" and om.ground_logit is False
        is_static = castf(torch.linalg.norm(gt_flow_bev - gt_static_flow, dim=-1, keepdim=True) <= 0.05)
        nod["static_logit"] = 100.0 * (is_static - 1.0)
    elif om.static_logit is True:
        assert om.dynamic_logit is False and om.ground_logit is False
        nod["static_logit"] = _const_like(ref, _extreme(nod["dynamic_logit"], nod["ground_logit"], torch.max) + 100.0)
    elif om.static_logit is False:
        assert om.dynamic_logit is not False or om.ground_logit is not False
        nod["static_logit"] = _const_like(ref, _extreme(nod["dynamic_logit"], nod["ground_logit"], torch.max) - 100.0)
    elif om.static_logit != "net":
        raise ValueError("unknown output mode: %s" % str(om.static_logit))
    # dynamic
    if om.dynamic_logit == "gt_label_based":
        nod["dynamic_logit"] = 100.0 * (castf(ohe[..., 1:2]) - 1.0)
    elif om.dynamic_logit == "gt_flow_based":
        nod["dynamic_logit"] = 100.0 - nod["static_logit"]
    elif om.dynamic_logit is True:
        nod["dynamic_logit"] = _const_like(ref, _extreme(nod["static_logit"], nod["ground_logit"], torch.max) + 100.0)
    elif om.dynamic_logit is False:
        nod["dynamic_logit"] = _const_like(ref, _extreme(nod["static_logit"], nod["ground_logit"], torch.min) - 100.0)
    elif om.dynamic_logit != "net":
        raise ValueError("unknown output mode: %s" % str(om.dynamic_logit))
    # ground
    if om.ground_logit == "gt_label_based":
        nod["ground_logit"] = 100.0 * (castf(ohe[..., 2:3]) - 1.0)
    elif om.ground_logit is True:
        assert om.static_logit is False and om.dynamic_logit is False
        nod["ground_logit"] = _const_like(ref, _extreme(nod["static_logit"], nod["dynamic_logit"], torch.max) + 100.0)
    elif om.ground_logit is False:
        nod["ground_logit"] = _const_like(ref, _extreme(nod["static_logit"], nod["dynamic_logit"], torch.min) - 100.0)
    elif om.ground_logit != "net":
        raise ValueError("unknown output mode: %s" % str(om.ground_logit))
    return nod
