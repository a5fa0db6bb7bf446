"""Training steps of the hot path.

DetectorTrainer.step mirrors the per-iteration body of liso/kabsch/liso_cli.py:362-618 for the CenterPoint-pillar
network (forward -> centerpoint_loss x cm_loss_weight + rotation regulariser -> backward -> AdamW -> OneCycleLR,
optimizer factory liso_cli.py:792-823).  The reference is single-GPU; data parallelism (one process per GPU,
gradient all-reduce over RCCL/xGMI in a single flat bucket overlapped with backward, per-rank BatchNorm) is the
only addition.
"""
import collections
import contextlib
import ctypes
import os

import torch
import torch.distributed as dist

from liso_amd import _lib as L

from liso_amd.losses.centerpoint_loss import centerpoint_loss, rotation_vec_on_unit_circle
from liso_amd.networks.simple_net.simple_net import BoxLearner
from liso_amd.utils import graph_capture as GC
from liso_amd.utils import tensor_tree as TT


def get_optimizer_scheduler(cfg, box_predictor, total_steps=None, flat=False):
    """liso_cli.py:792-823: AdamW(lr, weight_decay 0.01) + OneCycleLR(pct_start 0.4, momentum 0.85-0.95, div 10); training on
    ground truth runs one cycle over `num_training_steps` (+2, as in the reference), training on mined boxes one cycle per
    weight-drop period with final_div_factor 10.  `total_steps` overrides the cycle length (benchmarks)."""
    if flat:  # the same update as one launch over flat buffers (liso_amd/utils/flat_adamw.py, include/liso_optim.h)
        from liso_amd.utils.flat_adamw import FlatAdamW

        opt = FlatAdamW(box_predictor.parameters(), lr=cfg.optimization.learning_rate, weight_decay=0.01)
    else:
        opt = torch.optim.AdamW(box_predictor.parameters(), lr=cfg.optimization.learning_rate, weight_decay=0.01)
    common = dict(optimizer=opt, max_lr=cfg.optimization.learning_rate, pct_start=0.4, base_momentum=0.85, max_momentum=0.95,
                  div_factor=10.0)
    source = cfg.data.setdefault("train_on_box_source", "gt")
    if source == "gt":
        sched = torch.optim.lr_scheduler.OneCycleLR(total_steps=(total_steps or cfg.optimization.num_training_steps) + 2, **common)
    elif source == "mined":
        assert cfg.optimization.rounds.active, "assuming this"
        rounds = cfg.optimization.rounds
        sched = torch.optim.lr_scheduler.OneCycleLR(
            total_steps=(total_steps or rounds.steps_per_round * rounds.drop_net_weights_every_nth_round) + 2, final_div_factor=10,
            **common)
    else:
        raise NotImplementedError(source)
    return opt, sched


def get_slim_optimizer_scheduler(slim_cfg, params, flat=False):
    """slim/experiment.py:200-219: RMSprop(lr = initial) (or Adam) + linear warm-up over `warm_up.step_length` steps, then
    linear decay to 5 % of the initial rate at `iterations.train`.  `flat` (GPU): RMSprop over flat buffers, one update launch
    (liso_amd/utils/flat_adamw.py: FlatRMSprop)."""
    from liso_amd.utils.learning_rate import get_polynomial_decay_schedule_with_warmup

    if slim_cfg.optimizer == "rmsprop" and flat:
        from liso_amd.utils.flat_adamw import FlatRMSprop

        opt = FlatRMSprop(list(params), lr=slim_cfg.learning_rate.initial)
    elif slim_cfg.optimizer == "rmsprop":
        opt = torch.optim.RMSprop(params, lr=slim_cfg.learning_rate.initial)
    elif slim_cfg.optimizer == "adam":
        opt = torch.optim.Adam(params, lr=slim_cfg.learning_rate.initial)
    else:
        raise AssertionError("only rmsprop/adam supported")
    sched = get_polynomial_decay_schedule_with_warmup(
        optimizer=opt, num_warmup_steps=slim_cfg.learning_rate.warm_up.step_length,
        num_training_steps=slim_cfg.iterations.train, lr_end=slim_cfg.learning_rate.initial * 0.05)
    return opt, sched


def gather_gradients(device, params, add=False):
    """`params`: (parameter, its flat-buffer gradient view) whose `.grad` was None during the backward pass.  Their gradient
    tensors -> the flat views by one launch per 48 tensors (liso_gather_f32); `.grad` is the flat view again afterwards.  `add`: the
    second half of a split backward pass adds (nothing arrives there for these parameters today).  -> the source tensors (keep them
    alive until the launch has run: inside a capture they belong to the graph's pool anyway)."""
    jobs = []
    for p_, flat in params:
        g = p_.grad
        p_.grad = flat
        if g is None or g is flat:
            continue
        if add or g.dtype != torch.float32 or g.stride() != flat.stride() or g.shape != flat.shape:
            flat.add_(g) if add else flat.copy_(g)
            continue
        jobs.append((g, flat))
    if not jobs:
        return []
    n = len(jobs)
    src = (ctypes.c_void_p * n)(*[g.data_ptr() for g, _ in jobs])
    dst = (ctypes.c_void_p * n)(*[f.data_ptr() for _, f in jobs])
    cnt = (ctypes.c_size_t * n)(*[g.numel() for g, _ in jobs])
    with torch.cuda.device(device):
        L.check(L.lib().liso_gather_f32(n, src, dst, cnt, L.stream_ptr()), "gather_f32")
    return [g for g, _ in jobs]


_SIDE_STREAMS = {}


def side_stream(device, role, priority=0):
    """The process's side stream for `role` on `device`: ONE HIP stream per (device, role), shared by every trainer of the process.

    HIP binds a stream to one of a few hardware queues when it is first used, in order of first use.  A second LisoLoopTrainer that
    CREATED three more streams next to a first, already stepped one found its streams on queues that its own caller's stream or each
    other already occupied: its three pipeline stages took turns on a queue and its step ran at 11.3 ms instead of 4.37 (the first
    trainer, stepped again afterwards: 4.37; either trainer without overlap: 9.1-9.4; the second with its side streams replaced by
    fresh high-priority ones: 4.39 -- scripts/second_trainer_bisect.py, round 6; rounds 4-5 had seen it as "a trainer built second
    is 1.5x slower, cause not found" and moved bench.py's parity legs into child processes).  Streams are queues, not state: trainers
    of one process share them, an idle trainer leaves nothing on them, two active ones interleave on them.
    Every trainer captures on the shared "flow" stream: correct only while ONE host thread drives all trainers of the process.
    A role has one priority: asking for a cached role with another one is an error."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), role)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = (torch.cuda.Stream(device=device, priority=priority), priority)
    st, made_with = _SIDE_STREAMS[key]
    assert priority == made_with, f"side stream {role!r} exists with priority {made_with}, requested with {priority}"
    return st


def _prepare_device(device, exact):
    """before a trainer builds its network.  `exact`: True = fp32 convolutions on the native fp32 MFMA (2^-24 per product, the reference's
    fp32 semantics; the parity configuration), False = as bf16 hi/lo pairs (F32X3, 2^-16), None = keep mfma_conv.set_fp32_mode's."""
    from liso_amd.utils import mfma_conv as MC

    if exact is not None:
        MC.set_fp32_mode("exact" if exact else "x3")
    if device.type == "cuda":  # (persistent device flag of the sparse canvas convolutions: must exist before the first capture)
        MC._sparse_flag(device)


def _broadcast_replicas(net):  # (replicas start identical: what the DDP constructor would do)
    for t in list(net.parameters()) + list(net.buffers()):
        dist.broadcast(t.data, src=0)


@contextlib.contextmanager
def _captured_training_pass(tr, canvases, second_half=False):
    """prologue and epilogue of a captured training step, around its loss + backward.  `tr` carries `_flat_grad`, `_gather_params`,
    `device`, `_pack_jobs` (recorded in the warm-up: every layer's forward / data-gradient panels then come from ONE launch) and, where
    it has one, `_opt_packs` (then from the AdamW launch: no pack launch, no filter-building copy in this step; requests that table
    does not cover are packed as before).  `canvases`: the leaf inputs.  `second_half` of a backward pass split in two (GradCut):
    gradients and panels of the first stay."""
    from liso_amd.utils import conv_panels as CP

    if not second_half:
        tr._flat_grad.zero_()
        # (no zeroed gradient buffer for a canvas: with .grad = None autograd keeps the first layer's data gradient as the leaf's
        # gradient -- a 134-MB fill and a 400-MB accumulation into zeros per detector step at B = 4 otherwise)
        for c in canvases:
            c.grad = None
        tr._step_table = CP.step_table(tr._pack_jobs, getattr(tr, "_opt_packs", None))
    gathered = tr._gather_params or []
    with CP.step(tr._step_table):
        for p_, _ in gathered:  # (autograd then KEEPS the gradient tensor it is handed instead of adding it into the zeroed slice)
            p_.grad = None
        try:
            yield
        finally:
            tr._gather_keepalive = gather_gradients(tr.device, gathered, second_half)


class DetectorTrainer:
    def __init__(self, cfg, device, compute_dtype=torch.float32, total_steps=None, fused_loss=None, use_graph=False, exact=None,
                 grad_buckets=None, loss_scale="default"):
        """`grad_buckets` (graph path, several ranks): 2 (default) = the step is captured as TWO graphs, cut behind the backbone's first
        block (mfma_conv.GradCut): the gradients of everything downstream of the cut -- 97 % of the parameters -- are all-reduced
        between the two replays and the collective overlaps block 0's backward pass (the layers at the largest resolution), the
        pillar encoder's backward and the second, small all-reduce; 1 = one graph, one all-reduce behind it.  (ROCm refuses external
        events inside a captured graph -- "External events are disallowed in rocm" -- so the signal cannot come from inside ONE
        graph.)  A single rank always runs one graph.
        `exact` (with compute_dtype float32): the arithmetic of the fp32 convolutions, see `_prepare_device`.
        `fused_loss`: activations + decode + CenterPoint loss in one HIP pass (include/liso_detector.h) instead of
        ~140 torch launches; default = whenever the configuration is the overlay the kernel implements and the
        network runs on the GPU.
        `use_graph`: forward + loss + backward of one step (no device->host sync on that path) are captured once per input
        shape into a hipGraph and replayed; new clouds / targets are copied into the captured input buffers.  Gradients live
        in one flat buffer: data parallelism is ONE RCCL all-reduce of that buffer after the replay (no DDP wrapper), then
        the eager AdamW / OneCycleLR step.
        `loss_scale` (compute_dtype float16 only): "dynamic" (the fp16 default) = a loss scale that backs off on overflow and grows
        after clean steps, a float = that fixed scale, None = no scaling.  The state stays on the device (liso_amd/utils/loss_scale.py):
        the backward pass is seeded with it, steps whose gradients overflowed leave parameters and moments untouched.  bf16 / fp32
        trainers take no loss scale."""
        from liso_amd.losses import fused_centerpoint

        self.cfg, self.device = cfg, device
        _prepare_device(device, exact)
        self.use_graph = bool(use_graph) and device.type == "cuda"
        self._graph, self._graph2, self._graph_sig = None, None, None
        self._opt_packs = None
        self.fused_loss = (fused_centerpoint.supports(cfg) and device.type == "cuda") if fused_loss is None else fused_loss
        self.net = BoxLearner(cfg).to(device)
        self.net.model.set_compute_dtype(compute_dtype)
        if self.use_graph and not self.fused_loss:
            # only the fused loss keeps the captured region free of hipMemsetAsync nodes (graph_safety.py): torch's multi-block
            # reductions (centerpoint_loss) put them into the graph
            from liso_amd.utils.graph_safety import require_node_replay

            require_node_replay("DetectorTrainer(use_graph=True) without the fused loss")
        # (the filters stay contiguous fp32 master weights: the kernels pack their panels from them; channels-last parameters would
        # cost a layout copy per pack and strided gradient accumulations -- ~170 extra launches per step, measured)
        self.model = self.net
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        # on the GPU the parameters, their gradients and the AdamW moments are views into four flat buffers: the update is one
        # launch, the gradient all-reduce one collective, zero_grad one memset
        self.optimizer, self.lr_scheduler = get_optimizer_scheduler(cfg, self.net, total_steps, flat=device.type == "cuda")
        self.loss_scaler = None
        if loss_scale == "default":
            loss_scale = "dynamic" if compute_dtype == torch.float16 else None
        if loss_scale is not None:
            if compute_dtype != torch.float16:
                raise ValueError(f"loss scaling is for fp16 training (compute_dtype {compute_dtype})")
            if device.type != "cuda":
                raise ValueError("fp16 training runs on the device kernels only")
            from liso_amd.utils.loss_scale import DeviceLossScale

            if loss_scale == "dynamic":
                self.loss_scaler = DeviceLossScale(device)
            elif isinstance(loss_scale, (int, float)) and not isinstance(loss_scale, bool):
                self.loss_scaler = DeviceLossScale(device, init_scale=float(loss_scale), dynamic=False)
            else:
                raise ValueError(f"loss_scale: 'dynamic', a number or None, got {loss_scale!r}")
            self.optimizer.loss_scale = self.loss_scaler
        if self.world > 1 and not self.use_graph:
            # ~19 MB of fp32 gradients: one flat bucket, launched as backward reaches the first layer's grads
            self.model = torch.nn.parallel.DistributedDataParallel(
                self.net, device_ids=[device.index] if device.type == "cuda" else None, bucket_cap_mb=64,
                broadcast_buffers=False, gradient_as_bucket_view=device.type != "cuda")
        self.n_grad_buckets = 1
        if self.use_graph:
            self._flat_grad = self.optimizer.flat_grad  # data parallelism: SUM all-reduce of this buffer, 1 / world inside the AdamW launch
            if self.world > 1:
                _broadcast_replicas(self.net)
                self.optimizer.grad_scale = 1.0 / self.world
                self._setup_gradient_buckets(grad_buckets)
            elif grad_buckets == 2:  # (one rank, asked for explicitly: the two-graph step without a collective -- tests)
                self._setup_gradient_buckets(2)
        from liso_amd.networks.centerpoint.fused_bn import defer_batch_counters
        self._bn_counters = defer_batch_counters(self.net.model.rpn) + defer_batch_counters(self.net.model.center_head)

    def _setup_gradient_buckets(self, grad_buckets):
        """two gradient buckets: [pillar encoder | backbone block 0] and [everything else] -- the second one is complete when the
        backward pass arrives at the output of block 0 (rpn.py: grad_cut), with block 0's backward (the layers at the largest
        resolution) and the pillar encoder's still to come"""
        from liso_amd.utils import mfma_conv as MC

        rpn = self.net.model.rpn
        if grad_buckets is None:
            grad_buckets = int(os.environ.get("LISO_GRAD_BUCKETS", "2"))
        if grad_buckets < 2 or len(rpn.blocks) < 2 or not hasattr(self.optimizer, "offsets"):
            return
        first = next(rpn.blocks[1].parameters())
        split = self.optimizer.offsets[id(first)]
        # (the flat buffer follows net.parameters(): pillar encoder, blocks 0.., deblocks, head)
        order = [id(p_) for p_ in self.net.parameters() if p_.requires_grad]
        assert all(self.optimizer.offsets[i] < split for i in order[:order.index(id(first))])
        assert all(self.optimizer.offsets[i] >= split for i in order[order.index(id(first)):])
        self._bucket_split = int(split)
        self._grad_cut = MC.GradCut()
        self.n_grad_buckets = 2

    def _reduce_gradients(self, rest_of_backward):
        """SUM all-reduce of the flat gradient buffer over the ranks (the mean's 1 / world is applied inside the AdamW launch).
        Called behind the replay of the (first) graph; `rest_of_backward()` = what is still to run: the second graph (two buckets)
        and the pillar encoder's eager backward."""
        if getattr(self, "skip_collective", False):  # bench.py's measurement of the collective's exposed cost (replicas diverge)
            rest_of_backward()
            return
        if self.n_grad_buckets < 2:
            rest_of_backward()
            dist.all_reduce(self._flat_grad)
            return
        # (the collective runs on the process group's own stream, which waits for the caller's stream as it stands NOW: behind the
        # first graph; the caller's stream goes on with the rest of the backward pass and waits for both collectives at the end)
        w1 = dist.all_reduce(self._flat_grad[self._bucket_split:], async_op=True)
        rest_of_backward()
        w2 = dist.all_reduce(self._flat_grad[:self._bucket_split], async_op=True)
        w1.wait()
        w2.wait()

    def loss(self, pcls, targets, canvas=None):
        """liso_cli.py:452-614.  `canvas`: precomputed pillar canvas (bev, occupancy) -- the hipGraph path"""
        if self.model.training:
            from liso_amd.networks.centerpoint.fused_bn import step_batch_counters
            step_batch_counters(self._bn_counters)
        cfg = self.cfg
        sup = cfg.loss.supervised.supervised_on_clusters
        gt_maps = {a: targets[a] for a in sup.attrs}
        mask = targets["center_bool_mask"]
        if self.fused_loss:
            from liso_amd.losses.fused_centerpoint import fused_centerpoint_loss

            _, _, raw, _ = self.model(None, pcls, None, centermaps_gt=None, decode=False, canvas=canvas)
            total, losses = fused_centerpoint_loss(
                cfg=cfg, raw_box_maps=raw, gt_maps=gt_maps, gt_center_mask=mask,
                ignore_region_is_true_mask=targets.get("ignore_region_is_true_mask", None),
                pillar_center_coors_m=self.net.pillar_center_coors_m)
            return total, losses, None
        pred_boxes, decoded, activated, aux = self.model(None, pcls, None, centermaps_gt=None)
        ignore = targets.get("ignore_region_is_true_mask", torch.zeros_like(mask))
        losses = centerpoint_loss(loss_cfg=cfg.loss, raw_activated_pred_box_maps=activated, decoded_pred_box_maps=decoded,
                                  gt_maps=gt_maps, gt_center_mask=mask,
                                  rotation_loss_weights_map=torch.ones_like(gt_maps["probs"]),
                                  box_prediction_cfg=cfg.box_prediction, ignore_region_is_true_mask=ignore)
        total = 0.0
        for v in losses.values():
            total = total + sup.weight * v
        rr = cfg.box_prediction.rotation_representation
        if rr.method == "vector":  # main_utils.py:119-134
            total = total + rotation_vec_on_unit_circle(activated) * rr.regul_weight
        return total, losses, pred_boxes

    def step(self, pcls, targets, prep=None):
        """`prep` (extension): `self.net.model.pfn.prepare(pcls)` issued earlier (LisoLoopTrainer: on another stream, next to the previous
        step) -- the weight-independent half of the pillar encoder"""
        self.model.train()
        if self.use_graph:
            return self._graph_step(pcls, targets, prep)
        self.optimizer.zero_grad(set_to_none=True)
        total, losses, _ = self.loss(pcls, targets)
        self._backward(total)
        self.optimizer.step()
        self.lr_scheduler.step()
        return total.detach()

    def _backward(self, total):
        """total.backward(), seeded with the device-resident loss scale when there is one (read at run / replay time: no sync)"""
        if self.loss_scaler is None:
            total.backward()
        else:
            total.backward(self.loss_scaler.seed)

    def loss_scale_stats(self):
        """{scale, applied_steps, skipped_steps, growth_tracker} of the fp16 loss scale, None without one (reads the device: a sync)"""
        return None if self.loss_scaler is None else self.loss_scaler.stats()

    def eager_pass(self, pcls, targets):
        """forward + loss + backward with eager launches and NO update: no collective, no optimizer / scheduler step (bench.py
        times individual kernels this way next to graph-replayed steps; every rank may call it independently)"""
        self.model.train()
        saved = [p.grad for p in self.net.parameters()]
        for p in self.net.parameters():
            p.grad = None
        ctx = self.model.no_sync() if hasattr(self.model, "no_sync") else contextlib.nullcontext()
        with GC.frozen_buffers(self.net, keep=lambda k, v: "running" in k or "num_batches" in k), ctx:
            total, _, _ = self.loss(pcls, targets)
            self._backward(total)  # (fp16: seeded with the loss scale like the real step, so the same gradients flow)
        for p, g in zip(self.net.parameters(), saved):
            p.grad = g
        return total.detach()

    # ---- hipGraph path ----------------------------------------------------------------------------------------------
    # The graph holds backbone + head + fused loss, forward and backward (~95 % of the step's launches).  The pillar encoder
    # (voxelise + PFN + scatter; 10 launches) runs eagerly around it: its launches carry the raw clouds' lengths as kernel arguments
    # (the history of that rule, and the capture protocol: liso_amd/utils/graph_capture.py).
    def eval_model(self, val_batches, max_iterations=None, **run_val_args):
        """The detector's counterpart of `SlimTrainer.eval_model`: liso_amd.eval.eval_ours.run_val over `val_batches` (dictionaries
        with `pcls`, `gt_boxes`, `benchmark_gt_boxes` and optionally `pcl_full_w_ground`) in eval mode, then the previous mode again.
        -> the metric dictionary.  No parameter or buffer changes.  `run_val_args` go to run_val as they are (`dataset_kind`,
        `waymo_metrics=True`, `nuscenes_metrics=True` for the nuScenes mAP / NDS under `final_result/NUSC_OFFICIAL/`, ...)."""
        from liso_amd.eval.eval_ours import run_val

        was_training = self.net.training
        self.net.eval()
        try:
            return run_val(self.cfg, val_batches, self.net, max_num_steps=max_iterations, **run_val_args)
        finally:
            self.net.train(was_training)

    @torch.no_grad()
    def summary_images(self, pcls, targets, pred_boxes=None):
        """The training loop's pictures of a batch (reference liso/kabsch/main_utils.py:464-503), as a dictionary of device tensors
        made without a host read; `step` never calls it.  For the first n = min(B, cfg.logging.max_log_img_batches) samples:
        `_post_nms_SHAPES_COMPARISON_PRED_GT` fp32 [n, H, W, 3]: the occupancy image of the clouds on cfg.data.img_grid_size with the
        predictions over it, coloured by confidence, after the picture's NMS (liso_amd/visu/bbox_image.py `draw_box_image`);
        `TARGET_CENTER_HEATMAP` fp32 [n, h, w, 1]: the centre heat map the step regresses against (`targets["probs"]`), a picture as
        it stands.  `pred_boxes` (a padded Shape [B, P]) defaults to `self.net.predict_boxes` on the clouds in eval mode, the
        previous mode set again afterwards, no parameter or buffer changed; their probs go through the sigmoid when
        cfg.box_prediction.activations.probs == "none", as the reference does for the picture."""
        from liso_amd.visu.bbox_image import draw_box_image
        from liso_amd.visu.pcl_image import create_occupancy_pcl_image

        cfg = self.cfg
        if pred_boxes is None:
            was_training = self.net.training
            self.net.eval()
            try:
                pred_boxes, _, _ = self.net.predict_boxes(None, pcls)
            finally:
                self.net.train(was_training)
        preds = pred_boxes.clone()
        if cfg.box_prediction.activations.probs == "none":
            preds.probs = torch.sigmoid(preds.probs)
        canvas = torch.stack([create_occupancy_pcl_image(p, cfg.data.bev_range_m, cfg.data.img_grid_size) for p in pcls]).permute(0, 3, 1, 2)
        n = min(canvas.shape[0], int(cfg.logging.max_log_img_batches))
        return {"_post_nms_SHAPES_COMPARISON_PRED_GT": draw_box_image(cfg=cfg, pred_boxes=preds, gt_boxes=None, canvas_f32=canvas,
                                                                       gt_background_boxes=None, perform_nms=True),
                "TARGET_CENTER_HEATMAP": targets["probs"][:n].to(torch.float32)}

    def _pillars(self, pcls, out=None, prep=None):
        """`out`: (canvas rows [B, gx, gy, 64], occupancy) to write into -- the graph's static inputs (no copy afterwards)"""
        return self.net.model.pfn(pcl_t0=pcls, img_t0=None, out=out, prep=prep)

    def _capture(self, pcls, targets):
        from liso_amd.utils import mfma_conv as MC

        dev = self.device
        # snapshot FIRST: the shape-probing pillar pass below runs the PFN BatchNorm in training mode and must not count as a batch
        with GC.frozen_buffers(self.net) as restore:
            with torch.no_grad():
                bev, occ = self._pillars(pcls)
            self._static_bev = bev.detach().clone().requires_grad_(True)
            self._static_occ = occ.detach().clone()
            self._static_targets = {k: v.to(dev).clone() for k, v in targets.items()}
            side = side_stream(dev, "flow")  # (the process's one: in the loop trainer, SLIM inference's stream)
            self._graph2, self._pack_jobs, self._gather_params = None, [], None
            merged_jobs = []
            cut = self._grad_cut if self.n_grad_buckets == 2 else None
            rpn = self.net.model.rpn

            def body(part=None):
                """part None: the whole step; 1: forward + loss + backward down to the cut; 2: the backward pass above the cut"""
                with _captured_training_pass(self, [self._static_bev], second_half=part == 2):
                    MC.set_direct_grads(True, keep_touched=part == 2)  # gradients of conv / BatchNorm parameters land in the flat buffer without an add each
                    try:
                        if part in (None, 1):
                            rpn.grad_cut = cut
                            try:
                                total, _, _ = self.loss(None, self._static_targets, canvas=(self._static_bev, self._static_occ))
                            finally:
                                rpn.grad_cut = None
                            self._backward(total)
                            self._body_loss = total.detach()
                        if cut is not None and part in (None, 2):
                            cut.finish()
                    finally:
                        MC.set_direct_grads(False, keep_touched=True)
                return self._body_loss

            def after_first_pass():
                # parameters whose gradient no kernel wrote in place during that pass (merged head convolutions, sliced BatchNorm
                # vectors, block-diagonal filters): autograd would launch one `add_` each into the zeroed flat buffer -- instead
                # their gradient tensors are collected behind the backward pass by ONE launch (liso_gather_f32)
                in_place = MC.direct_touched()
                outside = {id(p_) for p_ in self.net.model.pfn.parameters()}  # (the pillar encoder's backward runs outside the graph)
                self._gather_params = [(p_, p_.grad) for p_ in self.net.parameters()
                                       if p_.requires_grad and p_.grad is not None and id(p_) not in in_place and id(p_) not in outside]

            if self._opt_packs is not None:
                self._opt_packs.ensure_current()  # (the warm-up passes of a re-capture read the table's panels)
            GC.warm_up(body, side, pack_jobs=self._pack_jobs, merged_jobs=merged_jobs, after_first=after_first_pass, restore=restore)
            self._attach_optimizer_packs(merged_jobs)
            if cut is None:
                self._graph, self._static_loss = GC.capture(body, side)
            else:  # two graphs sharing one memory pool: the second one reads the leaf gradient and the saved tensors of the first
                self._graph, self._static_loss = GC.capture(lambda: body(1), side)
                self._graph2, _ = GC.capture(lambda: body(2), side, pool=self._graph.pool())

    def _attach_optimizer_packs(self, merged_jobs):
        """after the warm-up of the first capture: the panels / merged filters its pack requests asked for become outputs of the AdamW
        launch (liso_amd/utils/optimizer_packs.py).  Built once: a re-capture for another input signature asks for the same panels."""
        from liso_amd.utils import mfma_conv as MC
        from liso_amd.utils.flat_adamw import FlatAdamW

        if self._opt_packs is not None or not MC.optimizer_packs_enabled() or not self._pack_jobs:
            return
        if not isinstance(self.optimizer, FlatAdamW) or self.optimizer.loss_scale is not None:
            return  # (the fp16 loss-scaled update keeps its own launches)
        from liso_amd.utils.optimizer_packs import OptimizerPacks

        self._opt_packs = OptimizerPacks(self.optimizer, self._pack_jobs, merged_jobs)
        self.optimizer.attach_packs(self._opt_packs)

    def _graph_step(self, pcls, targets, prep=None):
        # what the graph consumes: the [B, 64, gx, gy] canvas (batch size; grid and dtype are fixed per trainer) and the target maps.
        # The clouds themselves never enter it (the pillar encoder runs eagerly in front): their point counts are not part of the key.
        tsig = targets.shapes() if isinstance(targets, _BatchedTargets) else tuple((k, tuple(v.shape), v.dtype) for k, v in sorted(targets.items()))
        from liso_amd.utils import mfma_conv as MC

        sig = (len(pcls), tsig, MC.optimizer_packs_enabled())
        if self._graph is None or sig != self._graph_sig:
            self._graph = None
            self._capture(pcls, targets)
            self._graph_sig = sig
        # the eager pillar encoder writes straight into the graph's input buffers (its own backward runs on saved feature rows)
        bev, occ = self._pillars(pcls, out=(self._static_bev.detach().permute(0, 2, 3, 1), self._static_occ), prep=prep)
        with torch.no_grad():
            stage = []  # (one launch for all target tensors: _lib.multi_copy)
            if isinstance(targets, _BatchedTargets):
                off = {}
                for t in targets.per_sample:  # (running offset per key: samples may carry more than one row)
                    for k, v in t.items():
                        o = off.get(k, 0)
                        stage.append((self._static_targets[k][o:o + v.shape[0]], v))
                        off[k] = o + v.shape[0]
            else:
                for k, v in targets.items():
                    stage.append((self._static_targets[k], v))
            L.multi_copy(stage)
        if self._opt_packs is not None and sig[2]:
            # the captured step reads panels the optimizer wrote: repack (one launch) if anything else has touched a parameter since
            self._opt_packs.ensure_current()
        self._graph.replay()

        def rest_of_backward():
            if self._graph2 is not None:  # (two gradient buckets: the backward pass above the cut)
                self._graph2.replay()
            if bev.requires_grad:  # the pillar encoder's own parameters: its backward runs eagerly on the replayed d loss / d canvas
                bev.backward(self._static_bev.grad)

        if self.world > 1:
            self._reduce_gradients(rest_of_backward)
        else:
            rest_of_backward()
        self.optimizer.step()
        self.lr_scheduler.step()
        return self._static_loss.clone()


class SlimTrainer:
    """SLIM self-supervised train step, mirror of liso/slim/experiment.py:834-919 (`train_one_step`) with the optimizer /
    schedule factory of :200-219: RMSprop(lr 1e-4) + linear warm-up (2000) then linear decay to 5 %; the loss is the
    un-weighted sum over the 6 RAFT iterations.  The reference cloud of every kNN query is bucketed on the device once
    per step (the reference rebuilds a host KD-tree for each of the 12+ queries).

    `use_graph=True`: forward + loss + backward of one step (≈7 800 kernel launches, no device->host sync) are captured
    once per input shape into a hipGraph and replayed; new sweeps are copied into the captured input buffers.  Gradients
    live in one flat buffer: data parallelism is one RCCL all-reduce of that buffer after the replay (no DDP wrapper),
    then the eager RMSprop step."""

    def __init__(self, cfg, device, num_train_samples=1000, use_graph=False, exact=None):
        """`exact`: the arithmetic of the fp32 convolutions (True: the parity configuration, False: the production default), see
        `_prepare_device`"""
        from liso_amd.slim.model.slim import SLIM

        _prepare_device(device, exact)
        self.cfg, self.slim_cfg, self.device = cfg, cfg.SLIM, device
        self.net = SLIM(cfg, num_train_samples=num_train_samples).to(device)
        self.model = self.net
        self.use_graph = bool(use_graph) and device.type == "cuda"
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        if self.world > 1 and not self.use_graph:
            self.model = torch.nn.parallel.DistributedDataParallel(
                self.net, device_ids=[device.index] if device.type == "cuda" else None, bucket_cap_mb=64,
                broadcast_buffers=False, gradient_as_bucket_view=True)
        # (flat buffers unless DistributedDataParallel owns the gradients as views of ITS buckets)
        flat = device.type == "cuda" and self.model is self.net
        self.optimizer, self.lr_scheduler = get_slim_optimizer_scheduler(self.slim_cfg, self.net.parameters(), flat=flat)
        self._flat_opt = hasattr(self.optimizer, "flat_grad")
        import numpy as np
        half = 0.5 * np.array(cfg.data.bev_range_m, dtype=np.float32)
        self.bev_extent = np.concatenate([-half, half], axis=0)
        self._graph, self._graph_sig = None, None
        if self.use_graph:
            from liso_amd.utils.graph_safety import require_node_replay

            require_node_replay("SlimTrainer(use_graph=True)")
            # once-per-step weight gradients of the update block (deferred_wgrad.py): inside a captured graph the gate adds them
            # into the flat gradient buffer itself ("direct"); returned to autograd they would go through AccumulateGrad nodes
            # bound to the warm-up's stream -- a cross-stream hop the capture cannot contain (wrong losses / crashes, measured)
            self.net.raft_network.defer_update_block_wgrad = "direct"
            params = [p for p in self.net.parameters() if p.requires_grad]
            if self._flat_opt:  # the optimizer's own flat gradient buffer (parameters, gradients, square averages: one element order)
                self._flat_grad = self.optimizer.flat_grad
            else:
                self._flat_grad = torch.zeros(sum(p.numel() for p in params), dtype=torch.float32, device=device)
                off = 0
                for p in params:  # gradients are views into one flat buffer: one memset, one all-reduce
                    p.grad = self._flat_grad[off:off + p.numel()].view_as(p)
                    off += p.numel()
            # parameters whose gradients are produced INSIDE the captured step (everything but the pillar encoder, whose backward
            # runs eagerly behind the replay): with .grad = None during the captured backward pass autograd keeps the gradient
            # tensors instead of launching one add_ per parameter into the zeroed flat buffer (~100 launches per step), and one
            # gather launch per 48 tensors moves them into their slices (DetectorTrainer does the same for its few such parameters)
            outside = {id(p) for p in self.net.raft_network.pp_layer.parameters()} if hasattr(self.net.raft_network, "pp_layer") else set()
            self._gather_params = [(p, p.grad) for p in params if id(p) not in outside]
            if self.world > 1:
                _broadcast_replicas(self.net)

    def _inputs(self, sample_t0, sample_t1):
        pc1, m1 = sample_t0["pcl_ta"]["pcl"].to(self.device), sample_t0["pcl_ta"]["pcl_is_valid"].to(self.device)
        pc2, m2 = sample_t1["pcl_ta"]["pcl"].to(self.device), sample_t1["pcl_ta"]["pcl_is_valid"].to(self.device)
        return pc1, m1, pc2, m2

    def loss(self, sample_t0, sample_t1, all_valid=None, canvases=None, gather_plan=None):
        """`all_valid` = (bool, bool): whether every row of the two loss clouds is a real point; evaluated here (the step's
        only device->host sync, before any work is queued) unless the caller already knows.  `canvases`: precomputed pillar
        canvases of both sweeps (the hipGraph path keeps the pillar encoder outside of the graph)."""
        from liso_amd.slim.slim_loss.knn_graph import KnnIndex
        from liso_amd.slim.slim_loss.slim_loss_adaptor import selfsupervisedSlimSingleScaleLoss

        pc1, m1, pc2, m2 = self._inputs(sample_t0, sample_t1)
        if all_valid is None:
            all_valid = (bool(m1.all()), bool(m2.all()))
        ext = [float(v) for v in self.bev_extent]
        # bucket both clouds before the network runs
        idx1 = [KnnIndex(pc1[b][:, :3], extent=ext, all_rows_finite=True) for b in range(pc1.shape[0])] if all_valid[0] else None
        idx2 = [KnnIndex(pc2[b][:, :3], extent=ext, all_rows_finite=True) for b in range(pc2.shape[0])] if all_valid[1] else None
        if canvases is None:
            preds_fw, preds_bw = self.model(sample_t0, sample_t1, None)
        else:
            preds_fw, preds_bw = self.model(sample_t0, sample_t1, None, canvases=canvases, gather_plan=gather_plan)
        kw = dict(moving_thresh_module=self.net.moving_dynamicness_threshold, loss_cfg=self.slim_cfg.losses.unsupervised,
                  model_cfg=self.slim_cfg.model, bev_extent=self.bev_extent, metrics_collector={})
        stacked = getattr(self.net, "stacked_predictions", None)
        if stacked is not None and not self.slim_cfg.model.use_static_aggr_flow_for_aggr_flow:
            # experiment.py:834-919 sums the loss over the RAFT iterations.  Every term of it is a mean over the points /
            # samples of one iteration, so with the iterations stacked along the batch axis (same clouds, same masks) ONE
            # evaluation gives exactly sum_i loss_i / n_it.  (Not used when the loss also updates the dynamicness
            # threshold: that update is sequential in the iterations.)
            sfw, sbw, n_it = stacked
            rep = lambda t: t.repeat(n_it, *([1] * (t.dim() - 1)))  # noqa: E731
            total = n_it * selfsupervisedSlimSingleScaleLoss(
                pc1=rep(pc1), valid_mask_pc1=rep(m1), pc2=rep(pc2), valid_mask_pc2=rep(m2), pred_fw=sfw, pred_bw=sbw,
                knn_index_pc1=None if idx1 is None else idx1 * n_it, knn_index_pc2=None if idx2 is None else idx2 * n_it, **kw)
            return total, preds_fw, preds_bw
        total = torch.zeros(1, device=self.device)
        for pfw, pbw in zip(preds_fw, preds_bw):
            total = total + selfsupervisedSlimSingleScaleLoss(pc1=pc1, valid_mask_pc1=m1, pc2=pc2, valid_mask_pc2=m2, pred_fw=pfw,
                                                              pred_bw=pbw, knn_index_pc1=idx1, knn_index_pc2=idx2, **kw)
        return total, preds_fw, preds_bw

    def step(self, sample_t0, sample_t1, eager=False, update=True):
        """`update=False` (with `eager=True`): forward + loss + backward only -- no collective, no optimizer / scheduler step
        (bench.py times individual kernels this way after a graph-replayed region; every rank may call it independently)."""
        self.model.train()
        if self.use_graph and not eager:
            return self._graph_step(sample_t0, sample_t1)
        total, _, _ = self.loss(sample_t0, sample_t1)
        if self.use_graph:
            self._flat_grad.zero_()
        else:
            self.optimizer.zero_grad(set_to_none=True)
        if not update:
            with self.model.no_sync() if hasattr(self.model, "no_sync") else contextlib.nullcontext():
                total.backward()
            return total.detach()
        total.backward()
        self._reduce_and_update()
        return total.detach()

    def eval_model(self, val_batches, max_iterations=None):
        """liso/slim/experiment.py:560-578 without its TensorBoard writers: the validation pass over `val_batches` ((sample_t0,
        sample_t1) pairs with flow labels) in eval mode, then the previous mode again.  -> (eval_metrics, flow_metrics) of
        liso_amd.slim.validation.run_eval_on_this_dataset.  No parameter, buffer or threshold state changes."""
        from liso_amd.slim.validation import run_eval_on_this_dataset

        was_training = self.net.training
        self.net.eval()
        try:
            return run_eval_on_this_dataset(self.net, val_batches, max_iterations=max_iterations)
        finally:
            self.net.train(was_training)

    def _reduce_and_update(self):
        if self.use_graph and self.world > 1:
            dist.all_reduce(self._flat_grad)
            self._flat_grad.div_(self.world)
        self.optimizer.step()
        self.lr_scheduler.step()

    # ---- hipGraph path (the capture protocol and why the encoder and the sorts stay outside: utils/graph_capture.py) --------
    def _capture(self, sample_t0, sample_t1, all_valid):
        self._static = TT.tree_map((sample_t0, sample_t1), lambda t: t.to(self.device).clone())
        s0, s1 = self._static
        with GC.frozen_buffers(self.net) as restore:  # (before the shape-probing passes)
            # the pillar encoder stays OUTSIDE the graph (as in DetectorTrainer): its canvases are graph inputs, their gradients outputs
            with torch.no_grad():
                canv = self._pillars(sample_t0, sample_t1)
            self._static_canv = tuple(c.detach().clone() for c in canv)
            leaves = [self._static_canv[i].requires_grad_(True) for i in (0, 2)]
            # so does the decoder's point -> cell plan (a torch.sort of 12 x B x N keys): it depends on the sweeps only
            self._static_plan = None
            meta = getattr(self.net, "gather_plan_meta", None)
            if meta is None:
                with torch.no_grad():
                    self.net(s0, s1, None, canvases=self._static_canv)
                meta = getattr(self.net, "gather_plan_meta", None)
            if meta is not None:
                self._static_plan = self.net.build_gather_plan(s0, s1, *meta)
                self._static_plan.lin64  # (its lazily built int64 copy is a graph input too)
            # several ranks + the dynamicness threshold learned from the loss (static aggregation): its updates all-reduce a histogram
            # increment each -- a collective cannot sit inside the graph -- so the captured step only RECORDS the per-rank increments and
            # `_graph_step` reduces and applies them behind the replay (movavg_cls_threshold.py: apply_deferred)
            thr = self.net.moving_dynamicness_threshold
            defer = self.world > 1 and bool(self.slim_cfg.model.use_static_aggr_flow_for_aggr_flow)
            self._thr_items = None

            def body():
                with _captured_training_pass(self, leaves):
                    thr._defer = [] if defer else None
                    try:
                        total, _, _ = self.loss(s0, s1, all_valid, canvases=self._static_canv, gather_plan=self._static_plan)
                        total.backward()
                    finally:
                        self._thr_items, thr._defer = thr._defer, None
                return total.detach()

            self._pack_jobs = []
            self._graph, self._static_loss = GC.capture(body, side_stream(self.device, "flow"), warm_ups=2, pack_jobs=self._pack_jobs,
                                                        restore=restore)

    def capture(self, sample_t0, sample_t1):
        """Capture the graph for inputs shaped like these (no collective is issued: callers running several ranks can
        agree on the outcome before the first step).  Raises whatever the runtime raises if capture is refused."""
        _, m1, _, m2 = self._inputs(sample_t0, sample_t1)
        all_valid = (bool(m1.all()), bool(m2.all()))
        sig = (TT.tree_signature((sample_t0, sample_t1)), all_valid)
        if self._graph is None or sig != self._graph_sig:
            self._graph = None
            self._capture(sample_t0, sample_t1, all_valid)
            self._graph_sig = sig
            return True
        return False

    def _pillars(self, sample_t0, sample_t1):
        from liso_amd.slim.model.slim import get_network_input_pcls

        dev = self.device
        return self.net.raft_network.encode_pillars(get_network_input_pcls(self.cfg, sample_t0, "ta", to_device=dev),
                                                    get_network_input_pcls(self.cfg, sample_t1, "ta", to_device=dev))

    def _graph_step(self, sample_t0, sample_t1):
        if not self.capture(sample_t0, sample_t1):
            TT.tree_copy_(self._static, (sample_t0, sample_t1))
        canv = self._pillars(sample_t0, sample_t1)  # eager, with autograd: the encoder's parameters get their gradients below
        with torch.no_grad():
            for d, c in zip(self._static_canv, canv):
                d.copy_(c.detach(), non_blocking=True)
            if self._static_plan is not None:
                fresh = self.net.build_gather_plan(sample_t0, sample_t1, *self.net.gather_plan_meta)
                for name in ("lin", "sorted_lin", "order", "seg_rank"):
                    getattr(self._static_plan, name).copy_(getattr(fresh, name), non_blocking=True)
                self._static_plan.lin64.copy_(fresh.lin, non_blocking=True)
        self._graph.replay()
        if self._thr_items:  # (several ranks: the threshold updates the captured step recorded, reduced over the ranks and applied)
            with torch.no_grad():
                self.net.moving_dynamicness_threshold.apply_deferred(self._thr_items)
        live = [(canv[i], self._static_canv[i].grad) for i in (0, 2) if canv[i].requires_grad]
        if live:
            torch.autograd.backward([c for c, _ in live], [g for _, g in live])
        self._reduce_and_update()
        return self._static_loss.clone()  # the captured output is overwritten by the next replay


class _Prefetched:
    """what the pipeline of LisoLoopTrainer holds for one announced sample pair: the point flow of stage A and, after stage B, the
    target maps / boxes and the cluster count (pinned host tensor) -- each guarded by the event recorded behind its work.  `shared`:
    the voxelisation of the inference batch the pair went through (_SharedVoxelisation), `index`: the pair's place in that batch."""
    __slots__ = ("pair", "flow", "done", "targets", "boxes", "cluster_count", "shared", "index")

    def __init__(self, pair, flow, done, targets=None, boxes=None, cluster_count=None, shared=None, index=None):
        self.pair, self.flow, self.done = pair, flow, done
        self.targets, self.boxes, self.cluster_count = targets, boxes, cluster_count
        self.shared, self.index = shared, index

    def is_for(self, pair):
        return self.pair[0] is pair[0] and self.pair[1] is pair[1]


class _SharedVoxelisation:
    """the one voxelisation of an inference batch (stage A: the t0 sweeps of its pairs, then the t1 sweeps), kept for the detector
    steps on those pairs: `prep` = pp_layer.prepare(clouds), `ready` = the event recorded right behind it on the stream that issued
    it, `geometry` = the pillar geometry it was made with.  It lives exactly as long as a pipeline entry of one of its pairs or a
    detector step's autograd node refers to it; the consumers only read it."""
    __slots__ = ("prep", "clouds", "ready", "geometry", "seen")

    def __init__(self, prep, clouds, ready, geometry):
        self.prep, self.clouds, self.ready, self.geometry = prep, clouds, ready, geometry
        self.seen = set()  # streams other than the issuing one that its tensors are marked as in use on


def _pillar_geometry(pfn):
    """what must agree for two PointsPillarFeatureNetWrapper to voxelise a cloud identically"""
    return (tuple(float(v) for v in pfn.pc_range), tuple(float(v) for v in pfn.voxel_size), tuple(pfn.grid), pfn.max_num_points,
            pfn.max_voxels, pfn.num_input_channels)


class _BatchedTargets(dict):
    """target maps of a batch given as one dict per sample ([1, ...] tensors): behaves like the concatenated dict (built lazily,
    one torch.cat per key) and lets the graph path copy sample by sample into its captured inputs without concatenating"""

    def __init__(self, per_sample):
        super().__init__()
        self.per_sample = list(per_sample)
        for k in self.per_sample[0]:
            dict.__setitem__(self, k, None)

    def __getitem__(self, k):
        v = dict.__getitem__(self, k)
        if v is None:
            v = torch.cat([t[k] for t in self.per_sample], dim=0)
            dict.__setitem__(self, k, v)
        return v

    def get(self, k, default=None):
        return self[k] if k in self else default

    def items(self):
        return [(k, self[k]) for k in self.keys()]

    def values(self):
        return [self[k] for k in self.keys()]

    def shapes(self):
        rows = {k: sum(t[k].shape[0] for t in self.per_sample) for k in self.per_sample[0]}
        return tuple((k, (rows[k],) + tuple(v.shape[1:]), v.dtype) for k, v in sorted(self.per_sample[0].items()))


class LisoLoopTrainer:
    """One fused LISO iteration per sample pair: SLIM forward (no_grad) -> per-point flow ->
    FlowClusterDetector (BEV dynamicness, DBSCAN, region moments, z-fit, filters, Kabsch heading/velocity) -> rotated NMS
    (pre 1000 / post 100 / IoU 0.1, liso_config.yml:4,27-28) -> CenterPoint target maps -> detector train step.
    The reference runs these stages as separate jobs that exchange files (flow export: slim/experiment.py:363-471;
    box mining + box DB: tracker/; training: liso_cli.py); here the tensors stay in HBM from the sweep to the gradient.
    Box-DB augmentation and tracking between the stages are outside this loop."""

    def __init__(self, cfg, device, compute_dtype=torch.float32, total_steps=None, slim_state_dict=None, use_graph=False,
                 overlap=False, infer_batch=2, flow_ahead=0, exact=None, share_voxelisation=True):
        """`use_graph`: the frozen SLIM inference (one capture per input shape) and the detector's forward+loss+backward are
        replayed from hipGraphs; the flow clustering in between stays eager (its box count sizes the padded Shape).
        `overlap`: step(pair_i, upcoming=(pair_i+1, pair_i+2)) runs the iteration as a three-stage software pipeline on
        three HIP streams (see _stage_a / _stage_b below); results are those of the one-stream loop.
        `infer_batch`: pairs per SLIM inference replay; `flow_ahead`: steps by which an inference batch is issued BEFORE stage B needs
        its first flow (0: just in time -- stage B of the next two pairs then queues behind a whole batch replay).  The pipeline uses
        up to `2 + flow_ahead + infer_batch - 1` announced pairs.
        `share_voxelisation` (LISO_SHARE_VOXELISATION=0 overrides): every sweep is voxelised once -- the frozen SLIM inference puts
        both sweeps of its pairs through one pillar-encoder call, and the detector step reads its t0 clouds' rows out of that call's
        voxelisation (see _step_batch); False: two encoder calls per inference and the detector voxelises again, as before round 12."""
        from liso_amd.networks.flow_cluster_detector.flow_cluster_detector import FlowClusterDetector
        from liso_amd.slim.model.slim import SLIM

        self.cfg, self.device = cfg, device
        _prepare_device(device, exact)  # (`exact`: SLIM's convolutions; the detector's too when compute_dtype is float32)
        self.use_graph = bool(use_graph) and device.type == "cuda"
        self._graph_infer = self.use_graph and use_graph in (True, "infer")
        self._graph_det = self.use_graph and use_graph in (True, "detector")
        self._graph_mine = self.use_graph and use_graph is True
        sync = lambda: torch.cuda.synchronize(device)  # noqa: E731
        self._infer_graphs, self._mine_graphs = GC.GraphLRU(sync), GC.GraphLRU(sync)
        # real sweeps differ in their point count from sample to sample: the padded loss clouds are grown to the next multiple of
        # `infer_point_bucket` rows (TT.pad_pcl_ta) so that the inference graph's input signature repeats, and at most `max_infer_graphs`
        # captured graphs (each with its static inputs and a private memory pool) stay resident, least recently used first out
        tcfg = cfg.data.tracking_cfg
        self.infer_point_bucket = int(tcfg.setdefault("infer_point_bucket", 8192))
        self.max_infer_graphs = int(tcfg.setdefault("max_infer_graphs", 8))
        # stage B's captured graphs are keyed on the same bucket-padded shapes (plus the full cloud's padded length): resident graphs
        # per mining stream, and the number of captures after which a new signature runs the eager fixed-slot path instead of evicting
        # a graph whose replays may still be in flight
        self.max_mine_graphs = int(tcfg.setdefault("max_mine_graphs", 6))
        self.mine_capture_budget = int(tcfg.setdefault("mine_capture_budget", 24))
        self.mine_capture_window = int(tcfg.setdefault("mine_capture_window", 400))
        self.mine_captures, self.mine_eager_fallbacks = 0, 0
        self._mine_calls, self._mine_capture_calls, self._mine_fallback_warned = 0, [], False
        self._views = collections.OrderedDict()  # id(sample) -> (sample, bucket-padded view); the samples themselves are never edited
        self.overlap = bool(overlap) and device.type == "cuda"
        self.infer_batch, self.flow_ahead = int(infer_batch), int(flow_ahead)
        self.box_capacity, self.capacity_overflows = int(cfg.data.tracking_cfg.setdefault("flow_cluster_capacity", 64)), 0
        self._flow_stream, self._mine_stream, self._main_used_static = None, None, None
        self._inputs_ready = None  # event on the caller's stream at the head of a step: the side streams' reads of `upcoming` wait on it
        self._flows, self._mined = [], []
        self.slim = SLIM(cfg, num_train_samples=1000).to(device)
        if slim_state_dict is not None:
            self.slim.load_state_dict(slim_state_dict)
        self.slim.eval()
        for p_ in self.slim.parameters():  # frozen: its packed convolution panels are built once and never re-packed
            p_.requires_grad_(False)
        self.cluster_detector = FlowClusterDetector(cfg).to(device)
        self.detector = DetectorTrainer(cfg, device, compute_dtype=compute_dtype, total_steps=total_steps, use_graph=self._graph_det)
        if device.type == "cuda":
            # three streams in all (the caller's, A, B): HIP multiplexes streams onto 4 hardware queues, and two streams on one
            # queue take turns.  Graph capture / warm-up of both networks borrows stream A.
            # (one set per device and PROCESS, not per trainer: side_stream)
            self._flow_stream = side_stream(device, "flow")
            self._mine_stream = side_stream(device, "mine0", priority=-1)  # many tiny kernels + host reads: dispatch first
            # stage B is a chain of ~100 dependent small launches; under contention it is the slowest stage (the host waits ~1.4 ms
            # per step for it).  LISO_MINE_STREAMS=2 alternates consecutive pairs between two mining streams (two chains in
            # flight): 4.46-4.65 instead of 4.6-4.8 ms per step on one GPU, but that is the 4th stream -- one more (RCCL's, in a
            # multi-GPU run) and two streams share a hardware queue (measured with 3 mining streams: 6.4 ms).  Default 1.
            n_mine = max(1, int(os.environ.get("LISO_MINE_STREAMS", "1")))
            self._mine_streams = [self._mine_stream] + [side_stream(device, f"mine{k}", priority=-1) for k in range(1, n_mine)]
            self._mine_turn = 0
        # compute units the captured SLIM inference's persistent 3x3 convolutions may take while the pipeline overlaps it with the
        # detector step (0 = all): half the chip by default, see _infer_flow_padded
        self.infer_cus = 0
        if device.type == "cuda" and self.overlap:
            n_cu = torch.cuda.get_device_properties(device).multi_processor_count
            self.infer_cus = int(os.environ.get("LISO_INFER_CUS", str(n_cu // 2)))
            if self.infer_cus >= n_cu:
                self.infer_cus = 0
        self._pillar_prep = None  # (clouds, pfn.prepare(clouds), event) of the next detector step
        self._prep_ahead = os.environ.get("LISO_PREP_AHEAD", "1") != "0"
        self.share_voxelisation = bool(share_voxelisation) and os.environ.get("LISO_SHARE_VOXELISATION", "1") != "0"
        self.slim.raft_network.encode_once = self.share_voxelisation
        # stage A's inference calls / the voxelisation calls they issued (one each when shared, two otherwise) / detector steps that
        # took their rows out of a stage-A voxelisation
        self.stage_a_replays, self.stage_a_voxelisations, self.shared_prep_steps = 0, 0, 0
        self._infer_vox_calls, self._step_shared = 0, []
        self.pre_nms, self.post_nms = tcfg.max_num_boxes_before_nms, tcfg.max_num_boxes_after_nms
        self.nms_iou = cfg.setdefault("nms_iou_threshold", 0.1)

    @torch.no_grad()
    def mine_boxes(self, sample_t0, sample_t1):
        """-> (Shape [B,K] after NMS, padded with zeros; point flow [B,N,3])"""
        flow = self._infer_flow(sample_t0, sample_t1)  # one direction, last RAFT iteration
        _, boxes = self._targets_from_flow(sample_t0, flow)
        return boxes, flow

    _stack_samples = staticmethod(TT.tree_stack)

    def _pad_loss_cloud(self, sample):
        """the sample with the point axis of `pcl_ta` (TT.pad_pcl_ta) and of `pcl_full_w_ground_ta` (NaN rows at the end: no box
        contains them) grown to the next multiple of `infer_point_bucket`.  A new dict: the caller's sample is not modified."""
        pa, bk = sample["pcl_ta"], self.infer_point_bucket
        n = pa["pcl"].shape[1]
        pad = (-n) % bk if bk > 1 else 0
        full = sample.get("pcl_full_w_ground_ta")
        fpad = (-full.shape[1]) % bk if (bk > 1 and torch.is_tensor(full) and full.dim() == 3) else 0
        if pad == 0 and fpad == 0:
            return sample
        out = {**sample, "pcl_ta": TT.pad_pcl_ta(pa, n + pad)}
        if fpad:
            out["pcl_full_w_ground_ta"] = torch.nn.functional.pad(full, (0, 0, 0, fpad), value=float("nan"))
        return out

    def _view(self, sample):
        """bucket-padded view of a sample, built once per sample object and kept on the trainer (bounded, oldest first out).  The
        three pipeline stages run on different streams: the padding launches are followed by an event, a stage that meets the view on
        another stream waits for it and marks the padded tensors as in use there (they must not be recycled under that stream when
        the entry leaves the cache)."""
        cuda = self.device.type == "cuda"
        cur = torch.cuda.current_stream(self.device) if cuda else None
        hit = self._views.get(id(sample))
        if hit is not None and hit[0] is sample:
            self._views.move_to_end(id(sample))
            _, v, ev, made_on, seen = hit
            if cuda and ev is not None and cur.cuda_stream != made_on and cur.cuda_stream not in seen:
                cur.wait_event(ev)
                for t in self._padded_tensors(sample, v):
                    t.record_stream(cur)
                seen.add(cur.cuda_stream)
            return v
        v = self._pad_loss_cloud(sample)
        ev = None
        if cuda and v is not sample:
            ev = torch.cuda.Event()
            ev.record(cur)
        self._views[id(sample)] = (sample, v, ev, cur.cuda_stream if cuda else None, set())  # (the strong reference pins id(sample))
        while len(self._views) > 64:
            self._views.popitem(last=False)
        return v

    @staticmethod
    def _padded_tensors(sample, view):
        """the tensors `_pad_loss_cloud` created for `view` (those that are not the sample's own)"""
        out = []
        if view["pcl_ta"] is not sample["pcl_ta"]:
            out += [view["pcl_ta"][k] for k in ("pcl", "pcl_is_valid", "pillar_coors")]
        if view.get("pcl_full_w_ground_ta") is not sample.get("pcl_full_w_ground_ta"):
            out.append(view["pcl_full_w_ground_ta"])
        return out

    def _infer_view(self, sample):
        """what the frozen SLIM inference reads from a (padded) sample: the loss cloud, the odometry and the network-input clouds --
        samples whose OTHER tensors differ in shape (the full cloud with ground) still stack into one inference batch"""
        v = self._view(sample)
        key = "pcl_full_w_ground_ta" if self.cfg.data.use_ground_for_network else "pcl_full_no_ground_ta"
        return {"pcl_ta": v["pcl_ta"], "gt": {"odom_ta_tb": v["gt"]["odom_ta_tb"]}, key: list(sample[key])}

    def _infer_flow(self, sample_t0, sample_t1):
        """frozen SLIM inference of one sample pair (any batch size): eager pillar encoder + one hipGraph replay per input signature.
        Eager and replayed calls see the same (bucket-padded) clouds: their results are bit-identical.  -> flow [B, N, 3] of the
        sample's own rows."""
        n_true = sample_t0["pcl_ta"]["pcl"].shape[1]
        flow = self._infer_flow_padded(self._infer_view(sample_t0), self._infer_view(sample_t1))
        return flow if flow.shape[1] == n_true else flow[:, :n_true].contiguous()

    @staticmethod
    def _graph_inputs(sample_t0, sample_t1):
        """what the captured inference reads from the samples (the network-input clouds go through the eager pillar encoder)"""
        return tuple({"pcl_ta": s_["pcl_ta"], "gt": {"odom_ta_tb": s_["gt"]["odom_ta_tb"]}} for s_ in (sample_t0, sample_t1))

    def _infer_flow_padded(self, sample_t0, sample_t1, share=None):
        """`share`: a list that receives the _SharedVoxelisation of this call's clouds, if it made one"""
        from liso_amd.slim.model.slim import get_network_input_pcls

        raft = self.slim.raft_network
        with torch.no_grad():
            once = raft.encodes_once(len(get_network_input_pcls(self.cfg, sample_t0, "ta")))
        self._infer_vox_calls = 1 if once else 2
        if not self._graph_infer:
            return self.slim.infer_point_flow_t0_t1(sample_t0, sample_t1)
        from liso_amd.utils import mfma_conv as MC

        dev = self.device
        ins = self._graph_inputs(sample_t0, sample_t1)
        # the key holds only what the graph consumes: the padded loss clouds + odometry (the raw clouds' lengths do not enter)
        sig = TT.tree_signature(ins)
        pcls = (get_network_input_pcls(self.cfg, sample_t0, "ta", to_device=dev), get_network_input_pcls(self.cfg, sample_t1, "ta", to_device=dev))
        st = self._infer_graphs.lookup(sig)
        with torch.no_grad():  # pillar encoder eagerly (its rocPRIM sort memsets: liso_amd/utils/graph_safety.py) ...
            # (compact canvases -- mfma_conv.PillarCanvas -- where the encoders' stems read them: the graph's static inputs are then
            # the pillar rows, the cell -> row map and the occupancy map, ~25 MB per pair instead of the dense canvases' 134 MB)
            compact = raft.compact_canvas_ok(dev) if st is None else st["compact"]
            prep = None
            if once:  # ONE voxelisation of both sweeps; the event sits right behind it, not behind the replay: a detector step waits for no more
                clouds = [*pcls[0], *pcls[1]]
                prep = raft.pp_layer.prepare(clouds)
                if share is not None:
                    ready = torch.cuda.Event()
                    ready.record(torch.cuda.current_stream(dev))
                    share.append(_SharedVoxelisation(prep, clouds, ready, _pillar_geometry(raft.pp_layer)))
            if st is None:
                canv = raft.encode_pillars(*pcls, compact=compact, prep=prep)
            else:  # ... straight into the graph's input buffers: no copy, no concatenation of the two sweeps
                raft.encode_pillars(*pcls, out=st["rows"], compact=compact, prep=prep)
            # a device scan (torch.cumsum): eagerly, its memset nodes do not survive in a graph (graph_safety.py)
            thr = self.slim.moving_dynamicness_threshold.value()
        if st is None:
            st = self._infer_graphs.insert(sig, {}, self.max_infer_graphs)  # (the least recently used graphs + their buffers go)
            st["in"] = TT.tree_map(ins, lambda t: t.to(dev).clone())
            B_ = canv[0].shape[0]
            st["compact"] = compact
            if compact:  # (encode_pillars allocated the stacked canvas of both sweeps: it becomes the static input as it is)
                st["rows"], st["canv"] = canv[4], canv
            else:
                rows = torch.cat([canv[0], canv[2]], dim=0).permute(0, 2, 3, 1).contiguous()  # [2B, gx, gy, 64]
                occ = torch.cat([canv[1], canv[3]], dim=0).contiguous()
                st["rows"] = (rows, occ)
                st["canv"] = (rows[:B_].permute(0, 3, 1, 2), occ[:B_], rows[B_:].permute(0, 3, 1, 2), occ[B_:], rows.permute(0, 3, 1, 2), occ)
            st["thr"] = thr.clone()
            s0, s1 = st["in"]
            # In the pipeline the captured inference leaves compute units to the other streams (`infer_cus`, LISO_INFER_CUS=n; 0 = all;
            # mfma_conv.roles_cus: its 3x3 convolutions are persistent blocks, one per CU, and a 60-us launch that holds all 256 makes
            # every kernel of the detector step -- the critical path, ~250 small dependent launches -- wait for it to drain).  Measured:
            # round 5, one box: all CUs 4.23-4.26 ms per step; 128: 4.16-4.17; 144: 4.26; 112: 4.35; 96: 4.34; 64: 4.78 (then stage A is
            # the slowest stage); round 6, one box, 40 steps, twice each: all 4.38 / 4.40; 128: 4.25 / 4.27; 160: 4.39 / 4.40; 96: 4.33 /
            # 4.34 (scripts/infer_cus_sweep.sh).  Default since round 6: half the chip; bench.py's `roofline` prices the capped launches
            # against the peak of the CUs they may use.
            # (HIP maps streams onto 4 hardware queues: capture on a pipeline stream, no extra one)
            with torch.no_grad(), MC.roles_cus(self.infer_cus):
                st["graph"], st["flow"] = GC.capture(
                    lambda: self.slim.infer_point_flow_t0_t1(s0, s1, canvases=st["canv"], dynamicness_threshold=st["thr"]),
                    self._flow_stream, warm_ups=2)
        else:
            TT.tree_copy_(st["in"], ins)
            st["thr"].copy_(thr, non_blocking=True)
        st["graph"].replay()
        return st["flow"]

    def eager_pass(self, sample_t0, sample_t1, also=()):
        return self.eager_pass_batch([(sample_t0, sample_t1)], also)

    def eager_pass_batch(self, pairs, also=()):
        """`_eager_pass_batch` with the convolution plans the pipelined steps use (the kernels bench.py times are the replayed ones)"""
        with self._shared_gpu():
            return self._eager_pass_batch(pairs, also)

    def _shared_gpu(self):
        from liso_amd.utils import mfma_conv as MC

        return MC.shared_gpu() if self.device.type == "cuda" else contextlib.nullcontext()

    def _eager_pass_batch(self, pairs, also=()):
        """the whole iteration on a batch of pairs with eager launches and no parameter update (per-kernel event timing in bench.py).
        `also`: further pairs that join the SLIM inference batch, as in the pipeline's stage A (the kernels are then timed at the
        batch they run at; their launches count len(pairs) / (len(pairs) + len(also)) towards this step)"""
        from liso_amd.utils import mfma_conv as MC

        g, self._graph_infer = self._graph_infer, False
        try:
            allp = [*pairs, *also]
            with torch.no_grad():
                L.TIMER.weight = len(pairs) / len(allp)  # (these launches serve len(allp) pairs, the step consumes len(pairs))
                try:  # (the plans of the captured inference: the same compute-unit cap as in _infer_flow_padded)
                    with MC.roles_cus(self.infer_cus):
                        flow = self._infer_flow_padded(self._stack_infer_views([p_[0] for p_ in allp]), self._stack_infer_views([p_[1] for p_ in allp]))
                finally:
                    L.TIMER.weight = 1.0
                b = flow.shape[0] // len(allp)
                per = [self._targets_from_flow(p_[0], flow[k * b:(k + 1) * b].contiguous())[0] for k, p_ in enumerate(pairs)]
        finally:
            self._graph_infer = g
        targets = per[0] if len(per) == 1 else {k: torch.cat([t[k] for t in per], dim=0) for k in per[0]}
        return self.detector.eager_pass([c for p_ in pairs for c in p_[0]["pcl_full_no_ground_ta"]], targets)

    def _mine_from_graph(self, sample_t0, flow, side):
        """stage B of one sweep pair -- flow clustering, z-fit, filters, Kabsch heading, NMS, target maps with `box_capacity` fixed
        slots -- replayed from a hipGraph on stream `side` (the caller's current stream): ~45 nodes, no scan / sort library call and
        therefore no memset node (liso_amd/utils/graph_safety.py), no host read.  The inputs are the sample's BUCKET-PADDED view
        (`_view`: loss cloud, validity, pillar coordinates, full cloud, all grown to multiples of `infer_point_bucket` like the
        inference graph's) and the padded flow, so sweeps of different point counts share a signature; they are copied into the
        captured inputs by one launch, inv(odom) - I is computed INSIDE the graph (liso_odom_inverse_minus_eye_f64), and all results
        come out of ONE packed buffer that is cloned behind the replay (the next replay overwrites the captured one).  Beyond
        `mine_capture_budget` captures per `mine_capture_window` calls a new signature runs the eager fixed-slot path instead of evicting a graph.
        -> (targets dict, boxes Shape, max cluster count int64 [1])"""
        from liso_amd.kabsch.shape_utils import Shape

        dev = self.device
        v = self._view(sample_t0)
        pa = v["pcl_ta"]
        gt = v[self.cfg.data.odom_source]
        flow = self._pad_flow(flow, pa["pcl"].shape[1])
        ins = {"pcl": pa["pcl"], "valid": pa["pcl_is_valid"], "coors": pa["pillar_coors"], "full": v["pcl_full_w_ground_ta"],
               "flow": flow, "dt": v["src_trgt_time_delta_s"], "odom": gt["odom_ta_tb"]}
        ins = {k: (t if t.device == dev else t.to(dev, non_blocking=True)) for k, t in ins.items()}  # (host-resident loader outputs)
        # (one captured graph -- static inputs, intermediates, packed output -- per mining stream: replays on different streams run
        # concurrently and must not share buffers)
        sig = (side.cuda_stream,) + tuple((k, tuple(t.shape), t.dtype) for k, t in ins.items())
        st = self._mine_graphs.lookup(sig)
        # the budget is a RATE -- at most `mine_capture_budget` captures per `mine_capture_window` mining calls -- so a signature that
        # was evicted from the LRU can be captured again later; a lifetime budget (round 4) left every non-resident signature on the
        # eager path for the rest of a long run
        self._mine_calls += 1
        while self._mine_capture_calls and self._mine_capture_calls[0] <= self._mine_calls - self.mine_capture_window:
            self._mine_capture_calls.pop(0)
        if st is None and len(self._mine_capture_calls) >= self.mine_capture_budget:
            # too many different signatures (bucket too fine for this data): same kernels, launched eagerly, nothing evicted
            self.mine_eager_fallbacks += 1
            if not self._mine_fallback_warned:
                self._mine_fallback_warned = True
                import warnings
                warnings.warn(f"LisoLoopTrainer: {self.mine_capture_budget} box-mining graph captures within {self.mine_capture_window} "
                              "calls -- new point-count signatures run stage B eagerly until the rate drops (raise "
                              "infer_point_bucket or max_mine_graphs)")
            targets, boxes = self._targets_from_flow(sample_t0, flow, capacity=self.box_capacity)
            return targets, boxes, self.cluster_detector.last_num_labels.max().reshape(1)
        if st is not None:
            if st["in_flat"] is not None:  # every input into the captured buffers with ONE launch (a byte-wise concatenation)
                TT.pack_into(st["in_flat"], st["in_layout"], ins)
            else:
                for k, t in ins.items():
                    st["in"][k].copy_(t, non_blocking=True)
        else:
            st = self._mine_graphs.insert(sig, {}, self.max_mine_graphs)
            self.mine_captures += 1
            self._mine_capture_calls.append(self._mine_calls)
            si, st["in_flat"], st["in_layout"] = TT.packed_statics(ins)
            st["in"] = si
            sample = {"pcl_ta": {"pcl": si["pcl"], "pcl_is_valid": si["valid"], "pillar_coors": si["coors"]},
                      "pcl_full_w_ground_ta": si["full"], "src_trgt_time_delta_s": si["dt"],
                      self.cfg.data.odom_source: {"odom_ta_tb": si["odom"]}}

            def body():
                targets, boxes = self._targets_from_flow(sample, si["flow"], capacity=self.box_capacity, padded=True)
                return TT.pack([("t_" + k, t) for k, t in targets.items()] +
                               [("b_" + k, t) for k, t in boxes.__dict__.items() if torch.is_tensor(t)] +
                               [("n_clusters", self.cluster_detector.last_num_labels.max().reshape(1))])

            with torch.no_grad():  # (`side` is the current stream: warm-up and capture stay on it)
                st["graph"], (st["flat"], st["layout"]) = GC.capture(body, side, warm_ups=2)
        st["graph"].replay()
        out = TT.unpack(st["flat"].clone(), st["layout"])
        targets = {k[2:]: t for k, t in out.items() if k.startswith("t_")}
        boxes = Shape(**{k[2:]: t for k, t in out.items() if k.startswith("b_")})
        return targets, boxes, out["n_clusters"]

    @staticmethod
    def _pad_flow(flow, n):
        """point flow [B, n', 3] -> [B, n, 3] (zero rows for the padding points, which are invalid everywhere downstream)"""
        if flow.shape[1] == n:
            return flow
        if flow.shape[1] > n:  # inferred in a batch with a larger point-count bucket: drop the extra padding rows
            return flow[:, :n].contiguous()
        return torch.nn.functional.pad(flow, (0, 0, 0, n - flow.shape[1]))

    def _targets_from_flow(self, sample_t0, flow, capacity=None, odom_minus_eye=None, padded=False):
        """flow clustering -> NMS -> CenterPoint target maps.  Reference-shaped call: two box-count reads size the padded Shape.
        `capacity`: fixed number of box slots and no device->host read at all (FlowClusterDetector.forward); the caller compares
        `self.cluster_detector.last_num_labels` with the capacity later.  Every path (one-stream loop, pipeline stage B eager or
        replayed) works on the sample's bucket-padded view (`_view`) and the flow padded to it: identical inputs, identical boxes;
        `padded`: `sample_t0` already is such a view (the mining graph's static inputs)."""
        from liso_amd.datasets.targets import render_center_targets
        from liso_amd.utils.nms_iou import perform_nms_on_shapes_padded

        with torch.no_grad():
            if not padded:
                sample_t0 = self._view(sample_t0)
            flow = self._pad_flow(flow, sample_t0["pcl_ta"]["pcl"].shape[1])
            sample = dict(sample_t0)
            sample[self.cfg.data.flow_source] = {**sample_t0.get(self.cfg.data.flow_source, {}), "flow_ta_tb": flow}
            boxes = self.cluster_detector(sample, global_step=1, capacity=capacity, odom_minus_eye=odom_minus_eye)
            B = boxes.shape[0]
            if boxes.shape[1] > 0:
                # confidence order, pre-NMS cut, rotated NMS, post-NMS selection, padding values: 3 small launches around the NMS
                # kernels; the fp32 box arrays for the target renderer come out of the last one
                boxes, (pos, dims, rot, valid) = perform_nms_on_shapes_padded(
                    boxes, max_num_boxes=self.post_nms, overlap_threshold=self.nms_iou, pre_nms_max_num_boxes=self.pre_nms,
                    return_target_arrays=True)
                rot = rot[..., None]
            else:  # nothing moved: an all-background target (one padded slot)
                z = torch.zeros((B, 1, 3), device=self.device)
                pos, dims, rot, valid = z, z + 1.0, z[..., :1], torch.zeros((B, 1), dtype=torch.bool, device=self.device)
            out = tuple(int(g) // 4 for g in self.cfg.data.img_grid_size)
            return render_center_targets(pos, dims, rot, valid, out, tuple(self.cfg.data.bev_range_m)), boxes

    # ---- three-stage software pipeline (overlap=True) ------------------------------------------------------------------
    # stage A: frozen SLIM inference of pair i+2 (no host synchronisation)          -> stream _flow_stream
    # stage B: flow clustering + NMS + target maps of pair i+1 (two box-count reads) -> stream _mine_stream
    # stage C: detector train step on pair i                                         -> the caller's stream
    # A and B depend on the sweeps and the frozen SLIM weights only, never on the detector: every pair gets exactly the
    # boxes, targets and parameter update of the one-stream loop (tests/test_gpu_liso_loop.py), the three stages -- each far
    # too small to fill 256 CUs at batch 1 -- share the GPU instead of taking turns, and the host never waits for stage A.
    def _stage_a(self, *pairs):
        """SLIM inference of one or several pairs in ONE batch (same shapes): every convolution of the replay then works on that many
        times the pixels -- at batch 1 they launch 100-200 blocks on 256 CUs"""
        side = self._flow_stream
        if self._inputs_ready is not None:
            side.wait_event(self._inputs_ready)
        if self._main_used_static is not None:  # the static inference buffers were last used on the caller's stream
            side.wait_event(self._main_used_static)
            self._main_used_static = None
        share = [] if self.share_voxelisation else None
        with torch.cuda.stream(side), torch.no_grad():
            # (the flows stay bucket-padded: stage B reads them next to the padded view of the sample)
            if len(pairs) == 1:
                flows = [self._infer_flow_padded(self._infer_view(pairs[0][0]), self._infer_view(pairs[0][1]), share).clone()]  # (the next replay overwrites the static output)
            else:
                # pairs from different point-count buckets share the batch at the largest bucket among them (more padding rows,
                # ignored everywhere): the inference graph's signature is (batch size, largest bucket), not one per combination
                flow = self._infer_flow_padded(self._stack_infer_views([p_[0] for p_ in pairs]), self._stack_infer_views([p_[1] for p_ in pairs]),
                                               share)
                b = flow.shape[0] // len(pairs)
                flows = [flow[k * b:(k + 1) * b].clone() for k in range(len(pairs))]
            done = torch.cuda.Event()
            done.record(side)
        self.stage_a_replays += 1
        self.stage_a_voxelisations += self._infer_vox_calls
        # (the batch holds the t0 clouds of its pairs first, one each: pair k's is sample k of the voxelisation -- _shared_prep checks)
        shared = share[0] if share else None
        for k, (p_, fl) in enumerate(zip(pairs, flows)):
            self._flows.append(_Prefetched(pair=p_, flow=fl, done=done, shared=shared, index=k))

    def _same_shapes(self, pa, pb):
        """can the two pairs share one inference batch?  What the captured inference consumes -- the loss clouds and the odometry --
        must agree in everything but the (bucket-padded) point count, which `_stage_a` levels to the largest bucket of the batch."""
        sig = lambda pair: TT.tree_signature(self._graph_inputs(self._infer_view(pair[0]), self._infer_view(pair[1])), skip_dim=1)  # noqa: E731
        return sig(pa) == sig(pb)

    def _stack_infer_views(self, samples):
        """the inference views of several samples as one batch, levelled to the largest point-count bucket among them"""
        views = [self._infer_view(s_) for s_ in samples]
        n = max(v["pcl_ta"]["pcl"].shape[1] for v in views)
        return self._stack_samples([self._grow_view(v, n) for v in views])

    @staticmethod
    def _grow_view(view, n):
        """an inference view with its loss cloud padded further, to `n` rows"""
        return {**view, "pcl_ta": TT.pad_pcl_ta(view["pcl_ta"], n)}

    @staticmethod
    def _take(store, pair):
        """pop the entry prefetched for exactly these sample objects"""
        for k, e in enumerate(store):
            if e.is_for(pair):
                return store.pop(k)
        return None

    def _stage_b(self, pair):
        f = self._take(self._flows, pair)
        if f is None:
            self._stage_a(pair)
            f = self._take(self._flows, pair)
        side = self._mine_streams[self._mine_turn % len(self._mine_streams)]
        self._mine_turn += 1
        side.wait_event(f.done)
        if self._inputs_ready is not None:
            side.wait_event(self._inputs_ready)
        with torch.cuda.stream(side):
            f.flow.record_stream(side)
            # fixed number of box slots: the host only enqueues (no box-count reads).  The cluster count goes to pinned memory
            # behind the work; step() looks at it when it takes the result (long after this stream got there) and redoes the
            # pair with the reference-shaped call in the -- so far never seen -- case of more clusters than slots.
            count = torch.empty(1, dtype=torch.int64, pin_memory=True)
            if self._graph_mine:
                targets, boxes, n_clusters = self._mine_from_graph(pair[0], f.flow, side)
                count.copy_(n_clusters, non_blocking=True)
            else:
                targets, boxes = self._targets_from_flow(pair[0], f.flow, capacity=self.box_capacity)
                count.copy_(self.cluster_detector.last_num_labels.max().reshape(1), non_blocking=True)
            done = torch.cuda.Event()
            done.record(side)
        self._mined.append(_Prefetched(pair=pair, flow=f.flow, done=done, targets=targets, boxes=boxes, cluster_count=count,
                                       shared=f.shared, index=f.index))

    def _take_mined(self, pair, cur):
        """targets + boxes of `pair` from stage B (made visible to stream `cur`), or None if the pair was not prefetched"""
        m = self._take(self._mined, pair)
        if m is None:
            return None
        self._step_shared.append((m.shared, m.index))
        if os.environ.get("LISO_NO_COUNT_WAIT") == "1":  # (experiment: what does the host's wait for the cluster count cost?  scripts/loop_floor.py)
            cur.wait_event(m.done)
            for t in list(m.targets.values()) + [v for v in m.boxes.__dict__.values() if torch.is_tensor(v)]:
                t.record_stream(cur)
            return m.targets, m.boxes
        m.done.synchronize()  # (stage B of this pair was enqueued one or two steps ago)
        cur.wait_event(m.done)
        if int(m.cluster_count[0]) > self.box_capacity:  # more clusters than slots: the exact, reference-shaped call
            m.flow.record_stream(cur)
            self.capacity_overflows += 1
            return self._targets_from_flow(pair[0], m.flow)
        for t in list(m.targets.values()) + [v for v in m.boxes.__dict__.values() if torch.is_tensor(v)]:
            t.record_stream(cur)  # (allocated on the mining stream, consumed here)
        return m.targets, m.boxes

    def _shared_prep(self, held, pcls):
        """can a detector step on `pcls` read a voxelisation of stage A?  `held`: (voxelisation, index) of the step's pairs, in order.
        Yes when all pairs went through ONE voxelisation as consecutive samples, the clouds it voxelised there are these very tensor
        objects (the detector reads `pcl_full_no_ground_ta`; SLIM reads the same list unless data.use_ground_for_network) and both
        pillar encoders have one geometry -> (voxelisation, first sample), else None: the step then voxelises for itself."""
        if not self.share_voxelisation or not held or len(held) != len(pcls):  # (one cloud per pair: samples of batch size 1)
            return None
        sv, first = held[0]
        if sv is None or any(h[0] is not sv or h[1] != first + j for j, h in enumerate(held)):
            return None
        if first + len(pcls) > len(sv.clouds) or any(sv.clouds[first + j] is not c for j, c in enumerate(pcls)):
            return None
        if sv.geometry != _pillar_geometry(self.detector.net.model.pfn):
            return None
        return sv, first

    def step(self, sample_t0, sample_t1, upcoming=()):
        """one iteration on (sample_t0, sample_t1).  With `overlap`, `upcoming` = the pairs of the following calls (up to
        infer_batch + flow_ahead + 1): stage A (SLIM inference) runs ahead on batches of them, stage B (box mining) up to two pairs ahead, each on
        its own stream.
        Prefetched results are matched by object identity; anything announced but not requested next is dropped."""
        return self.step_batch([(sample_t0, sample_t1)], upcoming)

    def step_batch(self, pairs, upcoming=(), inputs_ready=None):
        """`_step_batch` with the convolution plans of a shared GPU (the three pipeline stages run next to each other)"""
        with self._shared_gpu():
            return self._step_batch(pairs, upcoming, inputs_ready)

    def _step_batch(self, pairs, upcoming=(), inputs_ready=None):
        """one iteration on a BATCH of sweep pairs (each a (sample_t0, sample_t1) with batch size 1): boxes are mined per pair, the
        detector takes ONE train step on the batch of len(pairs) clouds and target maps -- the reference's `batch_size` (2 in
        liso_config.yml:121, 4 in the README commands :637-639), BatchNorm statistics over that batch like the reference's.
        `upcoming`: the pairs of the following calls in order (flat list); the pipeline keeps stage B two batches ahead."""
        cuda = self.device.type == "cuda"
        cur = torch.cuda.current_stream(self.device) if cuda else None
        if cuda:
            # `inputs_ready`: an event the CALLER recorded on the stream that produced / uploaded the announced samples (a DataLoader's
            # copy stream: bench.py --loader).  Every stream of the pipeline that reads them waits for it.  Without it the samples
            # must be complete when they are announced.  (An event recorded HERE on the caller's stream -- the first form of this,
            # early in round 6 -- sits behind the previous step's whole detector work in that stream: the side stages of step i then
            # start only when detector step i - 1 has finished, the host blocks on their results ~2 ms per step and the detector's
            # stream runs dry while the host enqueues the next step: 4.26 instead of 4.10 ms per step, 3.16 instead of 2.72 with both
            # side stages cached; scripts/loop_floor.py.)
            self._inputs_ready = inputs_ready
            if inputs_ready is not None:
                cur.wait_event(inputs_ready)
        mined = []
        self._step_shared = []  # (voxelisation, index) of every pair of this step that came out of the pipeline
        for pair in pairs:
            sample_t0, sample_t1 = pair
            got = self._take_mined(pair, cur) if cuda else None
            if got is None:
                f = self._take(self._flows, pair)
                if f is not None:
                    self._step_shared.append((f.shared, f.index))
                    cur.wait_event(f.done)
                    f.flow.record_stream(cur)
                    flow = f.flow
                else:
                    if self.overlap and cuda:
                        # not prefetched (first call, wrong or missing announcement): the inference runs HERE, on the caller's stream,
                        # with the same static graph buffers, packed weight panels and decoder caches stage A uses on its stream
                        cur.wait_stream(self._flow_stream)
                    with torch.no_grad():
                        flow = self._infer_flow_padded(self._infer_view(sample_t0), self._infer_view(sample_t1))
                got = self._targets_from_flow(sample_t0, flow)
                if self.overlap and f is None:  # the static inference buffers were used on this stream up to here
                    self._main_used_static = torch.cuda.Event()
                    self._main_used_static.record(cur)
            mined.append(got)
        self.last_boxes = mined[-1][1]
        self.last_boxes_batch = [m[1] for m in mined]
        nb = len(pairs)
        if nb == 1:
            targets = mined[0][0]
        else:  # (the graph path copies each sample's maps into its slice of the captured inputs: no concatenation launch)
            targets = _BatchedTargets([m[0] for m in mined])
        pcls = [c for p_ in pairs for c in p_[0]["pcl_full_no_ground_ta"]]
        prep = None
        if self.overlap and cuda and self._pillar_prep is not None:
            key, got_prep, done = self._pillar_prep
            self._pillar_prep = None
            if len(key) == len(pcls) and all(a is b_ for a, b_ in zip(key, pcls)):  # (matched by object identity like every prefetch)
                cur.wait_event(done)
                cat, _, parts = got_prep
                for t in (cat, *parts):
                    t.record_stream(cur)  # (allocated on the mining stream, consumed here and by the encoder's backward)
                prep = got_prep
        if prep is None and self.overlap and cuda:
            hit = self._shared_prep(self._step_shared if len(self._step_shared) == nb else [], pcls)
            if hit is not None:  # stage A voxelised these very clouds for SLIM: the detector reads its samples' rows out of that call
                sv, first = hit
                cur.wait_event(sv.ready)
                if cur.cuda_stream not in sv.seen:  # (allocated on the flow stream, consumed here and by the encoder's backward)
                    cat, _, parts = sv.prep
                    for t in (cat, *parts):
                        t.record_stream(cur)
                    sv.seen.add(cur.cuda_stream)
                prep = (*sv.prep, first, len(pcls))
                self.shared_prep_steps += 1
        self._step_shared = []
        loss = self.detector.step(pcls, targets, prep=prep) if prep is not None else self.detector.step(pcls, targets)
        prep_ahead = self.overlap and cuda and len(upcoming) >= len(pairs) and self._prep_ahead and self.detector.use_graph
        if prep_ahead and self.share_voxelisation:  # (nothing to prepare where the next step will find its clouds in a voxelisation of stage A)
            held = [next((e for e in (*self._mined, *self._flows) if e.is_for(p_)), None) for p_ in upcoming[:len(pairs)]]
            prep_ahead = self._shared_prep([(e.shared, e.index) if e is not None else (None, None) for e in held],
                                           [c for p_ in upcoming[:len(pairs)] for c in p_[0]["pcl_full_no_ground_ta"]]) is None
        if prep_ahead:
            # the weight-independent half of the NEXT step's pillar encoder (voxelisation + decorated rows: ~14 of its ~20 eager
            # launches) now, on the mining stream, next to the detector step that was just enqueued: the detector's stream is the
            # pipeline's critical path, and these launches sat at the head of every step of it
            nxt = [c for p_ in upcoming[:len(pairs)] for c in p_[0]["pcl_full_no_ground_ta"]]
            side = self._mine_stream
            if self._inputs_ready is not None:
                side.wait_event(self._inputs_ready)
            with torch.cuda.stream(side):
                got_prep = self.detector.net.model.pfn.prepare(nxt)
                done = torch.cuda.Event()
                done.record(side)
            self._pillar_prep = (nxt, got_prep, done)
        if self.overlap and len(upcoming) > 0:
            ahead = nb * (1 + len(self._mine_streams))  # stage B runs this many pairs ahead (one batch more than chains in flight)
            fa = nb * self.flow_ahead
            up = list(upcoming[:ahead + fa + self.infer_batch - 1])
            has = lambda store, p: any(e.is_for(p) for e in store)  # noqa: E731
            self._mined = [e for e in self._mined if any(e.is_for(q) for q in up)]
            self._flows = [e for e in self._flows if any(e.is_for(q) for q in up)]
            # stage A first (the GPU works on it while the host walks through stage B).  It runs when a pair that stage B needs now
            # (one of the next two batches) has no flow yet, and then takes every announced pair without a flow -- up to `infer_batch`
            # of the same shape -- in one batch: with k pairs announced it runs every k-1 pairs on k-1 pairs.
            missing = [p_ for k, p_ in enumerate(up) if not has(self._flows, p_) and not has(self._mined, p_)
                       and not any(p_[0] is q[0] and p_[1] is q[1] for q in up[:k])]
            if missing and any(p_ is q for p_ in missing for q in up[:ahead + fa]):
                # a detector step reads stage A's voxelisation only where its pairs sit in ONE inference batch: with batches of whole
                # detector batches, every inference batch ends where a detector batch ends.  A tail short of that waits for the next
                # step's announcements unless stage B needs it now.  (Which pairs share a replay does not change any pair's flow.)
                align = nb if self.share_voxelisation and nb > 1 and self.infer_batch % nb == 0 else 1
                where = {id(p_): k for k, p_ in reversed(list(enumerate(up)))}  # (first place in `up`; up[0] opens the next detector batch)
                while missing:
                    n = 1
                    while n < min(len(missing), self.infer_batch) and self._same_shapes(missing[0], missing[n]):
                        n += 1
                    if align > 1:
                        whole = [m for m in range(n, 0, -1) if (where[id(missing[m - 1])] + 1) % align == 0]
                        if whole:
                            n = whole[0]
                        elif where[id(missing[0])] >= ahead + fa:
                            break
                    self._stage_a(*missing[:n])
                    missing = missing[n:]
            for p_ in up[:ahead]:  # by the time a result is taken, its stream got there long ago
                if not has(self._mined, p_):
                    self._stage_b(p_)
        return loss
