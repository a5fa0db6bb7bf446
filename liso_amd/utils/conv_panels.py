"""Which packed filter panels serve a convolution's (weight, geometry, direction, arithmetic) request -- the one owner of that decision.

The kernels read bf16 / fp16 "panels" packed from the torch-layout fp32 master weights (include/liso_conv.h: liso_conv_pack_weights).
`pack_weights` resolves a request, in this order, against
    1. the open step table   (`with step(table):` -- panels that ONE batched launch packed for a captured step, or that the AdamW
                              launch keeps current: liso_amd/utils/optimizer_packs.py),
    2. the recorder          (`with recording() as rec:` -- a trainer's first warm-up pass; `rec.jobs` / `rec.merged_jobs` then
                              describe the tables of its captured steps),
    3. the rule that a weight which requires grad packs on every captured pass,
    4. the version cache     (per Parameter, until it is modified in place; entries die with their Parameter).
`merged_filters` gives the filter and bias of convolutions that run as ONE launch ("cat": same input, filters concatenated along the
output channels; "blockdiag": each on its own channel slice of one input, filters in diagonal blocks) from the same sources.
`request_key` / `merged_key` are the only spelling of the keys the tables use.  All state lives in `_STATE`."""
import collections
import contextlib
import weakref

import torch

from liso_amd import _lib as L

PackJob = collections.namedtuple("PackJob", "key weight spec for_dgrad mode")          # one recorded request of a Parameter
MergedJob = collections.namedtuple("MergedJob", "kind weights biases spec for_dgrad mode")  # one of a merged filter, by its sources


class _State:
    def __init__(self):
        self.cache = {}              # (id(Parameter), transposed, for_dgrad, mode) -> (weakref, _version, data_ptr, panel)
        self.recorder = None         # the open Recording
        self.table = None            # the open StepTable
        self.optimizer_packs = True  # set_optimizer_packs


_STATE = _State()


def request_key(weight, spec, for_dgrad, mode):
    """key of a request in a step table and in a recording.  A Parameter is known by its identity.  Any other tensor has none -- its
    storage is recycled -- unless a table keeps it (the merged filters of an optimizer table): then its address is stable."""
    if isinstance(weight, torch.nn.Parameter):
        return (id(weight), spec.kh, spec.kw, spec.transposed, bool(for_dgrad), mode)
    return ("merged", weight.data_ptr(), spec.kh, spec.kw, spec.transposed, bool(for_dgrad), mode)


def merged_key(kind, weights):
    """key of the merged filter of these source weights"""
    return (kind,) + tuple(id(w) for w in weights)


# ---- the launchers ---------------------------------------------------------------------------------------------------------------------
def _pack_operands(weight, spec, for_dgrad, mode):
    """-> (fp32 contiguous source, its two leading dimensions, uninitialised panel buffer) of one pack job"""
    w = weight.detach()
    if w.dtype != torch.float32 or not w.is_contiguous():
        w = w.float().contiguous()
    d0, d1 = w.shape[0], w.shape[1]
    K, N = (d1, d0) if spec.transposed == bool(for_dgrad) else (d0, d1)
    dst = torch.empty(L.lib().liso_conv_packed_bytes(K, N, spec.kh * spec.kw, mode), dtype=torch.uint8, device=w.device)
    return w, d0, d1, dst


def _pack_weights(weight, spec, for_dgrad, mode):
    """-> the panels of one request; one liso_conv_pack_weights call"""
    L.require_cuda(weight)
    w, d0, d1, out = _pack_operands(weight, spec, for_dgrad, mode)
    with torch.cuda.device(w.device):
        L.check(L.lib().liso_conv_pack_weights(L.ptr(w), d0, d1, spec.kh, spec.kw, int(spec.transposed), int(bool(for_dgrad)), mode,
                                               L.ptr(out), L.stream_ptr()), "conv_pack_weights")
    return out


def batched_pack(jobs):
    """`jobs`: PackJobs -> {key: packed panels}; one liso_conv_pack_weights_batched call"""
    out, arr = {}, (L.ConvPackJob * len(jobs))()
    keep = []
    for i, (key, weight, spec, for_dgrad, mode) in enumerate(jobs):
        L.require_cuda(weight)
        w, d0, d1, dst = _pack_operands(weight, spec, for_dgrad, mode)
        keep.append(w)
        arr[i] = L.ConvPackJob(w.data_ptr(), dst.data_ptr(), d0, d1, spec.kh, spec.kw, int(spec.transposed), int(bool(for_dgrad)), mode)
        out[key] = dst
    if jobs:
        with torch.cuda.device(jobs[0][1].device):
            L.check(L.lib().liso_conv_pack_weights_batched(arr, len(jobs), L.stream_ptr()), "conv_pack_weights_batched")
    return out


# ---- recording -------------------------------------------------------------------------------------------------------------------------
class Recording:
    """what `recording()` yields.  `jobs`: the PackJobs of the Parameters that were asked for, once per key; `merged_jobs`: the
    MergedJobs of the merged filters that were built (`merged_filters`) and asked for."""

    def __init__(self):
        self.jobs, self.merged_jobs = [], []
        self._seen = set()
        # address of a merged filter built inside -> (the filter, kind, weights, biases).  The entry keeps the filter alive: while it
        # exists no other tensor can live at that address.
        self._built = {}

    def _request(self, weight, spec, for_dgrad, mode):
        if isinstance(weight, torch.nn.Parameter):
            key = request_key(weight, spec, for_dgrad, mode)
            if key not in self._seen:
                self._seen.add(key)
                self.jobs.append(PackJob(key, weight, spec, bool(for_dgrad), mode))
            return
        src = self._built.get(weight.data_ptr())
        if src is not None and src[0].shape == weight.shape:
            key = merged_key(src[1], src[2]) + (spec.kh, spec.kw, spec.transposed, bool(for_dgrad), mode)
            if key not in self._seen:
                self._seen.add(key)
                self.merged_jobs.append(MergedJob(src[1], src[2], src[3], spec, bool(for_dgrad), mode))

    def _note(self, kind, merged, weights, biases):
        if all(isinstance(w, torch.nn.Parameter) for w in weights):
            self._built[merged.data_ptr()] = (merged, kind, list(weights), list(biases))


@contextlib.contextmanager
def recording():
    """`with recording() as rec:` -- the requests made inside are recorded (and served as they would be otherwise).  Leaving the block,
    on an exception too, switches recording off: only `rec.jobs` and `rec.merged_jobs` remain."""
    rec = Recording()
    prev, _STATE.recorder = _STATE.recorder, rec
    try:
        yield rec
    finally:
        _STATE.recorder = prev
        rec._seen, rec._built = None, None


# ---- the step table --------------------------------------------------------------------------------------------------------------------
class StepTable:
    """what the requests of one captured step resolve to.  `panels`: {request_key: panel}; `merged`: {merged_key: (W, bias)} of the
    merged filters that stay current without a launch (an optimizer table's)."""

    def __init__(self, panels, merged=None):
        self.panels, self.merged = panels, merged or {}

    @classmethod
    def packed(cls, jobs, panels=None, merged=None):
        """the panels of `jobs` by one batched launch (none without jobs), next to the `panels` / `merged` that are kept elsewhere"""
        panels = dict(panels or {})
        if jobs:
            panels.update(batched_pack(jobs))
        return cls(panels, merged)


def step_table(jobs, optimizer_packs=None):
    """the table of a captured step that recorded `jobs`: the optimizer table's (liso_amd/utils/optimizer_packs.py) where one is
    attached and the switch is on, else one batched launch; None without jobs (every request then packs for itself)"""
    if optimizer_packs is not None and _STATE.optimizer_packs:
        return optimizer_packs.step_table()
    return StepTable.packed(jobs) if jobs else None


@contextlib.contextmanager
def step(table):
    """`with step(table):` -- the requests inside resolve to `table` first (None: to no table).  The previous state returns on leaving,
    on an exception too.  The halves of a step captured as two graphs open the same table one after the other."""
    prev, _STATE.table = _STATE.table, table
    try:
        yield table
    finally:
        _STATE.table = prev


# ---- the request -----------------------------------------------------------------------------------------------------------------------
def pack_weights(weight, spec, for_dgrad, mode):
    """torch-layout fp32 master weights -> the kernels' packed panels (at most one launch).  Outside a step table the result is cached
    per weight tensor until the tensor is modified in place (`_version`: optimizer steps bump it), so frozen networks pack once and
    the forward / backward of one training step share the panels of a layer."""
    table, rec = _STATE.table, _STATE.recorder
    if table is not None:
        hit = table.panels.get(request_key(weight, spec, for_dgrad, mode))
        if hit is not None:
            return hit
    if rec is not None:
        rec._request(weight, spec, for_dgrad, mode)
    if not isinstance(weight, torch.nn.Parameter):  # (temporaries: their storage is recycled, no stable identity)
        return _pack_weights(weight, spec, for_dgrad, mode)
    if weight.requires_grad and weight.is_cuda and torch.cuda.is_current_stream_capturing():
        # a captured training step must re-pack on every replay (the optimizer changes the weights in between): never let a
        # cache hit elide the pack launch from the graph
        return _pack_weights(weight, spec, for_dgrad, mode)
    cache = _STATE.cache
    key = (id(weight), spec.transposed, bool(for_dgrad), mode)
    hit = cache.get(key)
    if hit is not None and hit[0]() is weight and hit[1] == weight._version and hit[2] == weight.data_ptr():
        return hit[3]
    out = _pack_weights(weight, spec, for_dgrad, mode)
    # the entry dies with the Parameter object (a recycled id() can therefore never hit a stale panel)
    cache[key] = (weakref.ref(weight, lambda _r, k=key: cache.pop(k, None)), weight._version, weight.data_ptr(), out)
    return out


# ---- panels and merged filters that the optimizer keeps current (include/liso_optim.h: liso_adamw_step_packed_f32) ---------------------
def set_optimizer_packs(on):
    """True: a graph-captured detector step reads packed panels, merged filters and concatenated biases that the AdamW launch wrote
    (no pack launch, no filter-building copy in the graph); False: every step packs and merges for itself.  Identical results.  Takes
    effect at the next capture.  -> the previous setting."""
    was, _STATE.optimizer_packs = _STATE.optimizer_packs, bool(on)
    return was


def optimizer_packs_enabled():
    return _STATE.optimizer_packs


# ---- merged filters --------------------------------------------------------------------------------------------------------------------
def _diagonal_blocks(gW, gb, co, ci, on_device):
    """the diagonal blocks of a block-diagonal filter's dense gradient and the slices of its bias gradient; `on_device`: every block by
    one launch (include/liso_optim.h: liso_multi_copy_rows)"""
    gws, gbs, o, c = [], [], 0, 0
    if on_device and gW is not None and gW.dtype == torch.float32:
        jobs = []
        for a, b in zip(co, ci):
            gws.append(gW.new_empty((a, b) + tuple(gW.shape[2:])))
            jobs.append((gws[-1], gW[o:o + a, c:c + b]))
            gbs.append(gb[o:o + a] if gb is not None else None)
            o, c = o + a, c + b
        L.copy_blocks(jobs)
        return gws, gbs
    for a, b in zip(co, ci):
        gws.append(gW[o:o + a, c:c + b].contiguous() if gW is not None else None)
        gbs.append(gb[o:o + a] if gb is not None else None)
        o, c = o + a, c + b
    return gws, gbs


class _BlockDiagonalFilters(torch.autograd.Function):
    """The output convolutions of the detector's heads -- same geometry, each on its own 64-channel slice of the merged hidden map -- as
    ONE convolution: filters [sum co_k, sum ci_k, kh, kw] with head k's filter in its diagonal block and zeros elsewhere, biases
    concatenated.  One forward, one data-gradient and one weight-gradient launch instead of four of each on 1-3 output channels
    (launch-bound: 9 + 21 + 28 us per head at B = 4).  Backward: the diagonal blocks of the dense weight gradient."""

    @staticmethod
    def forward(ctx, n, *wb):
        ws, bs = wb[:n], wb[n:]
        ctx.co, ctx.ci = [w.shape[0] for w in ws], [w.shape[1] for w in ws]
        W = ws[0].new_zeros((sum(ctx.co), sum(ctx.ci)) + tuple(ws[0].shape[2:]))
        ctx.on_device = W.is_cuda and W.dtype == torch.float32
        if ctx.on_device:  # every block and bias by one launch (include/liso_optim.h: liso_multi_copy_rows)
            bias = bs[0].new_empty(sum(ctx.co))
            jobs, o, c = [], 0, 0
            for w, b_, a, b in zip(ws, bs, ctx.co, ctx.ci):
                jobs += [(W[o:o + a, c:c + b], w.detach()), (bias[o:o + a], b_.detach())]
                o, c = o + a, c + b
            L.copy_blocks(jobs)
            return W, bias
        o = c = 0
        for w, a, b in zip(ws, ctx.co, ctx.ci):
            W[o:o + a, c:c + b] = w
            o, c = o + a, c + b
        return W, torch.cat(bs)

    @staticmethod
    def backward(ctx, gW, gb):
        gws, gbs = _diagonal_blocks(gW, gb, ctx.co, ctx.ci, ctx.on_device)
        return (None, *gws, *gbs)


class _KeptFilters(torch.autograd.Function):
    """(merged filter, merged bias) WITHOUT a launch: the buffers of the open step table, which the AdamW launch keeps equal to what the
    sources would build.  Backward: as that of the build -- "cat": the slices of the dense gradients, as torch.cat's; "blockdiag": the
    diagonal blocks."""

    @staticmethod
    def forward(ctx, kind, kept, n, *wb):
        ctx.kind, ctx.co, ctx.ci, ctx.on_device = kind, [w.shape[0] for w in wb[:n]], [w.shape[1] for w in wb[:n]], kept[0].is_cuda
        return kept[0].detach(), kept[1].detach()

    @staticmethod
    def backward(ctx, gW, gb):
        if ctx.kind == "blockdiag":
            gws, gbs = _diagonal_blocks(gW, gb, ctx.co, ctx.ci, ctx.on_device)
            return (None, None, None, *gws, *gbs)
        gws, gbs, o = [], [], 0
        for a in ctx.co:
            gws.append(gW.narrow(0, o, a) if gW is not None else None)
            gbs.append(gb.narrow(0, o, a) if gb is not None else None)
            o += a
        return (None, None, None, *gws, *gbs)


def _frozen_cat(convs):
    """frozen / inference: the concatenated filters are built once per weight version (their packed panels are cached with them)"""
    key = tuple((id(c), c.weight._version, c.weight.data_ptr(), None if c.bias is None else c.bias._version) for c in convs)
    hit = getattr(convs[0], "_liso_merged_weights", None)
    if hit is None or hit[0] != key:
        w = torch.nn.Parameter(torch.cat([c.weight.detach() for c in convs], dim=0), requires_grad=False)
        b = torch.cat([c.bias.detach() for c in convs], dim=0) if convs[0].bias is not None else None
        hit = convs[0]._liso_merged_weights = (key, w, b)
    return hit[1], hit[2]


def merged_filters(kind, convs):
    """-> (W, bias | None) of the convolutions `convs` run as one: "cat" (same geometry and input) or "blockdiag" (same geometry, each on
    its own channels of the input; biases required).  The open step table's always-current pair where it keeps one (no launch), else a
    fresh merge -- which a recording notes, so that the panels asked of it are recorded with their sources; "cat" of weights that take
    no gradient: one merge per weight version."""
    ws, bs = [c.weight for c in convs], [c.bias for c in convs]
    if kind == "cat" and not (torch.is_grad_enabled() and any(w.requires_grad for w in ws)):
        return _frozen_cat(convs)
    biased = bs[0] is not None
    table, rec = _STATE.table, _STATE.recorder
    kept = table.merged.get(merged_key(kind, ws)) if table is not None and biased else None
    if kept is not None:  # (kept current by the AdamW launch: nothing to build)
        return _KeptFilters.apply(kind, kept, len(ws), *ws, *bs)
    if kind == "cat":
        W, bias = torch.cat(ws, dim=0), (torch.cat(bs, dim=0) if biased else None)
    else:
        assert kind == "blockdiag", kind
        W, bias = _BlockDiagonalFilters.apply(len(ws), *ws, *bs)
    if rec is not None and biased:
        rec._note(kind, W, ws, bs)
    return W, bias
