"""hipGraph capture: the one protocol every trainer follows, and the only place of the package that creates a graph.  A capture site
keeps its static inputs, its `body` and what it does behind the replay; each rule below was learned from a fault or a wrong loss.

* WARM UP ON THE CAPTURE STREAM: lazy initialisations and allocator pools stay out of the capture, and the AccumulateGrad nodes of
  the parameters live on the stream of the first backward pass.  A capture on another stream forks into it and the replay computes
  garbage (measured on the detector step: loss 63 instead of 1082).  The flat gradient views are created on the default stream, so
  autograd's stream-mismatch warning (a process-wide switch) is silenced while capturing: `frozen_buffers`.
* SNAPSHOT MODULE STATE FIRST: the shape-probing pillar pass runs the PFN BatchNorm in training mode and must not count as a batch,
  nor may the warm-up passes count as training steps (BatchNorm / threshold statistics and counters).  `frozen_buffers` restores
  behind the warm-up and again on leaving (a capture does not execute; in case the backend ran eagerly).
* SYNCHRONISE BEFORE EVICTING A GRAPH: its replays may still be in flight on a side stream (`GraphLRU.insert`).
* THE PILLAR ENCODER AND ANYTHING THAT SORTS STAY OUTSIDE.  A graph that holds the encoder's launches faults (a GPU memory access
  fault inside a later replay) once a few thousand eager launches -- the optimizer's -- have run between replays
  (scripts/debug_slim_graph_fault*.py: replays alone, copies, allocations, the scheduler are harmless; RMSprop.step() with lr = 0 is
  enough; independent of the convolution backend), and so did replaying them while other encoder calls ran eagerly in the process
  (rounds 2-4, scripts/try_loop_graph3.py PART=pfn).  Root cause (round 5): rocPRIM's large-input radix sort on this ROCm build.  A
  captured torch.sort of more than ~1 M keys makes the replay fault after a few thousand unrelated eager launches
  (scripts/debug_pillar_graph_fault.py: 1.0 M keys replay cleanly, 1.5 M fault), and the memset nodes of scan / sort library calls
  do not survive replays (utils/graph_safety.py).  So SLIM's point -> cell plan (a torch.sort of 12 x B x N = 2.9 M keys) and the
  threshold's torch.cumsum are built eagerly and copied in.  The voxeliser no longer sorts (csrc/pillars.hip: per-cell segments +
  arrival rank): the reproducer replays cleanly and the guard-band runs of tests/test_gpu_canaries.py find no out-of-bounds write in
  any kernel of the encoder, at and beyond its capacities.  It still runs eagerly because its launches carry the raw clouds'
  lengths (host offsets) as kernel arguments, which a graph would freeze: canvases are graph inputs, their gradients graph outputs.
* NO FORKS.  MEASURED, removed: the weight gradients as a parallel branch of the captured backward pass (nothing in the backward
  chain reads them).  Results identical, but every fork edge of a replayed hipGraph costs ~240 us here: detector replay 7.15 vs
  2.54 ms (19 forks + 1 join), loop 6.44 vs 4.38 ms per step.
"""
import collections
import contextlib

import torch


@contextlib.contextmanager
def frozen_buffers(net, keep=lambda k, v: v.is_floating_point() or v.dtype == torch.long):
    """`with frozen_buffers(net) as restore:` -- the entries of `net.state_dict()` that `keep(name, tensor)` selects are copied now;
    `restore()` writes them back, and so does leaving the block.  Autograd's stream-mismatch warning is off inside."""
    saved = {k: v.clone() for k, v in net.state_dict().items() if keep(k, v)}

    def restore():
        with torch.no_grad():
            for k, v in net.state_dict().items():
                if k in saved:
                    v.copy_(saved[k])

    quiet = getattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch", lambda on: None)
    quiet(False)
    try:
        yield restore
    finally:
        restore()
        quiet(True)


def warm_up(body, stream, n=2, pack_jobs=None, merged_jobs=None, after_first=None, restore=None):
    """`body()` n times on `stream`, which starts behind the current stream's work; the current stream goes on behind the warm-up.
    The lists `pack_jobs` / `merged_jobs` receive the weight panels the first pass asks for (conv_panels.recording: a captured step then
    takes them from ONE launch, or from the optimizer's); `after_first()` runs between the first pass and the others; `restore()`
    (frozen_buffers) at the end."""
    from liso_amd.utils import conv_panels as CP

    cur = torch.cuda.current_stream(stream.device)
    if cur != stream:
        stream.wait_stream(cur)
    with torch.cuda.stream(stream):
        if pack_jobs is None and merged_jobs is None:
            body()
        else:
            with CP.recording() as rec:
                body()
            if pack_jobs is not None:
                pack_jobs.extend(rec.jobs)
            if merged_jobs is not None:
                merged_jobs.extend(rec.merged_jobs)
        if after_first is not None:
            after_first()
        for _ in range(n - 1):
            body()
    if cur != stream:
        cur.wait_stream(stream)
    if restore is not None:
        restore()


def capture(body, stream, pool=None, warm_ups=0, **warm_up_args):
    """-> (hipGraph of `body()` captured on `stream`, what `body` returned: the graph's static outputs), after `warm_ups` passes
    of `warm_up`.  `pool`: the memory pool of an earlier graph (`graph.pool()`) whose tensors this one reads."""
    if warm_ups:
        warm_up(body, stream, warm_ups, **warm_up_args)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, pool=pool, stream=stream):
        out = body()
    return graph, out


class GraphLRU(collections.OrderedDict):
    """signature -> dict of one resident captured graph (graph, static inputs and outputs), least recently used first out"""

    def __init__(self, synchronize=torch.cuda.synchronize):
        super().__init__()
        self._synchronize = synchronize  # (the device's; a stub in host tests)

    def lookup(self, sig):
        """the entry of `sig`, now the most recently used one, or None"""
        if sig in self:
            self.move_to_end(sig)
        return self.get(sig)

    def insert(self, sig, entry, capacity):
        """`entry` under `sig` with at most `capacity` (>= 1) entries resident afterwards"""
        capacity = max(int(capacity), 1)
        if len(self) >= capacity:
            self._synchronize()  # (replays of a graph that goes may still be in flight on a side stream)
        while len(self) >= capacity:
            self.popitem(last=False)[1].clear()
        self[sig] = entry
        return entry
