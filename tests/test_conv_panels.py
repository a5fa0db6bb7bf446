"""liso_amd/utils/conv_panels.py on the host: which panel serves a request -- version cache, recording, step table, merged filters.
The two launchers are replaced by stand-ins that count their calls and return fresh uint8 tensors; no device, no library."""
import gc
import weakref

import pytest
import torch

from liso_amd.utils import conv_panels as CP
from liso_amd.utils import mfma_conv as MC

MODE = 0  # (LISO_CONV_BF16; the stand-ins do not look at it)


class _Launches:
    def __init__(self):
        self.single, self.batched = 0, 0

    @property
    def total(self):
        return self.single + self.batched


@pytest.fixture
def launches(monkeypatch):
    n = _Launches()

    def pack_one(weight, spec, for_dgrad, mode):
        n.single += 1
        return torch.empty(4, dtype=torch.uint8)

    def pack_batch(jobs):
        n.batched += 1
        return {job.key: torch.empty(4, dtype=torch.uint8) for job in jobs}

    monkeypatch.setattr(CP, "_pack_weights", pack_one)
    monkeypatch.setattr(CP, "batched_pack", pack_batch)
    yield n
    assert CP._STATE.recorder is None and CP._STATE.table is None and CP._STATE.optimizer_packs  # (no test leaves state behind)


def _convs():
    torch.manual_seed(0)
    return torch.nn.Conv2d(8, 8, 3, padding=1), torch.nn.Conv2d(8, 8, 1)


def _spec(conv):
    return MC.ConvSpec.of(conv)


def test_the_old_entry_points_are_the_owners():
    assert MC.pack_weights is CP.pack_weights and MC.set_optimizer_packs is CP.set_optimizer_packs
    assert MC.optimizer_packs_enabled is CP.optimizer_packs_enabled
    was = MC.set_optimizer_packs(False)
    try:
        assert not CP.optimizer_packs_enabled()
    finally:
        CP.set_optimizer_packs(was)
    assert CP.optimizer_packs_enabled() == was


def test_version_cache_hits_until_the_parameter_changes_and_dies_with_it(launches):
    c3, _ = _convs()
    a = CP.pack_weights(c3.weight, _spec(c3), False, MODE)
    assert CP.pack_weights(c3.weight, _spec(c3), False, MODE) is a and launches.single == 1
    assert CP.pack_weights(c3.weight, _spec(c3), True, MODE) is not a and launches.single == 2  # (the other direction: its own panel)
    with torch.no_grad():
        c3.weight.mul_(2.0)
    b = CP.pack_weights(c3.weight, _spec(c3), False, MODE)
    assert b is not a and launches.single == 3
    assert CP.pack_weights(c3.weight, _spec(c3), False, MODE) is b and launches.single == 3

    ids = {id(c3.weight)}
    assert any(k[0] in ids for k in CP._STATE.cache)
    del c3
    gc.collect()
    assert not any(k[0] in ids for k in CP._STATE.cache)  # the dead entries are gone
    d3, _ = _convs()  # (a new Parameter of the same shape, wherever it lands)
    CP.pack_weights(d3.weight, _spec(d3), False, MODE)
    assert launches.single == 4


def test_a_temporary_is_never_cached(launches):
    c3, _ = _convs()
    w = c3.weight.detach() * 2.0
    CP.pack_weights(w, _spec(c3), False, MODE)
    CP.pack_weights(w, _spec(c3), False, MODE)
    assert launches.single == 2


def test_recording_lists_every_key_once(launches):
    c3, c1 = _convs()
    with CP.recording() as rec:
        for _ in range(2):
            CP.pack_weights(c3.weight, _spec(c3), False, MODE)
            CP.pack_weights(c1.weight, _spec(c1), False, MODE)
        CP.pack_weights(c3.weight, _spec(c3), True, MODE)
    assert [(j.weight, j.for_dgrad) for j in rec.jobs] == [(c3.weight, False), (c1.weight, False), (c3.weight, True)]
    assert [j.key for j in rec.jobs] == [CP.request_key(j.weight, j.spec, j.for_dgrad, j.mode) for j in rec.jobs]
    assert len({j.key for j in rec.jobs}) == 3 and rec.merged_jobs == []


def test_a_recording_that_raises_is_switched_off_and_keeps_nothing(launches):
    c3, c1 = _convs()
    with pytest.raises(RuntimeError, match="refused"):
        with CP.recording() as rec:
            CP.pack_weights(c3.weight, _spec(c3), False, MODE)
            CP.merged_filters("blockdiag", [c1, c1])
            raise RuntimeError("capture refused")
    assert CP._STATE.recorder is None
    n_jobs = len(rec.jobs)
    CP.pack_weights(c1.weight, _spec(c1), False, MODE)  # afterwards: recorded nowhere
    assert len(rec.jobs) == n_jobs == 1 and rec.merged_jobs == []
    refs = [weakref.ref(c3.weight), weakref.ref(c1.weight)]
    del rec, c3, c1
    gc.collect()
    assert all(r() is None for r in refs)  # the module's state holds no reference to the parameters


def test_recorded_keys_resolve_in_the_table_built_from_them(launches):
    """the key a recording hands to the table's constructor is the key a request inside the step looks up -- Parameters, and a merged
    filter that a table keeps"""
    c3, c1 = _convs()
    requests = [(c3.weight, _spec(c3), False), (c1.weight, _spec(c1), False), (c1.weight, _spec(c1), True), (c3.weight, _spec(c3), True)]
    with CP.recording() as rec:
        for w, spec, for_dgrad in requests:
            CP.pack_weights(w, spec, for_dgrad, MODE)
    n = launches.total
    table = CP.StepTable.packed(rec.jobs)
    assert launches.batched == 1 and launches.total == n + 1 and len(table.panels) == 4
    # a merged filter the table keeps (what OptimizerPacks does): stable storage, a panel under the key function's key
    W, bias = torch.zeros(16, 8, 1, 1), torch.zeros(16)
    kept_panel = torch.empty(4, dtype=torch.uint8)
    table.panels[CP.request_key(W, _spec(c1), False, MODE)] = kept_panel
    table.merged[CP.merged_key("cat", [c1.weight, c1.weight])] = (W, bias)
    with CP.step(table):
        got = [CP.pack_weights(w, spec, for_dgrad, MODE) for w, spec, for_dgrad in requests]
        Wm, _ = CP.merged_filters("cat", [c1, c1])
        got_merged = CP.pack_weights(Wm, _spec(c1), False, MODE)
    assert launches.total == n + 1  # no launch inside the step
    for g, job in zip(got, rec.jobs):
        assert g is table.panels[job.key]
    assert got_merged is kept_panel


def test_step_table_without_jobs_and_with_an_optimizer_table(launches):
    c3, _ = _convs()
    assert CP.step_table([]) is None and launches.total == 0
    job = CP.PackJob(CP.request_key(c3.weight, _spec(c3), False, MODE), c3.weight, _spec(c3), False, MODE)

    class Kept:  # (the interface of OptimizerPacks that a step uses)
        def step_table(self):
            return CP.StepTable.packed([job], {"kept": 1}, {"m": 2})

    t = CP.step_table([job], Kept())
    assert set(t.panels) == {"kept", job.key} and t.merged == {"m": 2} and launches.batched == 1
    was = CP.set_optimizer_packs(False)
    try:
        t = CP.step_table([job], Kept())
    finally:
        CP.set_optimizer_packs(was)
    assert set(t.panels) == {job.key} and t.merged == {} and launches.batched == 2


def test_step_restores_the_previous_state(launches):
    c3, _ = _convs()
    with CP.recording() as rec:
        CP.pack_weights(c3.weight, _spec(c3), False, MODE)
    table, outer = CP.StepTable.packed(rec.jobs), CP.StepTable({})
    assert CP._STATE.table is None
    for _ in range(2):  # (the two graphs of one step open the same table one after the other)
        with CP.step(table) as t:
            assert t is table and CP._STATE.table is table
            assert CP.pack_weights(c3.weight, _spec(c3), False, MODE) is table.panels[rec.jobs[0].key]
        assert CP._STATE.table is None
    with CP.step(outer):
        with pytest.raises(ZeroDivisionError):
            with CP.step(table):
                1 / 0
        assert CP._STATE.table is outer
        with CP.step(None):
            assert CP._STATE.table is None
        assert CP._STATE.table is outer
    assert CP._STATE.table is None


def _expected(kind, convs):
    ws, bs = [c.weight.detach() for c in convs], [c.bias.detach() for c in convs]
    if kind == "cat":
        return torch.cat(ws), torch.cat(bs)
    W = torch.zeros(sum(w.shape[0] for w in ws), sum(w.shape[1] for w in ws), *ws[0].shape[2:])
    o = c = 0
    for w in ws:
        W[o:o + w.shape[0], c:c + w.shape[1]] = w
        o, c = o + w.shape[0], c + w.shape[1]
    return W, torch.cat(bs)


@pytest.mark.parametrize("kind", ["cat", "blockdiag"])
def test_merged_filters_fresh_recorded_and_kept(launches, kind):
    torch.manual_seed(1)
    convs = [torch.nn.Conv2d(8, 8, 3, padding=1), torch.nn.Conv2d(8, 8, 3, padding=1)]
    spec = _spec(convs[0])
    eW, eb = _expected(kind, convs)

    W, b = CP.merged_filters(kind, convs)  # outside a table: a fresh merge
    assert torch.equal(W.detach(), eW) and torch.equal(b.detach(), eb) and W.requires_grad

    with CP.recording() as rec:  # a request on the result is recorded with its sources
        W, b = CP.merged_filters(kind, convs)
        CP.pack_weights(W, spec, False, MODE)
        CP.pack_weights(W.detach(), spec, False, MODE)  # (the backward side's view of the same filter: the same job)
        CP.pack_weights(W, spec, True, MODE)
    assert rec.jobs == [] and len(rec.merged_jobs) == 2
    for job, for_dgrad in zip(rec.merged_jobs, (False, True)):
        assert job.kind == kind and job.for_dgrad == for_dgrad and job.spec is spec and job.mode == MODE
        assert all(a is c.weight for a, c in zip(job.weights, convs)) and all(a is c.bias for a, c in zip(job.biases, convs))

    table = CP.StepTable({}, {CP.merged_key(kind, [c.weight for c in convs]): (eW.clone(), eb.clone())})
    kW, kb = table.merged[CP.merged_key(kind, [c.weight for c in convs])]
    with CP.step(table):
        W, b = CP.merged_filters(kind, convs)
    assert W.data_ptr() == kW.data_ptr() and b.data_ptr() == kb.data_ptr() and W.shape == kW.shape  # the table's buffers, no copy
    (W.sum() + b.sum()).backward()
    for c in convs:  # exactly the slice / diagonal block of ones
        assert torch.equal(c.weight.grad, torch.ones_like(c.weight)) and c.weight.grad.is_contiguous()
        assert torch.equal(c.bias.grad, torch.ones_like(c.bias))
    # (the dense gradient of the block-diagonal filter also has off-diagonal ones: they reach nobody)
    assert launches.single == 3 and launches.batched == 0


def test_cat_of_frozen_weights_merges_once_per_version(launches):
    c3a, c3b = torch.nn.Conv2d(8, 8, 3), torch.nn.Conv2d(8, 8, 3)
    with torch.no_grad():
        W, b = CP.merged_filters("cat", [c3a, c3b])
        W2, _ = CP.merged_filters("cat", [c3a, c3b])
        assert W2 is W and isinstance(W, torch.nn.Parameter) and not W.requires_grad
        assert torch.equal(W, torch.cat([c3a.weight, c3b.weight])) and torch.equal(b, torch.cat([c3a.bias, c3b.bias]))
        c3b.weight.mul_(2.0)
        W3, _ = CP.merged_filters("cat", [c3a, c3b])
        assert W3 is not W and torch.equal(W3, torch.cat([c3a.weight, c3b.weight]))


def test_a_recorded_merged_filter_keeps_its_address(launches):
    """the note of a merged filter keeps the filter alive: a later temporary of the same shape cannot take its address and be taken for it"""
    _, c1 = _convs()
    spec = _spec(c1)
    with CP.recording() as rec:
        W, _ = CP.merged_filters("cat", [c1, c1])
        ptr, shape = W.data_ptr(), W.shape
        del W
        gc.collect()
        others = [torch.empty(shape) for _ in range(8)]  # (the allocator would hand the freed block to the first of these)
        assert all(t.data_ptr() != ptr for t in others)
        for t in others:
            CP.pack_weights(t, spec, False, MODE)
        assert rec.merged_jobs == []
    assert rec._built is None  # (and the note is dropped with the recording)
