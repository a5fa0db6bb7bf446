"""Host-side helpers of the trainers: tensor trees, loss-cloud padding, byte packing (liso_amd/utils/tensor_tree.py) and the LRU of
resident graphs (liso_amd/utils/graph_capture.py).  CPU tensors only."""
import torch

from liso_amd.utils import tensor_tree as TT
from liso_amd.utils.graph_capture import GraphLRU


def _sample(b=1, n=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {"pcl_ta": {"pcl": torch.randn(b, n, 4, generator=g), "pcl_is_valid": torch.rand(b, n, generator=g) > 0.3,
                       "pillar_coors": torch.randint(0, 9, (b, n, 2), generator=g, dtype=torch.int32)},
            "gt": {"odom_ta_tb": torch.randn(b, 4, 4, generator=g, dtype=torch.float64)},
            "clouds": [torch.randn(n + i, 4, generator=g) for i in range(b)],
            "pair": (torch.zeros(b, 2), torch.tensor(3.0)), "name": "sweep", "count": 7}


def test_tree_map_keeps_structure_and_non_tensors():
    s = _sample()
    out = TT.tree_map(s, lambda t: t.double() + 1)
    assert out["name"] == "sweep" and out["count"] == 7
    assert isinstance(out["clouds"], list) and isinstance(out["pair"], tuple)
    assert out["pcl_ta"]["pcl"].dtype == torch.float64
    assert torch.equal(out["gt"]["odom_ta_tb"], s["gt"]["odom_ta_tb"] + 1)
    assert torch.equal(out["pair"][1], torch.tensor(4.0, dtype=torch.float64))
    assert s["pcl_ta"]["pcl"].dtype == torch.float32  # (the input tree is untouched)


def test_tree_signature_follows_the_map_order_and_can_skip_an_axis():
    s = _sample(b=2, n=5)
    seen = []
    TT.tree_map(s, lambda t: seen.append((tuple(t.shape), t.dtype)) or t)  # (how the signature used to be collected)
    assert TT.tree_signature(s) == tuple(seen) and len(seen) == 8
    assert TT.tree_signature((s, [s])) == tuple(seen) * 2
    a, b = _sample(n=5)["pcl_ta"], _sample(n=9)["pcl_ta"]
    assert TT.tree_signature(a) != TT.tree_signature(b)
    assert TT.tree_signature(a, skip_dim=1) == TT.tree_signature(b, skip_dim=1) == (((1, 4), torch.float32), ((1,), torch.bool), ((1, 2), torch.int32))
    assert TT.tree_signature({"x": 1, "y": "z"}) == ()


def test_tree_copy_writes_every_tensor_of_dst_from_src(monkeypatch):
    from liso_amd import _lib as L

    calls = []

    def multi_copy(pairs):  # (the device launch, here on the host)
        calls.append(len(pairs))
        for d, s_ in pairs:
            d.copy_(s_)

    monkeypatch.setattr(L, "multi_copy", multi_copy)
    src = _sample(seed=1)
    dst = TT.tree_map({k: src[k] for k in ("pcl_ta", "gt", "pair")}, torch.zeros_like)  # (src may hold more than dst)
    TT.tree_copy_(dst, src)
    assert calls == [6]
    for (d, s_) in TT.tree_pairs(dst, src):
        assert d is not s_ and torch.equal(d, s_)
    TT.tree_copy_({}, src)
    assert calls == [6]  # (nothing to copy: no launch)


def test_tree_stack_concatenates_tensors_and_chains_lists():
    a, b = _sample(seed=2), _sample(seed=3)
    out = TT.tree_stack([a, b])
    assert torch.equal(out["pcl_ta"]["pcl"], torch.cat([a["pcl_ta"]["pcl"], b["pcl_ta"]["pcl"]], dim=0))
    assert out["gt"]["odom_ta_tb"].shape == (2, 4, 4)
    assert isinstance(out["clouds"], list) and len(out["clouds"]) == 2 and out["clouds"][1] is b["clouds"][0]
    assert isinstance(out["pair"], tuple) and len(out["pair"]) == 4  # (tuples chain like lists)
    assert out["name"] == "sweep" and out["count"] == 7
    assert TT.tree_stack([torch.tensor(1.0), torch.tensor(2.0)]).item() == 1.0  # (0-dim: the first sample's)


def _same(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and x.contiguous().view(torch.uint8).equal(y.contiguous().view(torch.uint8))


def test_pad_pcl_ta_is_the_padding_both_call_sites_wrote_out():
    F = torch.nn.functional
    pa = dict(_sample(b=2, n=5)["pcl_ta"], extra="kept")
    for n in (5, 8, 16):
        pad = n - 5
        out = TT.pad_pcl_ta(pa, n)
        if pad == 0:
            assert out is pa
            continue
        # the expressions of LisoLoopTrainer._pad_loss_cloud and ._grow_view before they shared this function
        want = {**pa, "pcl": F.pad(pa["pcl"], (0, 0, 0, pad), value=float("nan")),
                "pcl_is_valid": F.pad(pa["pcl_is_valid"], (0, pad), value=False),
                "pillar_coors": F.pad(pa["pillar_coors"], (0, 0, 0, pad), value=-1)}
        assert out is not pa and set(out) == set(want) and out["extra"] == "kept"
        for k in ("pcl", "pcl_is_valid", "pillar_coors"):
            assert _same(out[k], want[k]), k
        assert out["pcl"][:, 5:].isnan().all() and not out["pcl_is_valid"][:, 5:].any() and (out["pillar_coors"][:, 5:] == -1).all()
    assert pa["pcl"].shape[1] == 5  # (the input is not modified)


def _mixed():
    g = torch.Generator().manual_seed(5)
    return [("f32", torch.randn(2, 3, generator=g)), ("flag", torch.rand(7, generator=g) > 0.5),  # (7 bytes: an odd count)
            ("i64", torch.randint(-9, 9, (1,), generator=g)), ("f64", torch.randn(4, 4, generator=g, dtype=torch.float64)),
            ("u8", torch.arange(3, dtype=torch.uint8)), ("bf16", torch.randn(5, generator=g).bfloat16()),
            ("strided", torch.randn(4, 6, generator=g)[:, ::2]), ("empty", torch.zeros(0, 3))]


def test_pack_unpack_round_trip_over_mixed_dtypes():
    named = _mixed()
    flat, layout = TT.pack(named)
    assert flat.dtype == torch.uint8 and flat.numel() == sum(t.numel() * t.element_size() for _, t in named)
    out = TT.unpack(flat, layout)
    assert set(out) == {k for k, _ in named}
    for k, t in named:
        assert _same(out[k], t), k
    for name, off, nbytes, dtype, _ in layout:  # every segment is aligned for its dtype
        assert off % torch.empty(0, dtype=dtype).element_size() == 0, name
    assert [torch.empty(0, dtype=d).element_size() for _, _, _, d, _ in layout] == sorted(
        (t.element_size() for _, t in named), reverse=True)


def test_packed_statics_are_views_of_one_buffer_refreshed_by_pack_into():
    tensors = {"flag": torch.rand(7) > 0.5, "cloud": torch.randn(1, 8, 4), "odom": torch.randn(1, 4, 4, dtype=torch.float64),
               "valid": torch.rand(1, 16) > 0.5}
    views, flat, layout = TT.packed_statics(tensors)
    assert flat.numel() == 7 + 128 + 128 + 16 and [name for name, *_ in layout] == ["cloud", "odom", "valid", "flag"]
    assert all(off % 16 == 0 for _, off, *_ in layout)  # (the one segment of an odd size goes last)
    for k, t in tensors.items():
        assert _same(views[k], t) and views[k].data_ptr() != t.data_ptr()
    fresh = {k: (torch.randn_like(t) if t.is_floating_point() else ~t) for k, t in tensors.items()}
    TT.pack_into(flat, layout, fresh)
    for k, t in fresh.items():
        assert _same(views[k], t), k
    # two segments of odd sizes, or a strided tensor: separate copies, no flat buffer
    for bad in ({**tensors, "flag2": torch.rand(3) > 0.5}, {**tensors, "cloud": torch.randn(1, 8, 8)[..., ::2]}):
        copies, flat, layout = TT.packed_statics(bad)
        assert flat is None and layout is None and all(_same(copies[k], t) and copies[k] is not t for k, t in bad.items())


def test_graph_lru_evicts_the_least_recently_used_and_clears_it():
    syncs = []
    lru = GraphLRU(synchronize=lambda: syncs.append(len(lru)))
    entries = {k: {"graph": k} for k in "abcde"}
    for k in "abc":
        assert lru.insert(k, entries[k], 3) is entries[k]
    assert list(lru) == ["a", "b", "c"] and syncs == [] and len(lru) == 3
    assert lru.lookup("a") is entries["a"] and list(lru) == ["b", "c", "a"]  # (a hit makes it the most recent)
    assert lru.lookup("zzz") is None and list(lru) == ["b", "c", "a"]
    lru.insert("d", entries["d"], 3)
    assert list(lru) == ["c", "a", "d"] and entries["b"] == {} and syncs == [3]
    lru.insert("e", entries["e"], 2)  # a smaller capacity: ONE synchronisation before the first eviction, then as many as needed
    assert list(lru) == ["d", "e"] and entries["c"] == {} and entries["a"] == {} and syncs == [3, 3]
    assert [v["graph"] for v in lru.values()] == ["d", "e"]
    lru.insert("f", {"graph": "f"}, 0)  # (a capacity below 1 counts as 1)
    assert list(lru) == ["f"] and len(lru.values()) == 1
    for i in range(20):
        lru.insert(i, {}, 4)
        assert len(lru) <= 4
