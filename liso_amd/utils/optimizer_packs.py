"""What a FlatAdamW launch writes besides the parameters (include/liso_optim.h: liso_adamw_step_packed_f32): the packed filter panels
of the convolutions, and the merged fp32 filters / concatenated biases of convolutions that run as one launch.

`OptimizerPacks` is built once from the pack requests that a warm-up step recorded (conv_panels.recording: `jobs`, `merged_jobs`).
Panels and merged buffers are allocated here, outside any graph's memory pool, filled once from the master weights, and from then on
rewritten by every `optimizer.step()`.  A captured step opens `step_table()` (conv_panels.step) and contains no pack launch.  Whatever
else changes a parameter (load_state_dict, an in-place edit, an update by another path) moves its `_version` away from the one the
panels were written at: `ensure_current()`, called before every replay, then repacks everything with one launch
(liso_conv_pack_weights_placed)."""
import ctypes

import torch

from liso_amd import _lib as L
from liso_amd.utils import conv_panels as CP

_MODES = (L.CONV_BF16, L.CONV_F32X3, L.CONV_F32)


class OptimizerPacks:
    def __init__(self, opt, pack_jobs, merged_jobs=()):
        """`opt`: the FlatAdamW; `pack_jobs`: conv_panels.PackJobs as recorded; `merged_jobs`: conv_panels.MergedJobs.  Requests this
        table does not cover (a parameter outside the optimizer, a third panel of one tensor, an fp16 panel) stay in `leftover_jobs`:
        the step packs those as before."""
        lib = L.lib()
        self.device = opt.flat_param.device
        self.panels, self.merged, self.leftover_jobs = {}, {}, []
        items = {}  # id(param) -> dict(param, spec geometry, dests, mirror)
        self._placed, self._mirror_jobs, self._keep = [], [], []

        def item_of(p, kh, kw, transposed):
            ok = id(p) in opt.offsets and p.dtype == torch.float32 and p.is_contiguous()
            if not ok:
                return None
            it = items.get(id(p))
            if it is None:
                d0, d1 = (p.shape[0], p.shape[1]) if p.dim() == 4 else (1, p.numel())
                it = items[id(p)] = dict(p=p, d0=d0, d1=d1, kh=kh, kw=kw, transposed=int(transposed), dests=[], mirror=None)
            return it if (it["kh"], it["kw"], it["transposed"]) == (kh, kw, int(transposed)) else None

        def panel(K, N, taps, mode):
            t = torch.zeros(lib.liso_conv_packed_bytes(K, N, taps, mode), dtype=torch.uint8, device=self.device)
            self._keep.append(t)
            return t

        def add_dest(it, dst, for_dgrad, mode, K, N, k_off, n_off):
            it["dests"].append((dst, int(bool(for_dgrad)), mode, K, N, k_off, n_off))
            p = it["p"]
            self._placed.append(L.ConvPackPlacedJob(p.data_ptr(), dst.data_ptr(), it["d0"], it["d1"], it["kh"], it["kw"], it["transposed"],
                                                    int(bool(for_dgrad)), mode, K, N, k_off, n_off))

        # merged filters first: their sources' two panel slots go to the merged panels
        groups = {}
        for kind, ws, bs, spec, for_dgrad, mode in merged_jobs:
            gkey = CP.merged_key(kind, ws)
            its = [item_of(w, spec.kh, spec.kw, spec.transposed) for w in ws]
            bits = [item_of(b, 1, 1, False) for b in bs]
            usable = mode in _MODES and not spec.transposed and all(i is not None for i in its + bits) and \
                all(len(i["dests"]) < 2 for i in its)
            if not usable:
                continue
            co, ci = [w.shape[0] for w in ws], [w.shape[1] for w in ws]
            taps = spec.kh * spec.kw
            if gkey not in groups:
                if any(i["mirror"] is not None for i in its + bits):
                    continue
                if kind == "cat":
                    W = torch.zeros((sum(co), ci[0], spec.kh, spec.kw), dtype=torch.float32, device=self.device)
                else:
                    W = torch.zeros((sum(co), sum(ci), spec.kh, spec.kw), dtype=torch.float32, device=self.device)
                bias = torch.zeros(sum(co), dtype=torch.float32, device=self.device)
                groups[gkey] = (W, bias)
                o = c = 0
                for w, b, it, bit, a, k in zip(ws, bs, its, bits, co, ci):
                    wv = W[o:o + a] if kind == "cat" else W[o:o + a, c:c + k]
                    it["mirror"] = (wv, W.stride(0))
                    bit["mirror"] = (bias[o:o + a], a)
                    self._mirror_jobs += [(wv, w), (bias[o:o + a], b)]
                    o, c = o + a, c + k
            W, bias = groups[gkey]
            # the merged convolution's panel geometry: a plain (not transposed) convolution [sum co][K columns]
            d0, d1 = W.shape[0], W.shape[1]
            K, N = (d0, d1) if for_dgrad else (d1, d0)
            dst = panel(K, N, taps, mode)
            o = c = 0
            for it, a, k in zip(its, co, ci):
                col = c if kind == "blockdiag" else 0
                k_off, n_off = (o, col) if for_dgrad else (col, o)
                add_dest(it, dst, for_dgrad, mode, K, N, k_off, n_off)
                o, c = o + a, c + k
            self.panels[CP.request_key(W, spec, for_dgrad, mode)] = dst
        self.merged = groups

        for job in pack_jobs:
            key, w, spec, for_dgrad, mode = job
            it = item_of(w, spec.kh, spec.kw, spec.transposed) if (w.dim() == 4 and mode in _MODES) else None
            if it is None or len(it["dests"]) >= 2:
                self.leftover_jobs.append(job)
                continue
            K, N = (it["d1"], it["d0"]) if spec.transposed == bool(for_dgrad) else (it["d0"], it["d1"])
            dst = panel(K, N, spec.kh * spec.kw, mode)
            add_dest(it, dst, for_dgrad, mode, K, N, 0, 0)
            self.panels[key] = dst

        self.params = [it["p"] for it in items.values()]
        arr = (L.AdamwPackItem * max(len(items), 1))()
        for i, it in enumerate(items.values()):
            a = arr[i]
            a.offset, a.d0, a.d1, a.kh, a.kw, a.transposed = opt.offsets[id(it["p"])], it["d0"], it["d1"], it["kh"], it["kw"], it["transposed"]
            a.n_dest = len(it["dests"])
            for k, (dst, for_dgrad, mode, K, N, k_off, n_off) in enumerate(it["dests"]):
                a.dest[k] = L.AdamwPackDest(dst.data_ptr(), for_dgrad, mode, K, N, k_off, n_off)
            if it["mirror"] is not None:
                a.mirror, a.mirror_row_stride = it["mirror"][0].data_ptr(), it["mirror"][1]
        nbytes, blocks = ctypes.c_size_t(0), ctypes.c_int(0)
        L.check(lib.liso_adamw_pack_table_plan(arr, len(items), opt.numel, ctypes.byref(nbytes), ctypes.byref(blocks)), "adamw_pack_table_plan")
        image = (ctypes.c_ubyte * nbytes.value)()
        L.check(lib.liso_adamw_pack_table_fill(arr, len(items), opt.numel, image, nbytes.value), "adamw_pack_table_fill")
        self.table = torch.frombuffer(image, dtype=torch.uint8).clone().to(self.device)
        self.blocks, self.n_items = blocks.value, len(items)
        self._placed_arr = (L.ConvPackPlacedJob * max(len(self._placed), 1))(*self._placed)
        self._versions = None
        self.repacks = 0
        self.repack(clear=True)

    def step_table(self):
        """what a captured step's requests resolve to: the panels and merged buffers kept here, and the `leftover_jobs` packed now with
        one launch"""
        return CP.StepTable.packed(self.leftover_jobs, self.panels, self.merged)

    def repack(self, clear=False):
        """panels and merged buffers from the current master weights: one pack launch (+ one zero fill with `clear`) and one copy launch"""
        with torch.no_grad(), torch.cuda.device(self.device):
            if self._placed:
                L.check(L.lib().liso_conv_pack_weights_placed(self._placed_arr, len(self._placed), int(bool(clear)), L.stream_ptr()),
                        "conv_pack_weights_placed")
            if self._mirror_jobs:
                L.copy_blocks([(d, s.detach()) for d, s in self._mirror_jobs])
        self.repacks += 1
        self.stamp()

    def stamp(self):
        """the panels now hold the parameters as they are"""
        self._versions = [p._version for p in self.params]

    def current(self):
        return self._versions is not None and all(p._version == v for p, v in zip(self.params, self._versions))

    def ensure_current(self):
        if not self.current():
            self.repack()
