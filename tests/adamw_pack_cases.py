"""The synthetic parameter list of the liso_adamw_step_packed_f32 tests (include/liso_optim.h) and its table, shared by the host test of
the table checks and the device test of the launch.

Tensors, in flat-buffer order (every offset a multiple of 4 elements, as FlatAdamW lays them out):
  a 3x3 filter [24, 8, 3, 3]          K = 8 < 16 and N = 24 < 64: both paddings of a panel
  a vector of 3
  a 3x3 filter [16, 5, 3, 3]          rows of 45 floats: the scalar path
  a vector of 7
  a 1x1 filter [64, 32, 1, 1]
  a vector of 64
  a transposed 2x2 filter [16, 12, 2, 2]
  a 3x3 filter [40, 72, 3, 3]         five row tiles x three column tiles (the last one 8 columns wide), one pure padding chunk along k
  a 1x1 filter [100, 16, 1, 1]        two row tiles of whole rows (64 + 36)
  four [8, 16, 3, 3] filters + their biases [8]: concatenated along the output channels into one panel / one fp32 filter / one bias
  four [co, 8, 3, 3] filters, co = 2, 3, 1, 2, + their biases: the diagonal blocks of one [8, 32, 3, 3] filter
The vectors, and the 1-3 element gaps behind tensors whose size is no multiple of 4, are the plain ranges of the launch."""
import ctypes

import torch

SINGLE = [("w33", (24, 8, 3, 3), 0), ("v3", (3,), 0), ("w45", (16, 5, 3, 3), 0), ("v7", (7,), 0), ("w11", (64, 32, 1, 1), 0), ("v64", (64,), 0),
          ("wT", (16, 12, 2, 2), 1), ("wbig", (40, 72, 3, 3), 0), ("wrows", (100, 16, 1, 1), 0)]
CAT = [("cat%d" % i, (8, 16, 3, 3)) for i in range(4)]
DIAG_CO = [2, 3, 1, 2]
DIAG = [("diag%d" % i, (co, 8, 3, 3)) for i, co in enumerate(DIAG_CO)]


def layout():
    """-> ([(name, shape, transposed)], {name: offset}, total elements)"""
    tensors = list(SINGLE)
    for (n, s) in CAT:
        tensors += [(n, s, 0), (n + "_b", (s[0],), 0)]
    for (n, s) in DIAG:
        tensors += [(n, s, 0), (n + "_b", (s[0],), 0)]
    offs, off = {}, 0
    for n, s, _ in tensors:
        offs[n] = off
        numel = 1
        for d in s:
            numel *= d
        off += (numel + 3) // 4 * 4
    return tensors, offs, off


def panel_geometry(shape, transposed, for_dgrad):
    d0, d1 = shape[0], shape[1]
    return (d1, d0) if bool(transposed) == bool(for_dgrad) else (d0, d1)  # K, N


def build_items(L, alloc_panel, alloc_f32, mode):
    """-> (ctypes item array, n_items, panels {(name, for_dgrad): (tensor, K, N, taps)}, mirrors {name: fp32 tensor}, placed jobs list of
    (name, for_dgrad, K, N, k_off, n_off)).  `alloc_panel(nbytes)` / `alloc_f32(shape)` allocate device memory."""
    lib = L.lib()
    tensors, offs, _ = layout()
    shapes = {n: (s, t) for n, s, t in tensors}
    panels, mirrors, placed = {}, {}, []
    items = []

    def item(name, dests, mirror=None, stride=0):
        s, t = shapes[name]
        a = L.AdamwPackItem()
        a.offset = offs[name]
        if len(s) == 4:
            a.d0, a.d1, a.kh, a.kw = s
        else:
            a.d0, a.d1, a.kh, a.kw = 1, s[0], 1, 1
        a.transposed, a.n_dest = t, len(dests)
        for k, (dst, fd, K, N, ko, no) in enumerate(dests):
            a.dest[k] = L.AdamwPackDest(dst.data_ptr(), fd, mode, K, N, ko, no)
            placed.append((name, fd, dst, K, N, ko, no))
        if mirror is not None:
            a.mirror, a.mirror_row_stride = mirror.data_ptr(), stride
        items.append(a)

    for n, s, t in SINGLE:
        if len(s) != 4:
            continue
        dests = []
        for fd in (0, 1):
            K, N = panel_geometry(s, t, fd)
            dst = alloc_panel(lib.liso_conv_packed_bytes(K, N, s[2] * s[3], mode))
            panels[(n, fd)] = (dst, K, N, s[2] * s[3])
            dests.append((dst, fd, K, N, 0, 0))
        item(n, dests)
    # concatenated along the output channels: merged [32, 16, 3, 3]
    mirrors["cat"], mirrors["cat_b"] = alloc_f32((32, 16, 3, 3)), alloc_f32((32,))
    cat_p = {}
    for fd in (0, 1):
        K, N = panel_geometry((32, 16), 0, fd)
        cat_p[fd] = alloc_panel(lib.liso_conv_packed_bytes(K, N, 9, mode))
        panels[("cat", fd)] = (cat_p[fd], K, N, 9)
    for i, (n, s) in enumerate(CAT):
        dests = [(cat_p[0], 0, 16, 32, 0, 8 * i), (cat_p[1], 1, 32, 16, 8 * i, 0)]
        item(n, dests, mirrors["cat"][8 * i:8 * i + 8], 16 * 9)
        item(n + "_b", [], mirrors["cat_b"][8 * i:8 * i + 8], 8)
    # diagonal blocks: merged [8, 32, 3, 3]
    mirrors["diag"], mirrors["diag_b"] = alloc_f32((8, 32, 3, 3)), alloc_f32((8,))
    diag_p = {}
    for fd in (0, 1):
        K, N = panel_geometry((8, 32), 0, fd)
        diag_p[fd] = alloc_panel(lib.liso_conv_packed_bytes(K, N, 9, mode))
        panels[("diag", fd)] = (diag_p[fd], K, N, 9)
    o = 0
    for i, (n, s) in enumerate(DIAG):
        co = s[0]
        dests = [(diag_p[0], 0, 32, 8, 8 * i, o), (diag_p[1], 1, 8, 32, o, 8 * i)]
        item(n, dests, mirrors["diag"][o:o + co, 8 * i:8 * i + 8], 32 * 9)
        item(n + "_b", [], mirrors["diag_b"][o:o + co], co)
        o += co
    arr = (L.AdamwPackItem * len(items))(*items)
    return arr, len(items), panels, mirrors, placed


def plan(L, arr, n_items, n):
    """-> (code, bytes, blocks)"""
    nbytes, blocks = ctypes.c_size_t(0), ctypes.c_int(0)
    rc = L.lib().liso_adamw_pack_table_plan(arr, n_items, n, ctypes.byref(nbytes), ctypes.byref(blocks))
    return rc, nbytes.value, blocks.value


def table_image(L, arr, n_items, n):
    rc, nbytes, blocks = plan(L, arr, n_items, n)
    assert rc == 0, rc
    image = (ctypes.c_ubyte * nbytes)()
    assert L.lib().liso_adamw_pack_table_fill(arr, n_items, n, image, nbytes) == 0
    return torch.frombuffer(image, dtype=torch.uint8).clone(), blocks
