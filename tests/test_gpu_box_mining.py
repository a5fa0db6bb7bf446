"""Every entry point of include/liso_box_mining.h (liso_amd/csrc/box_mining.hip) on its own against the host restatements of
oracle/flow_cluster.py, at the sizes and values where each kernel takes another path: the second chunk of the block-sum scan,
non-square grids and centroids outside them, boxes exactly on every filter threshold and one fp64 step to either side, survivors
across the 64-lane rounds, per-sample background transforms, ties / NaN / fp64-close confidences, hand-made NMS survivor lists.
Comparisons are bit for bit (outputs are pre-filled with a byte pattern and compared in full) except box motion, which is
measured against the same algebra in numpy.longdouble.  Every device buffer lies between guard bands (tests/guarded_alloc.py)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests.guarded_alloc import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
PATTERN = 0xA5
EINVAL, EWORKSPACE = -1, -2
BOX_KEYS = ("pos", "dims", "rot", "probs", "velo", "valid", "class_id", "difficulty")


def _L():
    from liso_amd import _lib as L

    return L


def dev(a):
    """numpy -> device, allocated by torch.empty (so: between guard bands inside guarded())"""
    src = torch.from_numpy(np.ascontiguousarray(a))
    t = torch.empty(tuple(src.shape), dtype=src.dtype, device=DEV)
    t.copy_(src)
    return t


def poisoned(shape, dtype):
    t = torch.empty(tuple(shape), dtype=dtype, device=DEV)
    t.view(-1).view(torch.uint8).fill_(PATTERN)
    return t


def pattern_like(shape, dtype):
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, PATTERN, np.uint8).view(dtype).reshape(shape)


def assert_bits(what, got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        u = {1: np.uint8, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        bad = np.flatnonzero(got.reshape(-1).view(u) != want.reshape(-1).view(u))
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} elements differ, first at flat index {i} "
                             f"(shape {got.shape}): got {got.reshape(-1)[i]!r}, want {want.reshape(-1)[i]!r}")


# ---- scan ---------------------------------------------------------------------------------------------------------------------
# 2048 elements per block, block sums scanned in chunks of 256: 524 288 = one full chunk, 524 289 = the first carry,
# 846 400 = the 920 x 920 grid of the reference's training resolution (414 blocks)
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n", [1, 7, 2047, 2048, 2049, 524288, 524289, 846400])
def test_scan_equals_cumsum(n, batch):
    L = _L()
    lib = L.lib()
    rng = np.random.default_rng(4 * n + batch)
    inputs = {"flags, 1 % set": rng.random((batch, n)) < 0.01, "signed in [-3, 3]": rng.integers(-3, 4, (batch, n)),
              "all ones": np.ones((batch, n))}
    nbytes = lib.liso_scan_workspace_bytes(batch, n)
    assert nbytes == 4 * batch * ((n + 2047) // 2048)
    with guarded() as gd:
        for what, x in inputs.items():
            x = x.astype(np.int32)
            xd, out, ws = dev(x), poisoned((batch, n), torch.int32), poisoned((nbytes,), torch.uint8)  # the workspace: exactly nbytes
            assert lib.liso_scan_inclusive_i32(L.ptr(xd), batch, n, L.ptr(out), L.ptr(ws), nbytes, L.stream_ptr()) == 0
            assert_bits(what, out, np.cumsum(x.astype(np.int64), axis=1).astype(np.int32))
            assert_bits(what + " (input)", xd, x)
        gd.check()


def test_scan_refuses_a_short_workspace_and_empty_rows():
    L = _L()
    lib = L.lib()
    batch, n = 2, 5000
    nbytes = lib.liso_scan_workspace_bytes(batch, n)
    with guarded() as gd:
        xd, out, ws = dev(np.ones((batch, n), np.int32)), poisoned((batch, n), torch.int32), poisoned((nbytes,), torch.uint8)
        assert lib.liso_scan_inclusive_i32(L.ptr(xd), batch, n, L.ptr(out), L.ptr(ws), nbytes - 1, L.stream_ptr()) == EWORKSPACE
        assert lib.liso_scan_inclusive_i32(L.ptr(xd), batch, 0, L.ptr(out), L.ptr(ws), nbytes, L.stream_ptr()) == EINVAL
        assert lib.liso_scan_workspace_bytes(batch, 0) == 0
        gd.check()
        assert_bits("out", out, pattern_like((batch, n), np.int32))  # nothing was launched


# ---- boxes from regions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gx,gy", [(96, 64), (64, 96)])
def test_boxes_from_regions_bit_for_bit_on_non_square_grids(gx, gy):
    from liso_amd.networks.flow_cluster_detector import mining_ops as MO
    from oracle import flow_cluster as OF

    rng = np.random.default_rng(gx)
    ppm = np.array([5.12, 3.3], np.float32)  # neither is an fp64 value: the ABI's float -> double widening shows in the quotient
    rows = ((np.arange(gx) - gx / 2 + 0.5) / 5.12).astype(np.float32)
    cols = ((np.arange(gy) - gy / 2 + 0.5) / 3.3 + 100.0).astype(np.float32)
    hi = min(gx, gy) - 1
    # 80 is a valid index of the longer axis but above min(gx, gy) - 1: the reference clips BOTH indices by the smaller extent
    edge = [-0.5, 0.999, float(hi), hi + 0.5, 80.0, 1e9, -3.7, 17.5, hi - 0.001]
    cross = np.array([(r, c) for r in edge for c in edge])
    B, K = 2, 100  # 200 boxes: two blocks of 128 threads, the second one partial
    props = np.zeros((B, K, 5))
    props[..., 0:2] = rng.uniform(-5.0, 100.0, (B, K, 2))
    props[0, :len(cross), 0:2], props[1, :len(cross), 0:2] = cross, cross[::-1]
    props[..., 2] = rng.uniform(-math.pi / 2, math.pi / 2, (B, K))
    props[..., 3] = rng.uniform(0.0, 40.0, (B, K))
    props[..., 4] = props[..., 3] * rng.uniform(0.0, 1.0, (B, K))
    props[:, 90] = 0.0                # an absent label
    props[0, 91, 3:5] = [7.3, 0.0]    # a one-pillar-wide region
    with guarded() as gd:
        got = MO.boxes_from_regions(dev(props), dev(rows), dev(cols), ppm)
        gd.check()
    want = OF.boxes_from_regions(props, rows, cols, ppm)
    for what, g, w in zip(("center", "dims", "rot", "dims_f32", "rot_f32"), got, want):
        assert_bits(what, g, w)


# ---- filters + compaction -------------------------------------------------------------------------------------------------------
def _step_until_it_moves(f, x, up):
    """the value nearest to x on the chosen side at which the fp64 quantity f leaves f(x)"""
    f0, to = f(x), (np.inf if up else -np.inf)
    x = np.nextafter(x, to)
    while f(x) == f0:
        x = np.nextafter(x, to)
    return x


def _filter_probes():
    """-> (probes, main thresholds, clamp thresholds).  A probe = (d0, d1, h fp32, points, passes under main, passes under clamp).
    Each threshold IS the fp64 quantity the host computes from its probe box, so the box sits exactly on it; its neighbours are one
    representable step of the computed quantity to either side.  A probe for one rule passes every other rule with room."""
    f32 = np.float32
    asp, length, foot, vol = (4.1, 1.03, f32(1.5)), (6.9, 2.5, f32(1.5)), (0.7, 0.5, f32(2.0)), (1.01, 0.52, f32(1.3))
    main = dict(min_points=10, aspect_ratio_max=asp[0] / asp[1], max_box_len_m=length[0], min_box_area_m2=foot[0] * foot[1],
                min_box_volume_m3=(vol[0] * vol[1]) * float(vol[2]))
    clamp_d0 = 0.003
    clamp = dict(min_points=10, aspect_ratio_max=clamp_d0 / 0.001, max_box_len_m=7.0, min_box_area_m2=-1.0, min_box_volume_m3=-1.0)
    P = []
    add = lambda d0, d1, h, n, m, c: P.append((float(d0), float(d1), f32(h), int(n), bool(m), bool(c)))
    # aspect <= : on the threshold passes, one step above fails (d0 up or d1 down), one step below passes
    add(*asp, 50, True, False)
    add(_step_until_it_moves(lambda x: x / asp[1], asp[0], True), asp[1], asp[2], 50, False, False)
    add(_step_until_it_moves(lambda x: x / asp[1], asp[0], False), asp[1], asp[2], 50, True, False)
    add(asp[0], _step_until_it_moves(lambda x: asp[0] / x, asp[1], False), asp[2], 50, False, False)
    add(asp[0], _step_until_it_moves(lambda x: asp[0] / x, asp[1], True), asp[2], 50, True, False)
    # length <=
    add(*length, 50, True, True)
    add(np.nextafter(length[0], np.inf), length[1], length[2], 50, False, True)
    add(np.nextafter(length[0], -np.inf), length[1], length[2], 50, True, True)
    # footprint > : on the threshold FAILS, one step above passes, one below fails
    add(*foot, 50, False, True)
    add(_step_until_it_moves(lambda x: x * foot[1], foot[0], True), foot[1], foot[2], 50, True, True)
    add(_step_until_it_moves(lambda x: x * foot[1], foot[0], False), foot[1], foot[2], 50, False, True)
    # volume > : the same, stepping the fp64 length and the fp32 height
    add(*vol, 50, False, True)
    add(_step_until_it_moves(lambda x: (x * vol[1]) * float(vol[2]), vol[0], True), vol[1], vol[2], 50, True, True)
    add(_step_until_it_moves(lambda x: (x * vol[1]) * float(vol[2]), vol[0], False), vol[1], vol[2], 50, False, True)
    add(vol[0], vol[1], np.nextafter(vol[2], f32(np.inf)), 50, True, True)
    add(vol[0], vol[1], np.nextafter(vol[2], f32(-np.inf)), 50, False, True)
    # points >=
    for n, ok in ((9, False), (10, True), (11, True)):
        add(3.0, 1.5, 1.5, n, ok, ok)
    # the max(d1, 0.001) clamp: under the main thresholds these fail the footprint rule whatever the aspect; under the clamp
    # thresholds (no footprint / volume rule, aspect limit = 0.003 / 0.001) the clamp alone decides
    add(clamp_d0, 0.0, 1.5, 50, False, True)
    add(clamp_d0, 5e-4, 1.5, 50, False, True)
    add(_step_until_it_moves(lambda x: x / 0.001, clamp_d0, True), 0.0, 1.5, 50, False, False)
    add(clamp_d0, np.nextafter(0.001, np.inf), 1.5, 50, False, True)
    add(2.0, 0.0, 1.5, 50, False, False)
    # plainly inside and outside
    add(3.0, 1.5, 1.5, 50, True, True)
    add(9.0, 4.0, 1.5, 50, False, False)
    add(2.0, 1.9, 1.0, 500, True, True)
    return P, main, clamp


FILTER_OUT = {"pos": (3, torch.float32), "dims": (3, torch.float64), "rot": (1, torch.float64), "probs": (1, torch.float64),
              "velo": (1, torch.float64), "valid": (None, torch.uint8), "class_id": (1, torch.int32), "difficulty": (1, torch.int32),
              "kabsch_pos": (3, torch.float32), "kabsch_dims": (3, torch.float32), "kabsch_rot": (None, torch.float32)}


@pytest.mark.parametrize("park", [0, 1])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 130])
def test_filter_compact_on_and_next_to_every_threshold(K, park):
    from oracle import flow_cluster as OF

    L = _L()
    probes, main, clamp = _filter_probes()
    B = 3
    num_labels = np.array([0, 40, K + 10], np.int64)
    rng = np.random.default_rng(K)
    # probes dealt round-robin from a different start per sample: passing and failing boxes alternate, so the survivors of a
    # sample come from every 64-lane round and land across the round boundaries
    which = (np.arange(K)[None, :] + np.array([0, 3, 7])[:, None]) % len(probes)
    pick = lambda j: np.array([[probes[i][j] for i in row] for row in which])
    dims2 = np.stack([pick(0), pick(1)], -1).astype(np.float64)
    fit_h, num_pts = pick(2).astype(np.float32), pick(3).astype(np.int64)
    center = rng.uniform(-50, 50, (B, K, 2)).astype(np.float32)
    rot = rng.uniform(-math.pi / 2, math.pi / 2, (B, K))
    fit_z = rng.uniform(-2, 2, (B, K)).astype(np.float32)
    with guarded() as gd:
        ins = [dev(a) for a in (num_labels, center, dims2, rot, num_pts, fit_z, fit_h)]
        for cfg_name, cfg, col in (("main", main, 4), ("clamp", clamp, 5)):
            want = OF.mine_filter_compact(num_labels, center, dims2, rot, num_pts, fit_z, fit_h, park_invalid=bool(park), **cfg)
            # the hand-stated verdict of every probe, independent of the restatement's comparisons
            exists = np.arange(K)[None, :] < num_labels[:, None]
            stated = pick(col).astype(bool) & exists
            assert want["counts"].tolist() == stated.sum(1).tolist(), cfg_name
            for b in range(B):
                assert_bits("survivor order", want["dims"][b, :stated[b].sum(), :2], dims2[b][stated[b]])
            out = {k: poisoned((B, K) + ((c,) if c else ()), dt) for k, (c, dt) in FILTER_OUT.items()}
            out["counts"] = poisoned((B,), torch.int32)
            c = L.MineFilterCfg(B, K, cfg["min_points"], cfg["aspect_ratio_max"], cfg["max_box_len_m"], cfg["min_box_area_m2"],
                                cfg["min_box_volume_m3"], park)
            order = ("pos", "dims", "rot", "probs", "velo", "valid", "class_id", "difficulty", "counts", "kabsch_pos", "kabsch_dims",
                     "kabsch_rot")
            rc = L.lib().liso_mine_filter_compact(ctypes.byref(c), *[L.ptr(t) for t in ins], *[L.ptr(out[k]) for k in order], L.stream_ptr())
            assert rc == 0
            for k in order:
                assert_bits(f"{cfg_name} thresholds: {k}", out[k], want[k])
        gd.check()


# ---- box motion -----------------------------------------------------------------------------------------------------------------
MOTION_S = [1, 63, 65, 130]
MOTION_B = 2


def _rigid(rng, n, yaw_max, tilt_max, t_max):
    yaw, pitch, roll = rng.uniform(-yaw_max, yaw_max, n), rng.uniform(-tilt_max, tilt_max, n), rng.uniform(-tilt_max, tilt_max, n)
    T = np.zeros((n, 4, 4))
    for i in range(n):
        cz, sz, cy, sy, cx, sx = math.cos(yaw[i]), math.sin(yaw[i]), math.cos(pitch[i]), math.sin(pitch[i]), math.cos(roll[i]), math.sin(roll[i])
        T[i, :3, :3] = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
                        @ np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    T[:, :3, 3] = rng.uniform(-t_max, t_max, (n, 3))
    T[:, 3, 3] = 1.0
    return T


def _motion_inputs(S):
    """rigid transforms (yaw, roll / pitch <= 0.05 rad, translations <= 3 m), another background per sample, positions to +/- 60 m,
    headings over (-pi, pi]; for S > 1 four boxes of sample 1 move with the background (stationary)"""
    rng = np.random.default_rng(100 + S)
    B = MOTION_B
    trafos = np.zeros((B, S + 1, 4, 4))
    fg = _rigid(rng, B * S, math.pi, 0.05, 3.0).reshape(B, S, 4, 4)
    if S > 1:  # every other box turns little, as in use
        fg[:, 1::2] = _rigid(rng, B * (S // 2), 0.05, 0.05, 3.0).reshape(B, S // 2, 4, 4)
    trafos[:, :S], trafos[:, S] = fg, _rigid(rng, B, 0.3, 0.05, 3.0)
    pos = np.concatenate([rng.uniform(-60, 60, (B, S, 2)), rng.uniform(-2, 2, (B, S, 1))], -1).astype(np.float32)
    pos[0, 0, :2], pos[1, 0, :2] = [60.0, -60.0], [-60.0, 60.0]
    rot = -rng.uniform(-math.pi, math.pi, (B, S, 1))  # (-pi, pi]
    rot[0, 0, 0] = math.pi
    rot[1, 0, 0] = np.nextafter(-math.pi, 0.0)
    stationary = np.zeros((B, S), bool)
    if S > 1:
        stationary[1, [0, 31, S - 2, S - 1]] = True
        trafos[1, :S][stationary[1]] = trafos[1, S]
    return trafos, pos, rot, stationary


def _inv_affine_ld(M):
    """inverse of affine 4x4 matrices [..., 4, 4] in longdouble: adjugate of the 3x3 part / determinant, then -A^-1 t"""
    a, t = M[..., :3, :3], M[..., :3, 3]
    adj = np.empty_like(a)
    for i in range(3):
        for j in range(3):
            r, c = [k for k in range(3) if k != j], [k for k in range(3) if k != i]  # adj[i][j] = cofactor[j][i]
            adj[..., i, j] = (-1) ** (i + j) * (a[..., r[0], c[0]] * a[..., r[1], c[1]] - a[..., r[0], c[1]] * a[..., r[1], c[0]])
    det = a[..., 0, 0] * adj[..., 0, 0] + a[..., 0, 1] * adj[..., 1, 0] + a[..., 0, 2] * adj[..., 2, 0]
    out = np.zeros_like(M)
    out[..., :3, :3] = adj / det[..., None, None]
    out[..., :3, 3] = -np.einsum("...ij,...j->...i", out[..., :3, :3], t)
    out[..., 3, 3] = 1
    return out


def _motion_reference_ld(trafos, pos, rot):
    """-> (translation [B,S,3], heading [B,S], speed [B,S]) of inv(T_box) inv(T_bg) (T_fg T_box) in numpy.longdouble"""
    ld = np.longdouble
    T, p, th = trafos.astype(ld), pos.astype(ld), rot[..., 0].astype(ld)
    B, S = th.shape
    Tb = np.zeros((B, S, 4, 4), ld)
    Tb[..., 0, 0], Tb[..., 0, 1], Tb[..., 1, 0], Tb[..., 1, 1] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th)
    Tb[..., :3, 3] = p
    Tb[..., 2, 2] = Tb[..., 3, 3] = 1
    M = np.matmul(np.matmul(_inv_affine_ld(Tb), _inv_affine_ld(T[:, S:])), np.matmul(T[:, :S], Tb))
    t = M[..., :3, 3]
    return t, th + np.arctan2(t[..., 1], t[..., 0]), np.sqrt((t * t).sum(-1))


def _motion_errors(rot, velo, ref, moving):
    """-> max over the moving boxes of (speed error [m], in-plane translation error across the heading [m], heading error [rad]).
    The kernel returns the translation only as its length and its direction: the heading error times the in-plane length is the
    translation error at right angles to the motion, the speed error the one along it."""
    t, heading, speed = ref
    dth = np.asarray(rot, np.float64)[..., 0].astype(np.longdouble) - heading
    dth = np.abs(dth - 2 * np.pi * np.round(dth / (2 * np.pi)))  # modulo 2 pi
    e_speed = np.abs(np.asarray(velo, np.float64)[..., 0].astype(np.longdouble) - speed)
    e_cross = dth * np.sqrt(t[..., 0] ** 2 + t[..., 1] ** 2)
    return float(e_speed[moving].max()), float(e_cross[moving].max()), float(dth[moving].max())


@pytest.fixture(scope="module")
def motion_cases():
    """inputs, longdouble reference and the yardstick, computed once: the largest error of the fp64 LU restatement
    (oracle.flow_cluster.box_motion: torch.linalg.inv) over the inputs of all four slot counts"""
    from oracle import flow_cluster as OF

    cases, lu = {}, []
    for S in MOTION_S:
        trafos, pos, rot, stationary = _motion_inputs(S)
        ref = _motion_reference_ld(trafos, pos, rot)
        in_plane = np.sqrt(ref[0][..., 0] ** 2 + ref[0][..., 1] ** 2)
        assert float(in_plane[~stationary].min()) > 1e-3, "a moving box whose heading could not be compared"
        lu_rot, lu_velo = OF.box_motion(trafos, pos, rot)
        lu.append(_motion_errors(lu_rot.numpy(), lu_velo.numpy(), ref, ~stationary))
        cases[S] = (trafos, pos, rot, stationary, ref)
    return cases, tuple(np.array(lu).max(0))


@pytest.mark.parametrize("S", MOTION_S)
def test_box_motion_within_four_times_the_lu_restatements_error(S, motion_cases):
    """Reference: the algebra of liso_mine_box_motion in numpy.longdouble.  Yardstick: the error of the fp64 LU restatement against
    it on the same inputs (all four slot counts).  The kernel (cofactor inverses, contracted FMAs) may be at most 4 times as far off,
    in speed and in the translation across the heading; a wrong term is orders of magnitude beyond that (the background transform of
    the wrong sample: metres).
    Measured on an MI355X, maxima over the moving boxes of all four slot counts: LU restatement 7.57e-14 m in speed and 6.30e-14 m
    across the heading (3.6e-14 rad); kernel 4.52e-14 m and 6.01e-14 m (3.6e-14 rad)."""
    from liso_amd.networks.flow_cluster_detector import mining_ops as MO

    cases, (lu_speed, lu_cross, lu_heading) = motion_cases
    trafos, pos, rot, stationary, ref = cases[S]
    with guarded() as gd:
        rot_d, velo_d = dev(rot), dev(np.full((MOTION_B, S, 1), np.nan))
        MO.box_motion(dev(trafos), dev(pos), rot_d, velo_d)
        gd.check()
    got_rot, got_velo = rot_d.cpu().numpy(), velo_d.cpu().numpy()
    k_speed, k_cross, k_heading = _motion_errors(got_rot, got_velo, ref, ~stationary)
    print(f"box motion S={S}: kernel speed {k_speed:.3e} m, across {k_cross:.3e} m, heading {k_heading:.3e} rad | LU restatement "
          f"speed {lu_speed:.3e} m, across {lu_cross:.3e} m, heading {lu_heading:.3e} rad")
    assert np.isfinite(got_rot).all() and np.isfinite(got_velo).all()
    assert k_speed <= 4 * lu_speed, (k_speed, lu_speed)
    assert k_cross <= 4 * lu_cross, (k_cross, lu_cross)
    if stationary.any():
        assert int(stationary.sum()) == 4 and float(got_velo[stationary].max()) <= 1e-9


# ---- NMS prepare ----------------------------------------------------------------------------------------------------------------
def _random_boxes(rng, B, K):
    return {"pos": rng.uniform(-50, 50, (B, K, 3)).astype(np.float32),
            "dims": rng.choice([1e-4, 0.0, 1e-3, 0.7, 2.5, 4.2], (B, K, 3)).astype(np.float64),
            "rot": rng.uniform(-math.pi, math.pi, (B, K, 1)), "probs": rng.uniform(0.05, 1.0, (B, K, 1)),
            "velo": rng.uniform(0, 9, (B, K, 1)), "valid": (rng.random((B, K)) < 0.75).astype(np.uint8),
            "class_id": rng.integers(0, 5, (B, K, 1)).astype(np.int32), "difficulty": rng.integers(0, 3, (B, K, 1)).astype(np.int32)}


def _confidences(kind, rng, B, K):
    """-> (probs [B,K,1], valid [B,K]); sample 0 of `ones` is what the mined boxes look like (all valid, all 1.0)"""
    valid = (rng.random((B, K)) < 0.75).astype(np.uint8)
    if kind == "ones":
        probs = np.ones((B, K))
        valid[0] = 1
    elif kind == "ties":  # blocks of five equal confidences, NaN on a tenth of the slots (valid ones among them)
        probs = np.repeat(rng.choice([0.25, 0.5, 0.5, 0.9, 1.0], (B, (K + 4) // 5)), 5, axis=1)[:, :K]
        probs = np.where(rng.random((B, K)) < 0.1, np.nan, probs)
        if K > 1:
            probs[:, 1], valid[:, 1] = np.nan, 1
    else:  # "close": pairs 1e-12 apart (equal as fp32), the larger one first in half of the pairs and second in the other half
        base = 0.3 + 0.01 * rng.integers(0, 6, (B, K))
        probs = base + 1e-12 * rng.integers(0, 3, (B, K))
        if K > 1:
            probs[:, 0], probs[:, 1], valid[:, 0:2] = 0.5, 0.5 + 1e-12, 1  # the later slot is the more confident one
    return probs[..., None].astype(np.float64), valid


@pytest.mark.parametrize("kind", ["ones", "ties", "close"])
@pytest.mark.parametrize("K", [1, 64, 65, 200])
def test_nms_prepare_equals_a_stable_sort(K, kind):
    from oracle import flow_cluster as OF

    L = _L()
    lib = L.lib()
    B = 2
    rng = np.random.default_rng(1000 + K)
    boxes = _random_boxes(rng, B, K)
    boxes["probs"], boxes["valid"] = _confidences(kind, rng, B, K)
    nv = int(boxes["valid"][0].sum())
    nbytes = lib.liso_mine_nms_workspace_bytes(B, K)
    assert nbytes == B * K * 72
    with guarded() as gd:
        for pre in sorted({0, -1, max(nv // 2, 1), nv, nv + 3}):  # <= 0: no cut; below, equal to, above sample 0's valid count
            want, want_enters, want_dense = OF.nms_prepare(boxes, pre)
            d = {k: dev(boxes[k]) for k in BOX_KEYS}
            dense, enters, ws = poisoned((B, K, 7), torch.float32), poisoned((B, K), torch.uint8), poisoned((nbytes,), torch.uint8)
            rc = lib.liso_mine_nms_prepare(B, K, pre, *[L.ptr(d[k]) for k in BOX_KEYS], L.ptr(dense), L.ptr(enters), L.ptr(ws), nbytes,
                                           L.stream_ptr())
            assert rc == 0
            for k in BOX_KEYS:
                assert_bits(f"pre_nms_max {pre}: {k}", d[k], want[k])
            assert_bits(f"pre_nms_max {pre}: enters", enters, want_enters)
            assert_bits(f"pre_nms_max {pre}: dense", dense, want_dense)
        gd.check()


# ---- NMS finish -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [65, 200])
def test_nms_finish_on_hand_made_survivor_lists(K):
    from oracle import flow_cluster as OF

    L = _L()
    lib = L.lib()
    B, b = 2, 1
    rng = np.random.default_rng(2000 + K)
    boxes = _random_boxes(rng, B, K)
    enters = (rng.random((B, K)) < 0.8).astype(np.uint8)  # independent of valid: entered-but-invalid and valid-but-not-entered slots
    both = np.flatnonzero((boxes["valid"][b] != 0) & (enters[b] != 0))
    listed = rng.permutation(K)[:K // 2]                   # in range, in no particular order, any kind of slot
    spare = int(np.setdiff1d(both, listed)[0])             # would survive if the kernel read behind `num`
    keep = np.full(K, spare, np.int64)
    n = listed.size + 4
    keep[:n] = np.concatenate([listed[:5], [-1], listed[5:9], [K], listed[9:], [listed[2], -7]])  # + a duplicate, out-of-range indices
    full = rng.integers(0, K, K).astype(np.int64)          # for num > K: K in-range entries, duplicates among them
    survivors = int(np.isin(both, listed).sum())
    assert survivors > 8 and ((boxes["valid"][b] == 0) & (enters[b] != 0))[listed].any() and ((boxes["valid"][b] != 0) & (enters[b] == 0))[listed].any()
    t_shapes = (((B, K, 3), np.float32), ((B, K, 3), np.float32), ((B, K), np.float32), ((B, K), np.uint8))
    t_pattern = tuple(pattern_like(s, dt) for s, dt in t_shapes)
    runs = [(keep, n, survivors - 2), (keep, n, survivors), (keep, n, survivors + 5), (keep, n, 0), (keep, 0, K), (keep, -3, K),
            (full, K + 5, K), (full, K + 5, 3)]
    with guarded() as gd:
        enters_d = dev(enters)
        for keep_h, num, max_boxes in runs:
            want, want_t = OF.nms_finish(b, boxes, enters, keep_h, num, max_boxes, t_pattern)
            d = {k: dev(boxes[k]) for k in BOX_KEYS}
            t = [poisoned(s, torch.from_numpy(np.zeros(0, dt)).dtype) for s, dt in t_shapes]
            rc = lib.liso_mine_nms_finish(b, K, max_boxes, L.ptr(dev(keep_h)), L.ptr(dev(np.array([num], np.int32))), L.ptr(enters_d),
                                          *[L.ptr(d[k]) for k in BOX_KEYS], *[L.ptr(x) for x in t], L.stream_ptr())
            assert rc == 0
            what = f"num {num}, max_boxes {max_boxes}: "
            if keep_h is keep:
                assert int(want["valid"][b].sum()) == (min(survivors, max_boxes) if num > 0 else 0)
            for k in BOX_KEYS:  # (sample 0 included: it must come back as it went in)
                assert_bits(what + k, d[k], want[k])
            for name, x, w in zip(("t_pos", "t_dims", "t_rot", "t_valid"), t, want_t):
                assert_bits(what + name, x, w)
        # more slots than the kernel's LDS flags hold: refused before anything is launched
        d = {k: dev(boxes[k]) for k in BOX_KEYS}
        t = [poisoned(s, torch.from_numpy(np.zeros(0, dt)).dtype) for s, dt in t_shapes]
        args = [L.ptr(dev(keep)), L.ptr(dev(np.array([n], np.int32))), L.ptr(enters_d), *[L.ptr(d[k]) for k in BOX_KEYS], *[L.ptr(x) for x in t]]
        assert lib.liso_mine_nms_finish(0, 16385, 5, *args, L.stream_ptr()) == EINVAL
        assert lib.liso_mine_nms_finish(0, 0, 5, *args, L.stream_ptr()) == EINVAL
        gd.check()
        for k in BOX_KEYS:
            assert_bits("refused: " + k, d[k], boxes[k])
