"""The target renderer on the device (liso_amd/csrc/detector_loss.hip: targets_box_max / targets_render) against
tests/center_loss_cases.py:targets_fp64 on non-square grids and ranges, centre cells on cell borders and the grid's edge, duplicate
boxes, boxes whose in-grid maximum is off their centre, padded slots holding zeros or NaN, K = 0 / 1 / 300 and awkward rotations.

Bounds (set before any run): probs within 1e-5 absolute in EVERY cell (the maximum over boxes is continuous); dims, pos and rot within
1e-5 * max(max |ref|, 1) in every cell the reference does not flag; in a flagged cell the attributes of one of the near-tied winners, or
zeros at the threshold; the centre mask equal everywhere; two calls bit-identical.  At most 2 cells per case are flagged (asserted on
the CPU, tests/test_center_loss_cases.py); in the cases here none is.

Worst values observed on an MI355X over all 15 cases: probs 5.2e-7 absolute; dims 5.0e-8, pos 6.5e-8, rot 4.9e-8 of their scale
(bound 1e-5 each); excluded cells: 0 in every case.

The border cases found the one defect: the kernel formed `pos + range / 2` in fp32, which rounds the largest coordinate below range / 2
up to the border, so that box marked no centre cell; it now compares the coordinate with the cell's borders, formed in fp64 and rounded
up to fp32 (an fp32 p satisfies p >= b exactly when p >= the smallest fp32 not below b).  The host formulation truncated instead of
flooring and marked cell 0 for a centre just below -range / 2 (tests/test_center_loss_cases.py).
What else the cases are there to catch (checked once against deliberately wrong builds, never committed): range_x and range_y swapped
in the cell centres -> every non-square case; the `>= 0` guards of the centre cell dropped -> the border cases and the box beyond the
low edge; `h >= 0.999 best` for `h == best` -> the near-tie case alone (300 random boxes do not show it)."""
import functools

import pytest
import torch

from tests import center_loss_cases as C

pytestmark = pytest.mark.gpu

CASES = C.target_cases()
ATTRS = ("dims", "pos", "rot")


@functools.lru_cache(maxsize=None)
def _ref(cid):
    c = CASES[cid]
    return C.targets_fp64(c["pos"], c["dims"], c["rot"], c["valid"], c["grid"], c["range"])


def _render(c):
    from liso_amd.datasets.targets import render_center_targets

    out = render_center_targets(c["pos"].cuda(), c["dims"].cuda(), c["rot"].cuda(), c["valid"].cuda(), c["grid"], c["range"])
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("cid", list(CASES))
def test_target_maps_match_fp64(cid):
    c, ref = CASES[cid], _ref(cid)
    got, again = _render(c), _render(c)
    flagged = ref["winner_uncertain"] | ref["threshold_uncertain"]
    err_p = float((got["probs"].double() - ref["probs"]).abs().max())
    print(f"{cid}: probs max abs err {err_p:.3e}; excluded cells {int(flagged.sum())} "
          f"(winner {int(ref['winner_uncertain'].sum())}, threshold {int(ref['threshold_uncertain'].sum())})")
    errs = {}
    for k in ATTRS:
        scale = max(float(ref[k].abs().max()), 1.0)
        d = (got[k].double() - ref[k]).abs().amax(-1)
        d = torch.where(torch.isfinite(got[k]).all(-1), d, torch.full_like(d, float("inf")))
        errs[k] = (float(d[~flagged].max()), scale)
        print(f"{cid}: {k} max abs err {errs[k][0]:.3e} over scale {scale:.3g} = {errs[k][0] / scale:.2e}")
    assert bool(torch.isfinite(got["probs"]).all()) and err_p <= 1e-5
    for k in ATTRS:
        assert errs[k][0] <= 1e-5 * errs[k][1], (k, errs[k])
    for b, y, x in flagged.nonzero().tolist():
        row = torch.cat([got[k][b, y, x].double() for k in ATTRS])
        options = list(ref["candidates"].get((b, y, x), [torch.cat([ref[k][b, y, x] for k in ATTRS])]))
        if bool(ref["threshold_uncertain"][b, y, x]):
            options.append(torch.zeros(8, dtype=torch.float64))
        assert any(float((row - o).abs().max()) <= 1e-5 * max(float(o.abs().max()), 1.0) for o in options), (b, y, x, row, options)
    assert torch.equal(got["center_bool_mask"], ref["center_bool_mask"])
    for k in got:
        assert torch.equal(got[k], again[k]), k
    if "same_as" in c:  # padding must not change a single bit
        base = _render(CASES[c["same_as"]])
        for k in got:
            assert torch.equal(got[k], base[k]), k


def test_border_centres_mark_the_cells_worked_out_by_hand():
    for cid in ("border-64x64", "border-64x32"):
        got = _render(CASES[cid])
        assert torch.equal(got["center_bool_mask"], C.border_expectation(CASES[cid])), cid


def test_empty_inputs_render_background():
    for cid in ("k0", "all-invalid"):
        got = _render(CASES[cid])
        assert all(float(got[k].abs().sum()) == 0.0 for k in ("probs",) + ATTRS) and not bool(got["center_bool_mask"].any()), cid


def test_identical_boxes_add_their_attributes_and_keep_the_heat():
    c = CASES["duplicate"]
    i, j = c["duplicate"]
    got = _render(c)
    keep = [k for k in range(c["valid"].shape[1]) if k != j]
    one = _render({**c, **{k: c[k][:, keep] for k in ("pos", "dims", "rot", "valid")}})
    assert torch.equal(got["probs"], one["probs"]) and torch.equal(got["center_bool_mask"], one["center_bool_mask"])
    won = (one["dims"][0] == c["dims"][0, i]).all(-1) & (one["pos"][0] == c["pos"][0, i]).all(-1)
    assert int(won.sum()) >= 4
    for k in ATTRS:
        assert torch.equal(got[k][0][won], 2.0 * one[k][0][won]), k
        assert torch.equal(got[k][0][~won], one[k][0][~won]), k


def test_normalisation_by_the_in_grid_maximum():
    c = CASES["normalisation"]
    got = _render(c)
    keep = [k for k in range(5) if k != c["far_box"]]
    without = _render({**c, **{k: c[k][:, keep] for k in ("pos", "dims", "rot", "valid")}})
    for k in got:  # ten ranges away: the maximum underflows, the clamp holds, the box leaves no trace
        assert torch.equal(got[k], without[k]), k
    for k in c["beyond_edge"]:  # a centre 1 m beyond the edge: the edge cells reach exactly 1.0
        alone = _render({**c, **{n: c[n][:, k:k + 1] for n in ("pos", "dims", "rot", "valid")}})
        assert float(alone["probs"].max()) == 1.0 and not bool(alone["center_bool_mask"].any())


def test_a_lead_of_three_in_ten_thousand_is_no_tie():
    c = CASES["near-tie"]
    got = _render(c)
    col = got["dims"][0, :, c["near_tie_col"]]
    lit = got["probs"][0, :, c["near_tie_col"], 0] > 0.01
    assert int(lit.sum()) >= 5 and bool((col[lit] == c["dims"][0, 0]).all())
