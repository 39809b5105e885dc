"""CPU checks of tests/_raster_rowwise_ref.py (no GPU): the cases stay inside
the masking caps, each reaches what it was picked for, the fp32 restatement
passes the bound with margin 1 (by construction) and today's rel-L1, and
mutations of the restatement's output that pass ``rel_l1 <= 1e-4`` -- the
only accuracy gate of tests/test_gpu_raster.py::check_against on gradients --
fail the row-wise check."""
import copy

import numpy as np
import pytest

import _raster_rowwise_ref as R
from _util import rel_l1

REL_L1_TOL = 1e-4  # GRAD_TOL / IMG_TOL of tests/test_gpu_raster.py
ALL = list(R.CASES) + R.golden_cases()
# the mutations need rows far below the tensor's sum for the old gate to miss
# them: the cases with more than a thousand Gaussians, or with gradients
# spread over many decades (saturated)
MUTATED = ["saturated", "deep_tile", "larger"]


def _spans(c, shift):
    """Visible Gaussians whose tile rectangle spans at least 2 bins at this shift."""
    r, vis = c.report["rect"], np.asarray(c.o64["radii"]) > 0
    x = ((r[:, 2] - 1) >> shift) > (r[:, 0] >> shift)
    y = ((r[:, 3] - 1) >> shift) > (r[:, 1] >> shift)
    return int(np.count_nonzero(vis & (x | y)))


@pytest.mark.parametrize("name", ALL)
def test_caps_hold(name):
    c = R.case(name)
    assert c.near_pixels.mean() <= R.MAX_MASKED, int(c.near_pixels.sum())
    for k in R.grad_tensors(c):
        carry = np.any(R.rows_of(c, k, c.o64[k]) != 0, axis=1)
        if carry.any():
            assert (carry & c.near_rows).sum() <= R.MAX_EXCLUDED * carry.sum(), k
    if name in R.CASES:
        assert c.inputs["means3D"].shape[0] % 64 != 0  # a part-filled last wave
        assert float(c.settings["bg"].abs().min()) >= 0 and float(c.settings["bg"].abs().max()) > 0
        assert (c.near_pixels.sum() + c.near_rows.sum()) < 20


def test_report_changes_no_other_output():
    """The oracle's near report is an addition: every other entry is bit for
    bit what a run without it returns (``small`` has no near pixel, so its
    masked upstream gradients are the unmasked ones)."""
    from oracle import dense
    c = R.case("small")
    assert not c.near_pixels.any()
    plain = dense.dense_forward_backward(c.inputs, c.settings, *c.grads)
    assert set(c.o64) - set(plain) == set(c.report)
    for k, v in plain.items():
        if v is not None:
            np.testing.assert_array_equal(np.asarray(v), np.asarray(c.o64[k]), err_msg=k)


def test_each_case_has_its_feature():
    small, wide, sat, deep = (R.case(n) for n in ("small", "wide", "saturated", "deep_tile"))
    assert small.settings["W"] % 16 and small.settings["H"] % 16          # partial tiles
    gx = (small.settings["W"] + 15) // 16
    assert gx % 2 and gx % 4                                               # partial bins at shift 1 and 2
    assert _spans(small, 1) >= 20 and _spans(small, 2) >= 5
    assert int(small.report["sh_clamped"].sum()) >= 10                     # clamped SH channels present
    assert _spans(wide, 1) >= 60 and _spans(wide, 2) >= 20
    r = wide.report["rect"]
    assert int(((r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1])).max()) >= 12   # many record slots per Gaussian
    assert int(sat.report["stopped"].sum()) >= 1000                        # pixels that stop early
    assert sat.report["sat_entries"] >= 1                                  # o G > 0.99
    live = np.any(sat.o64["dL_dmeans2D"] != 0, axis=1)
    assert np.count_nonzero((sat.o64["radii"] > 0) & ~live) >= 100         # list entries past the stop: no gradient
    assert int(deep.report["list_len"].max()) > 4 * 256                    # several render batches
    assert np.count_nonzero(deep.report["list_len"] > 256) <= 2            # ... in one or two tiles
    assert int(deep.report["stopped"].sum()) >= 10
    pre = R.case("precomp")
    assert set(R.grad_tensors(pre)) >= {"dL_dcolors", "dL_dcov3D"}
    assert np.abs(pre.o64["dL_dcolors"]).max() > 0 and np.abs(pre.o64["dL_dcov3D"]).max() > 0
    sm = R.case("scalemod")
    assert sm.settings["scale_modifier"] == 1.7 and sm.settings["sh_degree"] == 1
    assert sm.inputs["shs"].shape[1] == 16
    sh = R.rows_of(sm, "dL_dsh", sm.o64["dL_dsh"])
    assert np.abs(sh[:, :12]).max() > 0 and not np.any(sh[:, 12:])
    lg = R.case("larger")
    assert (lg.settings["W"], lg.settings["H"]) == (136, 104) and _spans(lg, 2) >= 50
    assert R.carrying(lg, "dL_dmeans3D").size > 2 * 256                    # several workgroups of 256 Gaussians


@pytest.mark.parametrize("name", ALL)
def test_restatement_passes_with_margin_one_and_todays_rel_l1(name):
    c = R.case(name)
    ratios = R.check(c, c.o32, margin=1)
    assert all(r <= 1.0 for r in ratios.values())
    for k in R.IMAGES + tuple(R.grad_tensors(c)):
        assert rel_l1(c.o32[k], c.o64[k]) <= REL_L1_TOL, k
    assert rel_l1(c.o32["dL_dtau"].sum(0), c.o64["dL_dtau"]) <= 1e-3


def _passes_rel_l1(c, got):
    return all(rel_l1(got[k], c.o64[k]) <= REL_L1_TOL for k in R.IMAGES + tuple(R.grad_tensors(c)))


def _mutants(c, k):
    """(what, mutated copy of the restatement's output) for gradient tensor k.

    rel-L1 sees a row by its share of the tensor's sum, so at these sizes
    (about a thousand rows) it misses a 100 % error only on rows of the lowest
    group; the scaled row is the largest of the middle group."""
    gr = R.groups(c, k)

    def mutant(row, f):
        got = copy.copy(c.o32)
        got[k] = c.o32[k].copy()
        v = got[k].reshape(got[k].shape[0], -1)
        v[row] = f(v[row])
        return got

    def negate(v):
        v = v.copy()
        j = int(np.argmax(np.abs(v)))
        v[j] = -v[j]
        return v
    mid = gr[len(gr) // 2]
    yield "a mid-magnitude row scaled by 1.001", mutant(mid[-1], lambda v: v * np.float32(1.001))
    yield "a small-magnitude row replaced by zero", mutant(gr[0][len(gr[0]) // 4], lambda v: v * 0)
    yield "one component of a row negated", mutant(gr[0][len(gr[0]) // 8], negate)


@pytest.mark.parametrize("name", MUTATED)
def test_row_mutations_pass_rel_l1_and_fail_the_rowwise_check(name):
    c = R.case(name)
    for k in R.grad_tensors(c):
        if k == "dL_dmeans2D":
            continue  # (its third column is structurally zero; covered through dL_dmeans3D)
        for what, got in _mutants(c, k):
            assert _passes_rel_l1(c, got), (k, what, rel_l1(got[k], c.o64[k]))
            with pytest.raises(AssertionError, match=k):
                R.check(c, got)


@pytest.mark.parametrize("name", MUTATED)
def test_colour_patch_mutation_passes_rel_l1_and_fails_the_rowwise_check(name):
    c = R.case(name)
    got = copy.copy(c.o32)
    got["color"] = c.o32["color"].copy()
    got["color"][:, 20:24, 36:40] += np.float32(2e-5)
    assert not c.near_pixels[20:24, 36:40].all()
    assert _passes_rel_l1(c, got)
    with pytest.raises(AssertionError, match="color"):
        R.check(c, got)
