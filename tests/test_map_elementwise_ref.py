"""CPU checks of tests/_map_elementwise_ref.py (no GPU): every case stays
inside its cap by the float64 oracle alone and reaches what it was picked for
(every mask with both outcomes), the fp32 restatements agree with the pinned
ones (oracle.tracking.loss_tracking and compute_grad_mask, the CPU branch of
wgsr.uncertainty.dino_regularization_loss, tests/golden/track_cases.npz and
dino_cases.npz, wgsr.camera.se3_exp with torch.optim.Adam) and pass the bound
with margin 1, and single corruptions of a restatement fail the check."""
import copy
import os

import numpy as np
import pytest
import torch

import _map_elementwise_ref as E
from _util import GOLDEN, rel_l1
from oracle import tracking as ot

TRACK_ALL = E.track_case_names()
POSE_ALL = E.pose_case_names()
DINO_ALL = list(E.DINO_CASES)


def _mutated(o32, k, f):
    got = copy.copy(o32)
    got[k] = np.array(o32[k], np.float64, copy=True)
    f(got[k])
    return got


def _ratios_ok(r):
    return all(v <= 1.0 for v in r.values())


# ------------------------------------------------------------ tracking loss

@pytest.mark.parametrize("name", TRACK_ALL)
def test_track_caps_census_and_restatement(name):
    c = E.track_case(name)
    print(f"{name}: {int(c.near.sum())} of {c.near.size} pixels excluded, DELTA {c.delta}")
    assert c.near.mean() <= E.CAP_LOSS
    if c.near.size > 1:  # (a one-pixel image has one outcome)
        for k, m in c.census.items():
            assert m.any() and not m.all(), f"{k} has one outcome only"
    assert float(c.t["ea"]) != 0 and float(c.t["eb"]) != 0
    assert _ratios_ok(E.track_check(c, c.o32, margin=1))
    # no decision is taken the other way by the restatement off the excluded pixels
    for k in E.TRACK_TENSORS:
        d = np.abs(c.o32[k] - c.o64[k])[:, ~c.near]
        assert d.size == 0 or d.max() <= 1e-4 * max(np.abs(c.o64[k]).max(), 1e-30)


@pytest.mark.parametrize("name", TRACK_ALL)
def test_track_restatement_is_the_pinned_loss(name):
    c = E.track_case(name)
    v = {k: x.clone() for k, x in c.t.items()}
    for k in ("ren", "opa", "ea", "eb"):
        v[k].requires_grad_(True)
    gm = v["gm"] if c.use_gm else torch.ones_like(v["gm"])
    ot.loss_tracking(v["ren"], v["opa"], v["gt"], v["ea"], v["eb"], gm, v["unc"] if c.use_unc else None).backward()
    for k, t in (("d_image", v["ren"]), ("d_opacity", v["opa"]), ("d_exposure_a", v["ea"]), ("d_exposure_b", v["eb"])):
        np.testing.assert_allclose(c.o32[k], t.grad.numpy(), rtol=2e-6, atol=1e-7 * np.abs(c.o64[k]).max())


def test_track_restatement_matches_the_reference_fixtures():
    z = np.load(os.path.join(GOLDEN, "track_cases.npz"))
    for k in sorted({n.split("_")[0] for n in z.files}):
        f = {n[len(k) + 1:]: z[n] for n in z.files if n.startswith(k + "_")}
        t = {n: torch.from_numpy(np.ascontiguousarray(f[n])) for n in ("gt", "ren", "opa", "gm", "ea", "eb")}
        use_unc = "unc" in f
        t["unc"] = torch.from_numpy(f["unc"]) if use_unc else torch.ones(f["gt"].shape[1:])
        o = E.track_run(t, True, use_unc, torch.float32)
        assert abs(o["loss"] - float(f["loss"])) <= 1e-6 * abs(float(f["loss"]))
        for mine, theirs in (("d_image", "g_ren"), ("d_opacity", "g_opa"), ("d_exposure_a", "g_ea"),
                             ("d_exposure_b", "g_eb")):
            np.testing.assert_allclose(o[mine], f[theirs], rtol=2e-6, atol=1e-7 * np.abs(f[theirs]).max())


@pytest.mark.parametrize("name", [n for n in TRACK_ALL if n.startswith(("7x37", "33x129"))])
def test_track_corruptions_fail(name):
    c = E.track_case(name)
    far = np.argwhere(~c.near & (np.abs(c.o64["d_image"]).sum(0) > 0))
    y, x = (int(v) for v in far[len(far) // 2])
    with pytest.raises(AssertionError, match="d_image"):
        E.track_check(c, _mutated(c.o32, "d_image", lambda g: g[:, y, x].__imul__(0.5)))
    g64 = c.o64["d_opacity"][0]
    ok = np.argwhere(~c.near[:, :-1] & ~c.near[:, 1:] & (g64[:, :-1] != g64[:, 1:]))
    i, j = (int(v) for v in ok[len(ok) // 2])

    def neighbour(g):
        g[0, i, j] = g[0, i, j + 1]
    with pytest.raises(AssertionError, match="d_opacity"):
        E.track_check(c, _mutated(c.o32, "d_opacity", neighbour))
    assert (c.H * c.W) % E.WGROUP
    dropped = E.track_run(c.t, c.use_gm, c.use_unc, torch.float32, drop_last_group=True)
    with pytest.raises(AssertionError, match="loss"):
        E.track_check(c, {**c.o32, "loss": dropped["loss"]})


# ------------------------------------------------------------ gradient mask

@pytest.mark.parametrize("name", list(E.GMASK_CASES))
def test_gmask_caps_and_restatement(name):
    c = E.gmask_case(name)
    print(f"{name}: {int(c.flagged.sum())} of {c.flagged.size} pixels flagged, DELTA {c.delta}")
    assert c.flagged.mean() <= E.CAP_MASK
    E.gmask_check(c, np.where(c.inside, c.o32["mask"], c.o32["inten"]))
    # the eps mask takes both values, also on the reflect-padded edge
    dark = np.abs(c.o64["grey"]) <= E.EPS_GREY
    edge = np.zeros_like(dark)
    edge[[0, -1], :] = edge[:, [0, -1]] = True
    assert dark.any() or E.GMASK_CASES[name][2] in ("columns", "spikes")
    if E.GMASK_CASES[name][2] == "dark":
        assert (dark & edge).any() and (~dark & edge).any()
    if (c.H // 32) * (c.W // 32) > 1:   # (a block of one element is under 4 x itself: all zero)
        m = c.o64["mask"][c.inside]
        assert (m == 1).any() and (m == 0).any()


def test_gmask_cases_reach_what_they_were_picked_for():
    size = {n: (E.GMASK_CASES[n][0] // 32) * (E.GMASK_CASES[n][1] // 32) for n in E.GMASK_CASES}
    assert [size[n] for n in ("40x45", "33x65", "64x96", "64x96-t1", "96x160", "544x544", "64x64-flat",
                              "64x66-columns", "67x100", "64x66-spikes")] == [1, 2, 6, 6, 15, 289, 4, 4, 6, 4]
    assert all(size[n] == 0 for n in ("2x2", "31x70", "70x31"))
    for n in ("40x45", "67x100"):   # remainder strips exist both ways
        c = E.gmask_case(n)
        assert (~c.inside[-1, :]).all() and (~c.inside[:, -1]).all() and c.inside[0, 0]
    c = E.gmask_case("64x64-flat")   # whole blocks at median 0, and not flagged
    zero_t = (c.o64["t"] == 0) & (c.o32["t"] == 0)
    assert zero_t.sum() >= 4 * 50 and not c.flagged[zero_t].any()
    c = E.gmask_case("64x66-columns")   # 4 x median >= 1 ends a block all zero; the first block column keeps ones
    t = c.o64["t"][c.inside]
    assert (t >= 1).sum() >= 0.9 * t.size and abs(np.median(c.o64["inten"][:, 1:64]) - 0.49) < 1e-3
    assert not c.o64["mask"][:, 2:64].any() and c.o64["mask"][:, 1].all() and not c.o64["mask"][:, 0].any()
    c = E.gmask_case("64x66-spikes")   # v > t >= 1: set to 1 by the first assignment, to 0 by the second
    undone = c.inside & ~c.flagged & (c.o64["t"] >= 1) & (c.o64["d"] > 0)
    assert undone.sum() >= 32 and not c.o64["mask"][undone].any()
    c = E.gmask_case("64x96-t1")   # at multiplier 1 the median is its own threshold: structural, not flagged
    assert ((c.o64["d"] == 0) & c.inside & ~c.flagged).sum() >= 1000


@pytest.mark.parametrize("name", list(E.GMASK_CASES))
def test_gmask_restatement_is_the_pinned_mask(name):
    c = E.gmask_case(name)
    want = ot.compute_grad_mask(torch.from_numpy(c.img), c.mult)[0].numpy()
    raw = ~c.inside & ~c.eps_near
    np.testing.assert_allclose(c.o32["inten"][raw], want[raw], rtol=0, atol=1e-6)
    blk = c.inside & ~c.flagged
    np.testing.assert_array_equal(c.o32["mask"][blk], want[blk])


def _gmask_tooth(c, **teeth):
    o = E.gmask_run(c.img, c.mult, np.float32, **teeth)
    return np.where(c.inside, o["mask"], o["inten"])


def test_gmask_corruptions_fail():
    c = E.gmask_case("64x96")
    with pytest.raises(AssertionError, match="unflagged block pixels differ"):
        E.gmask_check(c, _gmask_tooth(c, median="upper"))
    c = E.gmask_case("64x66-spikes")
    with pytest.raises(AssertionError, match="unflagged block pixels differ"):
        E.gmask_check(c, _gmask_tooth(c, keep_one=True))
    for name, match in (("31x70", "intensity"), ("67x100", "unflagged block pixels differ")):
        c = E.gmask_case(name)
        with pytest.raises(AssertionError, match=match):
            E.gmask_check(c, _gmask_tooth(c, top="edge"))
    # one differing pixel anywhere off the flagged ones is enough
    c = E.gmask_case("544x544")
    got = np.where(c.inside, c.o32["mask"], c.o32["inten"])
    y, x = np.argwhere(c.inside & ~c.flagged)[12345]
    got[y, x] = 1 - got[y, x]
    with pytest.raises(AssertionError, match="1 unflagged block pixels differ"):
        E.gmask_check(c, got)


# ---------------------------------------------------------------- pose step

@pytest.mark.parametrize("name", POSE_ALL)
def test_pose_restatement_passes_with_margin_one(name):
    c = E.pose_case(name)
    assert not c.conv_near
    assert _ratios_ok(E.pose_check(c, c.o32, c.conv, margin=1))
    assert abs(c.angle - float(name.split("_")[0][1:])) <= 1e-6 * c.angle
    assert c.n_part in (1, 3, 1500) and (c.n_part <= 1024 or c.n_part > 1024)


def test_pose_cases_take_both_branches_and_both_outcomes():
    cs = [E.pose_case(n) for n in POSE_ALL]
    assert {c.conv for c in cs} == {0, 1}
    assert any(c.angle < 1e-5 for c in cs) and any(0 < c.angle < 1e-5 for c in cs) and any(c.angle > 0.5 for c in cs)


@pytest.mark.parametrize("name", POSE_ALL)
def test_pose_restatement_is_adam_and_the_pinned_se3_exp(name):
    """One torch.optim.Adam step over the four groups and update_pose with
    wgsr.camera.se3_exp, in float64, against the float64 restatement."""
    from wgsr.camera import se3_exp
    c = E.pose_case(name)
    st = c.st.astype(np.float64)
    rot, trans = torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    a, b = torch.tensor([st[12]]), torch.tensor([st[13]])
    ps = [rot, trans, a, b]
    opt = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(ps, (c.lr[0], c.lr[1], c.lr[2], c.lr[2]))],
                           betas=E.POSE_BETAS, eps=E.POSE_EPS)
    part = c.part.astype(np.float64)
    grads = [c.dtau[3:6], c.dtau[0:3], [part[:, 1].sum()], [part[:, 2].sum()]]
    for p, g, sl in zip(ps, grads, (slice(16, 19), slice(19, 22), slice(22, 23), slice(23, 24))):
        p.grad = torch.tensor(np.asarray(g, np.float64))
        opt.state[p] = dict(step=torch.tensor(float(c.step - 1)), exp_avg=torch.tensor(st[sl]),
                            exp_avg_sq=torch.tensor(st[sl.start + 8:sl.stop + 8]))
    opt.step()
    w2c = torch.eye(4, dtype=torch.float64)
    w2c[:3, :3], w2c[:3, 3] = torch.tensor(st[0:9]).view(3, 3), torch.tensor(st[9:12])
    new = se3_exp(torch.cat([trans, rot])) @ w2c
    tol = dict(rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(c.o64[0:9], new[:3, :3].reshape(-1).numpy(), **tol)
    np.testing.assert_allclose(c.o64[9:12], new[:3, 3].numpy(), **tol)
    np.testing.assert_allclose(c.o64[12:14], [float(a), float(b)], **tol)
    view = new.T
    np.testing.assert_allclose(c.o64[32:48], view.reshape(-1).numpy(), **tol)
    np.testing.assert_allclose(c.o64[48:64], (view @ torch.tensor(c.proj.astype(np.float64)).view(4, 4)).reshape(-1),
                               **tol)
    # (-T^T R is the inverse's row for an orthogonal R; the fp32 state's R is orthogonal to 1e-7)
    np.testing.assert_allclose(c.o64[64:67], torch.linalg.inv(view)[3, :3].numpy(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(c.o64[67], float(torch.cat([trans, rot]).norm()), **tol)


@pytest.mark.parametrize("name", ["a1_s7_n3", "a0.01_s1_n1500", "a1_s1_n1"])
def test_pose_corruptions_fail(name):
    c = E.pose_case(name)
    for tooth, match in (("swap_c2c3", "T"), ("campos_sign", "campos"), ("no_bc2", "exposures")):
        got = E.pose_step(c.st, c.dtau, c.part, c.proj, c.lr, c.step, np.float32, tooth=tooth)[0]
        assert not np.array_equal(got, c.o32), tooth
        with pytest.raises(AssertionError, match=match):
            E.pose_check(c, got, c.conv)
    wrong = c.cam32.copy()
    wrong[64:67] *= -1
    with pytest.raises(AssertionError, match="campos"):
        E.pose_check_camera(c, wrong)
    E.pose_check_camera(c, c.cam32, margin=1)


# --------------------------------------------------------------------- DINO

@pytest.mark.parametrize("name", DINO_ALL)
def test_dino_zero_near_rows_and_restatement(name):
    c = E.dino_case(name)
    print(f"{name}: seed {c.seed}, DELTA {c.delta:.3e}, {int(c.near.sum())} near rows of {c.N}, "
          f"{int(c.over.sum())} rows with more than {c.K} candidates, {int(c.inside.sum())} cut inside a tie")
    assert not c.near.any() and E.dino_needs(c)
    assert c.u.min() >= 0.1 and c.u.max() <= 2.1
    assert _ratios_ok(E.dino_check(c, c.o32, margin=1))
    # the restatement takes every selection the way float64 does
    np.testing.assert_array_equal(c.o32["count"], c.o64["count"])


def test_dino_cases_reach_their_kernels():
    """The dispatch condition of wgsr_dino_reg (C % 64 == 0 and C <= 384: the
    MFMA kernel), restated on the shapes."""
    mfma = lambda C: C % 64 == 0 and C <= 384  # noqa: E731
    want = {"150x100": False, "130x33": False, "161x64": True, "160x384": True, "300x448": False, "96x768": False,
            "60x16": False, "3x16": False, "1x64": True, "64x64-apart": True}
    for n, m in want.items():
        assert mfma(E.DINO_CASES[n][1]) == m, n
    assert 100 % 32 == 4 and 33 % 32 == 1 and 768 // 32 == 24
    for N, C in E.DINO_PAD:
        assert mfma(C) and not mfma(C + 1)
    assert mfma(E.dino_case("ties-adjacent-k127").C) and not mfma(E.dino_case("ties-far-k127").C)


def test_dino_tie_cases_cut_inside_and_between_pairs():
    for lay in ("adjacent", "far"):
        odd, even = E.dino_case(f"ties-{lay}-k127"), E.dino_case(f"ties-{lay}-k128")
        assert odd.N == 192 and int(odd.inside.sum()) >= 8 and int((even.over & ~even.inside).sum()) >= 8
        a = np.arange(0, 192, 2) if lay == "adjacent" else np.arange(96)
        b = a + 1 if lay == "adjacent" else a + 96
        assert np.array_equal(odd.feat[a].view(np.uint32), odd.feat[b].view(np.uint32))
        assert np.array_equal(odd.u[a].view(np.uint32), odd.u[b].view(np.uint32))
        assert len(np.unique(odd.feat[a], axis=0)) == 96
        S = odd.o64["S"]
        assert np.array_equal(S[:, a], S[:, b])
        # the pair the cut falls inside: one copy selected, one not, and (far) in different 64-sample chunks
        straddle = 0
        for i in range(192):
            sel = set(E.dino_select(S, i, odd.K).tolist())
            cut = [(x, y) for x, y in zip(a, b) if (x in sel) != (y in sel)]
            assert len(cut) == 1 and cut[0][0] in sel   # index order: the first copy is the one taken
            straddle += cut[0][0] // 64 != cut[0][1] // 64
        assert straddle == (192 if lay == "far" else 0)


def test_dino_restatement_is_the_pinned_loss():
    from wgsr.uncertainty import dino_regularization_loss
    for name in ("150x100", "161x64", "300x448", "60x16", "64x64-apart", "ties-far-k128"):
        c = E.dino_case(name)
        u = torch.from_numpy(c.u).requires_grad_(True)
        ref = dino_regularization_loss(u, torch.from_numpy(c.feat))
        ref.backward()
        ref = float(ref.detach())
        assert abs(c.o32["loss"] - ref) <= 1e-5 * abs(ref) + 1e-12, name
        assert rel_l1(c.o32["grad_u"], u.grad.numpy()) <= 1e-5, name
    z = np.load(os.path.join(GOLDEN, "dino_cases.npz"))
    for ci in range(3):
        k = f"c{ci}_"
        feat = z[k + "feat"].reshape(-1, z[k + "feat"].shape[-1])
        o = E.dino_run(feat, z[k + "unc"].reshape(-1), np.float32)
        assert abs(o["loss"] - float(z[k + "loss"])) <= 1e-5 * abs(float(z[k + "loss"])), ci
        assert rel_l1(o["grad_u"], z[k + "grad"].reshape(-1)) <= 1e-5, ci


def test_dino_corruptions_fail():
    c = E.dino_case("161x64")
    row = int(np.flatnonzero(c.over)[3])
    got = E.dino_run(c.feat, c.u, np.float32, c.K, tooth="k_plus_1", tooth_row=row)
    assert got["count"][row] == c.K + 1
    with pytest.raises(AssertionError, match="row_var.*grad_u"):
        E.dino_check(c, got)
    i, j = 40, int(np.argsort(c.o64["S"][40])[80])
    with pytest.raises(AssertionError, match="S"):
        E.dino_check(c, _mutated(c.o32, "S", lambda s: s[i, j:j + 1].__iadd__(1e-4)))
    for name in ("ties-adjacent-k127", "ties-far-k127"):
        t = E.dino_case(name)
        got = E.dino_run(t.feat, t.u, np.float32, t.K, tooth="tie_twice", tooth_row=17)
        assert got["count"][17] == t.K
        with pytest.raises(AssertionError, match="row_var"):
            E.dino_check(t, got)
    # / c instead of / (c + eps) at c = 1 moves row_var by one ulp of a 1e-14 number: no rounding bound can see
    # that, the bit-equality of the single-sample rows with the fp32 restatement does
    a = E.dino_case("64x64-apart")
    rows = [r for r in range(a.N) if E.dino_run(a.feat, a.u, np.float32, a.K, tooth="no_eps", tooth_row=r)
            ["row_var_bits"][r] != a.o32["row_var_bits"][r]]
    assert len(rows) >= a.N // 4
    got = E.dino_run(a.feat, a.u, np.float32, a.K, tooth="no_eps", tooth_row=rows[0])
    with pytest.raises(AssertionError, match="single-sample rows"):
        E.dino_check(a, got)


# ------------------------------------------------------ mapping: activations

@pytest.mark.parametrize("P", E.MAP_P)
@pytest.mark.parametrize("iso", E.ISO_WEIGHTS)
def test_activation_caps_rows_and_restatement(P, iso):
    c = E.act_case(P, iso)
    print(f"{c.name}: {int(c.near.sum())} of {P} rows excluded, DELTA {c.delta:.3e}")
    assert c.near.mean() <= E.CAP_LOSS
    assert _ratios_ok(E.act_check_forward(c, c.o32, margin=1))
    assert _ratios_ok(E.act_check_backward(c, c.o32, margin=1))
    assert all(np.all(np.isfinite(c.o64[k])) for k in ("opacity", "scales", "rotations", "d_o", "d_s", "d_r"))
    if P > 16:
        s, q = c.inp["s"], c.inp["q"]
        assert c.inp["o"].max() == 20 and c.inp["o"].min() == -20 and s.min() == -9 and s.max() == 3
        assert int(c.equal3.sum()) == 2 and int(c.floor.sum()) == 3 and not q[10].any()
        assert abs(np.linalg.norm(q[9].astype(np.float64)) - 1e-20) < 1e-26
        assert not c.o64["rotations"][10].any() and np.abs(c.o64["rotations"][9]).max() < 1e-8
        for r in c.special["equal2"]:
            assert len(set(s[r].tolist())) == 2
        if c.iso_w:  # three bit-equal scales: the isotropic term contributes nothing, in autograd and in sgn - sm
            for r in c.special["equal3"]:
                np.testing.assert_allclose(c.o64["d_s"][r], c.inp["g_sc"][r].astype(np.float64) * c.o64["scales"][r],
                                           rtol=1e-12)
        assert np.abs(c.o64["d_r"][c.floor]).max() > 1e11   # g / 1e-12
        assert (c.inp["radii"] > 0).any() and (c.inp["radii"] < 0).any() and (c.inp["radii"] == 0).any()


@pytest.mark.parametrize("P", [255, 257, 1000])
def test_activation_backward_corruptions_fail(P):
    c = E.act_case(P, "10/3P")
    for tooth, match in (("no_sm", "d_s"), ("no_projection", "d_r")):
        got = E.act_run(c.inp, c.iso_w, torch.float32, tooth=tooth)
        with pytest.raises(AssertionError, match=match):
            E.act_check_backward(c, got)


# ------------------------------------------------------- mapping: rgbd loss

@pytest.mark.parametrize("H,W", E.MAP_IMAGES)
@pytest.mark.parametrize("use_ssim", [False, True])
def test_maploss_caps_census_and_restatement(H, W, use_ssim):
    c = E.maploss_case(H, W, use_ssim)
    print(f"{c.name}: {int(c.near.sum())} of {c.near.size} pixels excluded, DELTA {c.delta}")
    assert c.near.mean() <= E.CAP_LOSS
    if H * W > 1:
        for k, m in c.census.items():
            assert m.any() and not m.all(), f"{k} has one outcome only"
    assert _ratios_ok(E.maploss_check(c, c.o32, margin=1))
    # the per-pixel exposure terms sum to autograd's exposure gradients
    for a, b in (("sum_da", "grad_ea"), ("sum_db", "grad_eb")):
        np.testing.assert_allclose(c.o64[a], c.o64[b], rtol=1e-10, atol=1e-14)
    with pytest.raises(AssertionError, match="d_depth"):
        E.maploss_check(c, _mutated(c.o32, "d_depth", lambda g: g.__imul__(-1.0)))
