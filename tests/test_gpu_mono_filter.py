"""GPU tests of ``wgsr.frontend.filter_mono_depth`` (csrc/droid_mono_filter.hip)
against the float64 restatement of tests/_mono_filter_ref.py, on the inputs of
tests/golden/ref_mono_filter.npz (whose recorded mask is the reference's own)
and on small cases generated here.

What is compared: the two int32 count maps and the mask, which must be EQUAL
at every target the restatement does not mark ambiguous.  A target is ambiguous
when a candidate that can reach it sits within 1e-3 px of a rounding boundary
(the fp32 ulp at coordinate 75 is 8e-6, at 230 it is 1.5e-5: 60 ulps or more),
within 1e-5 of the Z threshold, or has a cosine within 1e-4 of the similarity
threshold (C <= 384 fp32 terms at 6e-8 each: an error of at most 2.3e-5), or
when its winner's err lies within 1e-4 of the error threshold.  The ambiguous
targets may be at most 5 % of H W, asserted before anything is compared.
"""
import os

import numpy as np
import pytest
import torch

import _mono_filter_ref as mf
from _util import GOLDEN

pytestmark = pytest.mark.gpu

_cache = {}


def _fixture():
    if "fixture" not in _cache:
        z = np.load(os.path.join(GOLDEN, "ref_mono_filter.npz"))
        inp = {k: z[k] for k in ("poses", "disps", "mask", "intrinsics", "dino")}
        _cache["fixture"] = (inp, int(z["idx"]), z["jj"], z["mask_out"])
    return _cache["fixture"]


def _small(name):
    """the generated cases, made once: (inputs, idx, jj)"""
    if name in _cache:
        return _cache[name]
    if name == "border":  # a 2 x 3 cell map: every blend clamps at a border
        xi = [[0, 0, 0, 0, 0, 0], [0.1, -0.04, 0.05, 0.01, -0.02, 0.02], [-0.08, 0.06, -0.3, -0.02, 0.02, -0.01]]
        inp = mf.make_case(28, 42, 16, xi, depth_scale={1: [(5, 15, 8, 20, 0.7)]}, seed=3, rank=4, noise=0.4)
        case = (inp, 0, [1, 2])
    elif name == "cells":  # 9 x 16 = 144 cells: 3 x 3 Gram tiles, some of a frame's own skipped; C = 40: a partial K chunk
        xi = [[0.02, 0.01, 0, 0, 0.01, 0], [0.1, -0.04, 0.05, 0.01, -0.02, 0.02], [-0.08, 0.06, -0.5, -0.02, 0.02, -0.01]]
        inp = mf.make_case(127, 230, 40, xi, depth_scale={2: [(30, 70, 60, 140, 0.75)]}, seed=5, rank=5, noise=0.6)
        case = (inp, 1, [2, 0])
    elif name == "identity":  # one neighbour with the keyframe's own pose, depth and features
        xi = [[0.05, -0.02, 0.03, 0.02, -0.01, 0.03]] * 2
        inp = mf.make_case(30, 45, 16, xi, seed=4, rank=4, noise=0.3)
        inp["disps"][:, 10:14, 20:30] = 0.0
        inp["disps"][1], inp["dino"][1] = inp["disps"][0], inp["dino"][0]
        case = (inp, 0, [1])
    inp["mask"] = np.ones(inp["disps"].shape, bool)
    inp["mask"][:, 1:3, 4:9] = False
    _cache[name] = case
    return case


def _ref(name, inp, idx, jj):
    key = ("ref", name, tuple(int(j) for j in jj))
    if key not in _cache:
        _cache[key] = mf.filter_mono_depth(inp["poses"], inp["disps"], inp["mask"], inp["intrinsics"], inp["dino"],
                                           idx, jj)
    return _cache[key]


def _run(inp, idx, jj, dino_on_host=False, **kw):
    """-> (mask [N, H, W], accurate, inaccurate) as numpy"""
    from wgsr.frontend import filter_mono_depth
    dev = torch.device("cuda:0")
    mask = torch.from_numpy(inp["mask"].copy()).to(dev)
    dino = torch.from_numpy(inp["dino"])
    acc, ina = filter_mono_depth(torch.from_numpy(inp["poses"]).to(dev), torch.from_numpy(inp["disps"]).to(dev), mask,
                                 torch.from_numpy(inp["intrinsics"]).to(dev), dino if dino_on_host else dino.to(dev),
                                 idx, jj, return_counts=True, **kw)
    return mask.cpu().numpy(), acc.cpu().numpy(), ina.cpu().numpy()


def _compare(name, inp, idx, jj, got):
    ref = _ref(name, inp, idx, jj)
    amb = ref["ambiguous"]
    assert amb.mean() <= mf.AMBIGUITY_CAP, amb.mean()
    mask, acc, ina = got
    keep = ~amb
    diff = (acc != ref["accurate"]) | (ina != ref["inaccurate"]) | (mask[idx] != ref["mask"])
    print(f"{name}: ambiguous {int(amb.sum())} of {amb.size} ({amb.mean():.2%}), differing inside them "
          f"{int((diff & amb).sum())}, outside {int((diff & keep).sum())}; matched share "
          f"{ref['matched'] / max(ref['valid'], 1):.3f}, collisions {ref['collisions']}")
    assert acc.dtype == np.int32 and ina.dtype == np.int32
    np.testing.assert_array_equal(acc[keep], ref["accurate"][keep])
    np.testing.assert_array_equal(ina[keep], ref["inaccurate"][keep])
    np.testing.assert_array_equal(mask[idx][keep], ref["mask"][keep])
    other = np.arange(mask.shape[0]) != idx
    np.testing.assert_array_equal(mask[other], inp["mask"][other])
    return ref


def test_fixture_counts_and_mask():
    inp, idx, jj, mask_out = _fixture()
    got = _run(inp, idx, jj)
    ref = _compare("fixture", inp, idx, jj, got)
    np.testing.assert_array_equal(ref["mask"], mask_out)  # (the restatement is the reference's result)
    keep = ~ref["ambiguous"]
    np.testing.assert_array_equal(got[0][idx][keep], mask_out[keep])
    # two calls give the same bits, and so does a call with the DINO maps left on the host
    for again in (_run(inp, idx, jj), _run(inp, idx, torch.from_numpy(jj), dino_on_host=True)):
        for a, b in zip(got, again):
            np.testing.assert_array_equal(a, b)


def test_empty_jj_leaves_the_mask_untouched():
    inp, idx, _ = _small("border")
    mask, acc, ina = _run(inp, idx, [])
    np.testing.assert_array_equal(mask, inp["mask"])
    assert not acc.any() and not ina.any()
    mask, acc, ina = _run(inp, idx, torch.empty(0, dtype=torch.int64, device="cuda:0"), check=False)
    np.testing.assert_array_equal(mask, inp["mask"])
    assert not acc.any() and not ina.any()


def test_a_frame_listed_twice_counts_twice():
    inp, idx, jj = _small("border")
    _, acc1, ina1 = _run(inp, idx, jj[:1])
    # (in a caller's scratch buffer, larger than needed and full of stale bits)
    from wgsr.frontend import mono_filter_workspace_bytes
    H, W = inp["disps"].shape[1:]
    ws = torch.full((mono_filter_workspace_bytes(3, H, W),), 0xFF, dtype=torch.uint8, device="cuda:0")
    assert mono_filter_workspace_bytes(2, H, W) < ws.numel()
    _, acc2, ina2 = _run(inp, idx, [jj[0], jj[0]], workspace=ws)
    assert acc1.any() and ina1.any()
    np.testing.assert_array_equal(acc2, 2 * acc1)
    np.testing.assert_array_equal(ina2, 2 * ina1)


@pytest.mark.parametrize("name", ["border", "cells"])
def test_small_cases(name):
    inp, idx, jj = _small(name)
    ref = _compare(name, inp, idx, jj, _run(inp, idx, jj))
    assert ref["accurate"].any() and ref["inaccurate"].any() and (inp["mask"][idx] & ~ref["mask"]).any()
    assert 0.1 < ref["matched"] / ref["valid"] < 0.99


def test_identity_pose_hits_every_target_once():
    inp, idx, jj = _small("identity")
    mask, acc, ina = _run(inp, idx, jj)
    positive = inp["disps"][idx] > 0
    assert positive.any() and not positive.all()
    np.testing.assert_array_equal(acc, positive.astype(np.int32))
    assert not ina.any()
    np.testing.assert_array_equal(mask, inp["mask"])


def test_bad_jj_is_refused_and_nothing_is_written():
    inp, idx, _ = _small("border")
    dev = torch.device("cuda:0")
    for jj in ([1, 3], torch.tensor([1, 3], device=dev), torch.tensor([-1], device=dev)):
        for host in (False, True):
            with pytest.raises(RuntimeError, match=r"jj"):
                _run(inp, idx, jj, dino_on_host=host)
    from wgsr.frontend import filter_mono_depth
    mask = torch.from_numpy(inp["mask"].copy()).to(dev)
    with pytest.raises(RuntimeError, match="WGSR_MONO_FILTER_BAD_JJ"):
        filter_mono_depth(torch.from_numpy(inp["poses"]).to(dev), torch.from_numpy(inp["disps"]).to(dev), mask,
                          torch.from_numpy(inp["intrinsics"]).to(dev), torch.from_numpy(inp["dino"]).to(dev), idx,
                          torch.tensor([2, 1, 7], device=dev))
    np.testing.assert_array_equal(mask.cpu().numpy(), inp["mask"])


def test_captures_into_a_graph():
    from wgsr.frontend import filter_mono_depth
    inp, idx, jj = _small("border")
    want = _run(inp, idx, jj)
    dev = torch.device("cuda:0")
    poses, disps = torch.from_numpy(inp["poses"]).to(dev), torch.from_numpy(inp["disps"]).to(dev)
    intr, dino = torch.from_numpy(inp["intrinsics"]).to(dev), torch.from_numpy(inp["dino"]).to(dev)
    start = torch.from_numpy(inp["mask"]).to(dev)
    mask = start.clone()
    jj_dev = torch.tensor(jj, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        acc, ina = filter_mono_depth(poses, disps, mask, intr, dino, idx, jj_dev, return_counts=True, check=False)
    for _ in range(2):
        mask.copy_(start)
        acc.fill_(-1)
        ina.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(want, (mask, acc, ina)):
            np.testing.assert_array_equal(a, b.cpu().numpy())
