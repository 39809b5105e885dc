"""GPU: csrc/dino.hip element by element against the float64 oracle, through
wgsr_dino_reg on the test's own guarded scratch buffers, so that the N x N
similarity S, row_var, grad_u and the loss are all read back
(tests/_map_elementwise_ref.py holds the cases, each with ZERO near rows by
the float64 oracle alone, and the bound; tests/test_map_elementwise_ref.py
shows on the CPU that the check fails on a row selecting K + 1, a tie taken
twice, one S entry moved by 1e-4 and row_var divided by c instead of c + eps).

* S per element, row_var per row, grad_u per sample, the loss; a row that
  selects itself alone is bit-equal to the fp32 restatement.
* k_dino_similarity2 (MFMA) against k_dino_similarity (VALU): one zero column
  appended to the features takes the other kernel and changes no product and
  no sum, so S, row_var and the loss must be BIT-EQUAL.
* Ties: 96 samples stored twice, at an even top_k (every row cuts between two
  pairs) and an odd one (every row cuts inside a pair).
* Two runs give bit-equal S, row_var and loss.
"""
import numpy as np
import pytest
import torch

import _map_elementwise_ref as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PLAIN = [n for n in E.DINO_CASES if not n.startswith("pad-")]


def run(feat, u, top_k=E.DINO_K):
    from wgsr import _lib
    L = _lib.load()
    N, C = feat.shape
    f, uu = (torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (feat, u))
    fn, S, rv, gu, loss = (E.Guarded(s) for s in ((N, C), (N, N), (N,), (N,), (1,)))
    with torch.cuda.device(DEV):
        _lib.check(L.wgsr_dino_reg(_lib.ptr(uu), _lib.ptr(f), N, C, top_k, E.DINO_TH, E.DINO_EPS, fn.ptr(), S.ptr(),
                                   rv.ptr(), gu.ptr(), loss.ptr(), _lib.stream_handle(DEV)))
    torch.cuda.synchronize()
    fn.read()
    return dict(S=S.read(), row_var=rv.read(), grad_u=gu.read(), loss=loss.read()[0])


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", PLAIN)
def test_dino_elements_match_the_float64_oracle(name):
    c = E.dino_case(name)
    E.dino_check(c, run(c.feat, c.u, c.top_k))


@pytest.mark.parametrize("N,C", E.DINO_PAD)
def test_dino_similarity_kernels_are_bit_identical(N, C):
    c = E.dino_case(f"pad-{N}x{C}")
    mfma = run(c.feat, c.u)
    valu = run(np.concatenate([c.feat, np.zeros((N, 1), np.float32)], 1), c.u)
    for k in ("S", "row_var", "loss"):
        diff = _bits(mfma[k]) != _bits(valu[k])
        assert not diff.any(), f"{k}: {int(diff.sum())} of {diff.size} elements differ in bits between the two kernels"
    E.dino_check(c, mfma)
    E.dino_check(c, valu)   # (grad_u: unordered atomics, inside the bound both times)


@pytest.mark.parametrize("name", ["161x64", "150x100", "ties-far-k127"])
def test_dino_is_repeatable(name):
    c = E.dino_case(name)
    a, b = run(c.feat, c.u, c.top_k), run(c.feat, c.u, c.top_k)
    for k in ("S", "row_var", "loss"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
