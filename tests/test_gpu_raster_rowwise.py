"""GPU: the rasteriser's forward and backward through the ``_C`` ABI against
the float64 oracle, row by row (tests/_raster_rowwise_ref.py holds the cases,
the masking and the bound; tests/test_raster_rowwise_ref.py shows on the CPU
that the cases are decisive and that the check fails on single wrong rows).

Every case runs under both render-backward kernels (WGSR_BWD_SPLIT_BELOW 0:
k_render_bwd_quad, 1000000: k_render_bwd_seg) and bin shifts 0, 1, 2, and
the committed golden scenes run the same way.  Each check prints its worst
err / spread ratio per tensor and per row group (DESIGN.md records them).
"""
import pytest

import _raster_rowwise_ref as R
from test_gpu_raster import run_c

pytestmark = pytest.mark.gpu


def _run_and_check(name, monkeypatch, split_below, bin_shift, depth_sort=None):
    c = R.case(name)
    monkeypatch.setenv("WGSR_BWD_SPLIT_BELOW", split_below)
    monkeypatch.setenv("WGSR_BIN_SHIFT", bin_shift)
    if depth_sort is not None:
        monkeypatch.setenv("WGSR_DEPTH_SORT", depth_sort)
    out = run_c(c.inputs, c.settings, c.grads)
    return R.check(c, out)


@pytest.mark.parametrize("bin_shift", ["0", "1", "2"])
@pytest.mark.parametrize("split_below", ["0", "1000000"])
@pytest.mark.parametrize("name", list(R.CASES) + R.golden_cases())
def test_rows_match_the_float64_oracle(name, split_below, bin_shift, monkeypatch):
    _run_and_check(name, monkeypatch, split_below, bin_shift)


@pytest.mark.parametrize("split_below", ["0", "1000000"])
@pytest.mark.parametrize("name", ["wide", "deep_tile"])
def test_rows_match_with_the_global_depth_sort(name, split_below, monkeypatch):
    """The Gaussian-level depth sort ahead of the duplication
    (WGSR_DEPTH_SORT=global) in place of the per-bin one."""
    _run_and_check(name, monkeypatch, split_below, "2", depth_sort="global")
