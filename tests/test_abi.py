"""CPU tests of the drop-in boundary (no GPU needed).

* libwgsr.so loads and exports every function include/wgsr.h declares.
* The Python surface matches the upstream contract the reference calls
  (gaussian_renderer/__init__.py:15-18, 58-74, 130-141; gaussian_model.py:18).
"""
import json
import os
import re

import pytest
import torch

from _util import GOLDEN  # noqa: F401  (sets up sys.path via conftest)

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def header_functions():
    src = open(os.path.join(ROOT, "include", "wgsr.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(wgsr_\w+)\s*\(", src)))


def test_library_exports_every_header_symbol():
    from wgsr import _lib
    L = _lib.load()
    names = header_functions()
    assert "wgsr_rasterize_forward" in names and "wgsr_dist_cuda2" in names
    for n in names:
        assert hasattr(L, n), n
    assert set(_lib.EXPORTED_SYMBOLS) == set(names)
    assert L.wgsr_version().startswith(b"wgsr")


def test_state_buffer_sizes_scale():
    from wgsr import _lib
    L = _lib.load()
    assert L.wgsr_geometry_bytes(0) >= 0
    g1, g2 = L.wgsr_geometry_bytes(1000), L.wgsr_geometry_bytes(2000)
    assert g2 > g1 and g1 >= 48 * 1000
    assert L.wgsr_image_bytes(1920, 1080) >= 8 * 1920 * 1080
    assert L.wgsr_binning_bytes(10_000, 64, 64) >= 16 * 10_000


def test_settings_tuple_is_upstream():
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    assert GaussianRasterizationSettings._fields == (
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier",
        "viewmatrix", "projmatrix", "projmatrix_raw", "sh_degree", "campos", "prefiltered",
        "debug")


def _settings():
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    e = torch.eye(4)
    return GaussianRasterizationSettings(8, 8, 1.0, 1.0, torch.zeros(3), 1.0, e, e, e, 0,
                                         torch.zeros(3), False, False)


def test_argument_misuse_raises_upstream_exceptions():
    from diff_gaussian_rasterization import GaussianRasterizer
    r = GaussianRasterizer(_settings())
    m = torch.zeros(2, 3)
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        r(means3D=m, means2D=m, opacities=torch.ones(2, 1), scales=m, rotations=torch.zeros(2, 4))
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        r(means3D=m, means2D=m, opacities=torch.ones(2, 1), shs=torch.zeros(2, 1, 3),
          colors_precomp=m, scales=m, rotations=torch.zeros(2, 4))
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(means3D=m, means2D=m, opacities=torch.ones(2, 1), shs=torch.zeros(2, 1, 3), scales=m)
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(means3D=m, means2D=m, opacities=torch.ones(2, 1), shs=torch.zeros(2, 1, 3), scales=m,
          rotations=torch.zeros(2, 4), cov3D_precomp=torch.zeros(2, 6))


def test_bad_means_shape_raises_runtime_error():
    from diff_gaussian_rasterization import _C
    with pytest.raises(RuntimeError, match=r"means3D must have dimensions \(num_points, 3\)"):
        _C.rasterize_gaussians(torch.zeros(3), torch.zeros(4, 2), torch.empty(0), torch.zeros(4, 1),
                               torch.zeros(4, 3), torch.zeros(4, 4), 1.0, torch.empty(0),
                               torch.eye(4), torch.eye(4), torch.eye(4), 1.0, 1.0, 8, 8,
                               torch.empty(0), 0, torch.zeros(3), False, False)


def test_host_tensors_are_rejected_before_any_launch():
    """A host pointer reaching a kernel would fault the GPU: the boundary
    raises RuntimeError instead (upstream's .data<T>() raises too)."""
    from diff_gaussian_rasterization import _C
    from simple_knn._C import distCUDA2
    with pytest.raises(RuntimeError, match="HIP device"):
        _C.rasterize_gaussians(torch.zeros(3), torch.zeros(4, 3), torch.empty(0), torch.zeros(4, 1),
                               torch.zeros(4, 3), torch.zeros(4, 4), 1.0, torch.empty(0),
                               torch.eye(4), torch.eye(4), torch.eye(4), 1.0, 1.0, 8, 8,
                               torch.zeros(4, 1, 3), 0, torch.zeros(3), False, False)
    with pytest.raises(RuntimeError, match="HIP device"):
        _C.mark_visible(torch.zeros(4, 3), torch.eye(4), torch.eye(4))
    with pytest.raises(RuntimeError, match="HIP device"):
        distCUDA2(torch.zeros(4, 3))


def test_simple_knn_module_surface():
    from simple_knn._C import distCUDA2
    assert callable(distCUDA2)
    with pytest.raises(RuntimeError, match="num_points, 3"):
        distCUDA2(torch.zeros(4, 2))


def test_reference_render_imports_this_package_unchanged():
    """The reference render() module resolves ``diff_gaussian_rasterization``
    to this package.  The names it uses of that package (its import, the
    fields it gives the settings, the keywords of its rasterizer call) are
    recorded in tests/golden/ref_render_call.json
    (tests/golden/make_text_fixtures.py)."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_render_call.json")) as f:
        rec = json.load(f)
    import diff_gaussian_rasterization as dgr
    assert set(rec["imports"]) == {"GaussianRasterizationSettings", "GaussianRasterizer"}
    for name in rec["imports"]:
        assert hasattr(dgr, name)
    # every keyword the reference passes is accepted by our rasterizer
    import inspect
    params = set(inspect.signature(dgr.GaussianRasterizer.forward).parameters)
    kws = set(rec["rasterizer_keywords"])
    assert kws and kws <= params, kws - params
    fields = set(rec["settings_fields"])
    assert fields == set(dgr.GaussianRasterizationSettings._fields)
