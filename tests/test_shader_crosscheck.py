"""Cross-check of the oracle against the only reference-held text of the
rasteriser's math ("Next round" item 6).

The upstream CUDA rasteriser is absent (empty submodule, .gitmodules:7-12),
but the reference's OpenGL viewer carries the same preprocess / fragment math
as GLSL:

* ``src/gui/gl_render/shaders/gau_vert.glsl:60-80``  computeCov3D
  (Sigma = (S R)^T (S R), quaternion (r, x, y, z));
* ``gau_vert.glsl:82-107``  computeCov2D (frustum clamp at 1.3 tan(fov),
  J, ``W = transpose(mat3(viewmatrix))``, ``T = W * J``,
  ``cov = T^T Sigma^T T``, +0.3 low-pass on the diagonal);
* ``gau_vert.glsl:148-154``  det, conic = (c, -b, a) / det;
* ``gau_vert.glsl:3-18, 174-211``  the SH basis constants and evaluation
  (+0.5; the viewer does not clamp);
* ``gau_frag.glsl:20-25``  power = -1/2 (cx dx^2 + cz dy^2) - cy dx dy,
  discard if power > 0, alpha = min(0.99, o exp(power)), discard if
  alpha < 1/255.

What those files say is recorded in tests/golden/ref_shader_facts.json
(tests/golden/make_text_fixtures.py, run against a reference checkout: which
of the STATEMENTS below occur in each shader, whitespace removed, and the
values of the SH_C* defines), so the test needs no reference checkout.  It
asserts the constants oracle/dense.py uses, and evaluates a line-for-line
numpy transcription of the GLSL functions -- with GLSL's column-major ``mat3``
semantics -- against dense.py's preprocess on every golden scene.  It pins
the oracle to reference TEXT, not to reference output: parity with the CUDA
binary stays "partial" (DESIGN.md section 4).
"""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from _util import load_scene, scene_names
from oracle import dense

FACTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_shader_facts.json")

# the statements the oracle's constants and formulas rest on, per shader file
STATEMENTS = {
    "gau_vert.glsl": {
        "limx": "floatlimx=1.3f*tan_fovx;",
        "limy": "floatlimy=1.3f*tan_fovy;",
        "lowpass_x": "cov[0][0]+=0.3f;",
        "lowpass_y": "cov[1][1]+=0.3f;",
        "M": "mat3M=S*R;",
        "Sigma": "mat3Sigma=transpose(M)*M;",
        "W": "mat3W=transpose(mat3(viewmatrix));",
        "T": "mat3T=W*J;",
        "cov": "mat3cov=transpose(T)*transpose(cov3D)*T;",
        "conic": "conic=vec3(cov2d.z*det_inv,-cov2d.y*det_inv,cov2d.x*det_inv);",
        # the 3-sigma quad of the viewer (the rasteriser's radius is 3 sqrt(lambda_max))
        "quad": "3.f*sqrt(cov2d.x)",
    },
    "gau_frag.glsl": {
        "power": "floatpower=-0.5f*(conic.x*coordxy.x*coordxy.x+conic.z*coordxy.y*coordxy.y)-conic.y*coordxy.x*coordxy.y;",
        "discard_power": "if(power>0.f)discard;",
        "alpha": "floatopacity=min(0.99f,alpha*exp(power));",
        "discard_alpha": "if(opacity<1.f/255.f)discard;",
    },
}


def _nows(s):
    return re.sub(r"\s+", "", s)


# ---- GLSL semantics -----------------------------------------------------------
def mat3(*v):
    """GLSL mat3(c0..c8): the arguments fill COLUMNS; returned as [row, col]."""
    return np.asarray(v, np.float64).reshape(3, 3).T


def compute_cov3d(scale, q):
    """gau_vert.glsl:60-80, line for line (S[i][i] = column i, row i)."""
    S = np.zeros((3, 3))
    S[0, 0], S[1, 1], S[2, 2] = scale
    r, x, y, z = q
    R = mat3(1. - 2. * (y * y + z * z), 2. * (x * y - r * z), 2. * (x * z + r * y),
             2. * (x * y + r * z), 1. - 2. * (x * x + z * z), 2. * (y * z - r * x),
             2. * (x * z - r * y), 2. * (y * z + r * x), 1. - 2. * (x * x + y * y))
    M = S @ R
    return M.T @ M


def compute_cov2d(mean_view, focal_x, focal_y, tan_fovx, tan_fovy, cov3D, viewmatrix_gl):
    """gau_vert.glsl:82-107, line for line.  viewmatrix_gl: the GLSL uniform
    as a [row, col] matrix (= W2C for the rasteriser's row-vector storage)."""
    t = np.array(mean_view, np.float64)
    limx = 1.3 * tan_fovx
    limy = 1.3 * tan_fovy
    txtz = t[0] / t[2]
    tytz = t[1] / t[2]
    t[0] = min(limx, max(-limx, txtz)) * t[2]
    t[1] = min(limy, max(-limy, tytz)) * t[2]
    J = mat3(focal_x / t[2], 0.0, -(focal_x * t[0]) / (t[2] * t[2]),
             0.0, focal_y / t[2], -(focal_y * t[1]) / (t[2] * t[2]),
             0, 0, 0)
    W = viewmatrix_gl[:3, :3].T                    # transpose(mat3(viewmatrix))
    T = W @ J
    cov = T.T @ cov3D.T @ T
    # cov[0][0] += 0.3 etc.: column 0 row 0 / column 1 row 1; the vec3 returned
    # is (cov[0][0], cov[0][1], cov[1][1]) = ([0,0], [1,0], [1,1]) as [row, col]
    cov[0, 0] += 0.3
    cov[1, 1] += 0.3
    return np.array([cov[0, 0], cov[1, 0], cov[1, 1]])


def conic_of(cov2d):
    """gau_vert.glsl:148-154."""
    det = cov2d[0] * cov2d[2] - cov2d[1] * cov2d[1]
    det_inv = 1.0 / det
    return np.array([cov2d[2] * det_inv, -cov2d[1] * det_inv, cov2d[0] * det_inv]), det


def frag_alpha(conic, dx, dy, opacity):
    """gau_frag.glsl:20-25: alpha, or None where the fragment is discarded."""
    power = -0.5 * (conic[0] * dx * dx + conic[2] * dy * dy) - conic[1] * dx * dy
    if power > 0.0:
        return None
    a = min(0.99, opacity * math.exp(power))
    if a < 1.0 / 255.0:
        return None
    return a


# ---- the constants ---------------------------------------------------------------
def test_shader_constants_are_the_oracles():
    with open(FACTS) as fh:
        facts = json.load(fh)
    # every statement above was looked for in its shader, and found
    for name, wanted in STATEMENTS.items():
        found = facts["statements"][name]
        assert set(found) == set(wanted), name
        assert all(found.values()), (name, [k for k, ok in found.items() if not ok])
    # SH basis: every #define equals the oracle's constant
    defs = facts["defines"]
    assert float(defs["SH_C0"]) == dense.SH_C0 and float(defs["SH_C1"]) == dense.SH_C1
    for i in range(5):
        assert float(defs[f"SH_C2_{i}"]) == dense.SH_C2[i]
    for i in range(7):
        assert float(defs[f"SH_C3_{i}"]) == dense.SH_C3[i]
    # the oracle's own thresholds
    src = open(dense.__file__).read()
    assert "1.3 * tanfovx" in src and "1.3 * tanfovy" in src
    assert "cov2[:, 0, 0] + 0.3" in src and "cov2[:, 1, 1] + 0.3" in src
    assert "0.99" in src and "1.0 / 255.0" in src and "(power <= 0)" in src
    assert "torch.ceil(3.0 * torch.sqrt(lam))" in src


# ---- the functions, evaluated ----------------------------------------------------
def _sh_glsl(deg, sh, d):
    """gau_vert.glsl:174-211 (the viewer's SH colour before its +0.5)."""
    x, y, z = d
    c = dense.SH_C0 * sh[0]
    if deg > 0:
        c = c - dense.SH_C1 * y * sh[1] + dense.SH_C1 * z * sh[2] - dense.SH_C1 * x * sh[3]
        if deg > 1:
            xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
            C2 = dense.SH_C2
            c = (c + C2[0] * xy * sh[4] + C2[1] * yz * sh[5] + C2[2] * (2.0 * zz - xx - yy) * sh[6]
                 + C2[3] * xz * sh[7] + C2[4] * (xx - yy) * sh[8])
            if deg > 2:
                C3 = dense.SH_C3
                c = (c + C3[0] * y * (3.0 * xx - yy) * sh[9] + C3[1] * xy * z * sh[10]
                     + C3[2] * y * (4.0 * zz - xx - yy) * sh[11] + C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy) * sh[12]
                     + C3[4] * x * (4.0 * zz - xx - yy) * sh[13] + C3[5] * z * (xx - yy) * sh[14]
                     + C3[6] * x * (xx - 3.0 * yy) * sh[15])
    return c + 0.5


@pytest.mark.parametrize("name", scene_names())
def test_shader_transcription_matches_dense_preprocess(name):
    inputs, settings, expect, grads = load_scene(name)
    if inputs.get("cov3D_precomp") is not None and inputs["cov3D_precomp"].numel() > 0:
        pytest.skip("precomputed covariances: computeCov3D is not on this path")
    res = dense.dense_forward_backward(inputs, settings, *grads)
    vis = res["visible"].numpy()
    if not vis.any():
        pytest.skip("nothing visible")
    W, H = settings["W"], settings["H"]
    tx, ty = settings["tanfovx"], settings["tanfovy"]
    fx, fy = W / (2.0 * tx), H / (2.0 * ty)
    V = settings["viewmatrix"].double().numpy().T          # row-vector storage -> W2C
    means = inputs["means3D"].double().numpy()
    scales = inputs["scales"].double().numpy() * settings["scale_modifier"]
    rots = inputs["rotations"].double().numpy()
    opac = inputs["opacities"].double().numpy()[:, 0]
    cov_o, con_o, xy_o = res["cov2d"].numpy(), res["conic"].numpy(), res["xy"].numpy()
    rng = np.random.default_rng(0)
    n_alpha = 0
    for i in np.nonzero(vis)[0]:
        mv = V @ np.append(means[i], 1.0)
        cov2 = compute_cov2d(mv, fx, fy, tx, ty, compute_cov3d(scales[i], rots[i]), V)
        np.testing.assert_allclose(cov2, cov_o[i], rtol=1e-10, atol=1e-12 * abs(cov2).max())
        con, det = conic_of(cov2)
        assert det != 0
        np.testing.assert_allclose(con, con_o[i], rtol=1e-9, atol=1e-12 * abs(con).max())
        # fragment rule vs the oracle's per-pixel alpha at a few pixel offsets
        for _ in range(4):
            dx, dy = rng.normal(0.0, 2.0 / math.sqrt(max(con[0], 1e-12)), 2)
            a = frag_alpha(con, dx, dy, opac[i])
            power = -0.5 * (con_o[i, 0] * dx * dx + con_o[i, 2] * dy * dy) - con_o[i, 1] * dx * dy
            araw = opac[i] * math.exp(power)
            valid = power <= 0 and min(araw, 0.99) >= 1.0 / 255.0
            assert (a is not None) == valid
            if a is not None:
                assert abs(a - min(araw, 0.99)) <= 1e-12
                n_alpha += 1
    assert n_alpha > 0
    # SH colour (the viewer's formula; dense clamps at 0 like upstream)
    if inputs.get("shs") is not None and inputs["shs"].numel() > 0:
        deg = settings["sh_degree"]
        sh = inputs["shs"].double().numpy()
        cam = settings["campos"].double().numpy()
        rgb_o = res["rgb"].numpy()
        for i in np.nonzero(vis)[0][:200]:
            d = means[i] - cam
            d = d / np.linalg.norm(d)
            np.testing.assert_allclose(np.maximum(_sh_glsl(deg, sh[i], d), 0.0), rgb_o[i], rtol=1e-12, atol=1e-12)
