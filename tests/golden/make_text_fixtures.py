"""Generate the fixtures of the two tests that pin this project to reference
TEXT (not to reference output), so that the tests themselves need no
reference checkout:

* tests/golden/ref_render_call.json -- the names the reference's render()
  module (thirdparty/gaussian_splatting/gaussian_renderer/__init__.py) uses of
  ``diff_gaussian_rasterization``: what it imports, the fields it gives
  ``GaussianRasterizationSettings`` and the keywords of its rasterizer call
  (tests/test_abi.py);
* tests/golden/ref_shader_facts.json -- for the viewer's shaders
  (src/gui/gl_render/shaders/gau_vert.glsl, gau_frag.glsl): which of the
  statements listed in tests/test_shader_crosscheck.py (STATEMENTS) occur in
  them, whitespace removed, the values of their SH_C* defines, and the sha256
  of the two files the record was taken from.

Both files hold names, numbers and true / false only.

Usage:  python tests/golden/make_text_fixtures.py <reference checkout>
"""
import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [TESTS, os.path.dirname(TESTS)]  # test_shader_crosscheck and what it imports


def render_call(ref):
    src = open(os.path.join(ref, "thirdparty/gaussian_splatting/gaussian_renderer/__init__.py")).read()
    imp = src[src.index("from diff_gaussian_rasterization import ("):]
    imports = re.findall(r"(\w+),", imp[: imp.index(")\n")])
    call = src[src.index("rendered_image, radii, depth, opacity, n_touched = rasterizer("):]
    call = call[: call.index(")\n")]
    fields = re.findall(r"^\s+(\w+)=", src[src.index("GaussianRasterizationSettings(\n"):
                                           src.index("rasterizer = GaussianRasterizer")], re.M)
    return {"imports": imports, "settings_fields": fields, "rasterizer_keywords": re.findall(r"(\w+)=", call)}


def shader_facts(ref):
    from test_shader_crosscheck import STATEMENTS, _nows
    out = {"sha256": {}, "statements": {}}
    for name, wanted in STATEMENTS.items():
        text = open(os.path.join(ref, "src/gui/gl_render/shaders", name)).read()
        out["sha256"][name] = hashlib.sha256(text.encode()).hexdigest()
        out["statements"][name] = {k: s in _nows(text) for k, s in wanted.items()}
        if name == "gau_vert.glsl":
            out["defines"] = dict(re.findall(r"#define\s+(SH_C\d(?:_\d)?)\s+(-?[0-9.]+)f", text))
    return out


def main():
    ref = sys.argv[1]
    for name, rec in (("ref_render_call.json", render_call(ref)), ("ref_shader_facts.json", shader_facts(ref))):
        with open(os.path.join(HERE, name), "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", name)


if __name__ == "__main__":
    main()
