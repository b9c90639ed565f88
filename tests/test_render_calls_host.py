"""CPU: the layer between the user and the native binding (render, render_raw, importance._forward and the autograd functions under
them) hands ``_C.rasterize_gaussians`` / ``_C.rasterize_gaussians_backward`` what it handed them before its copies were folded into
one settings builder, one raw-tensor rule, one assembly of each argument tuple and one raw autograd function, and sends every
gradient where it went (tests/golden/render_calls.json, recorded by tests/golden/make_golden_render_calls.py from the cases in
tests/render_call_cases.py).  Not reachable without a GPU, so left to the GPU suite: render()'s fast path and the binding below ``_scene``."""
import json
import os
import re

import pytest

import render_call_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "4d-gaussian-splatting_amd")


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "render_calls.json")) as f:
        return json.load(f)


def test_the_recorded_cases_are_the_cases():
    table = _golden()
    assert list(table) == render_call_cases.cases() and len(table) == 33
    assert not any("raised" in v for v in table.values())
    assert sum(len(v["calls"]) for v in table.values()) == 60   # a forward and a backward each; importance: the forward only


@pytest.mark.parametrize("case", render_call_cases.cases())
def test_render_calls_did_not_move(case, monkeypatch):
    want = _golden()[case]
    got = json.loads(json.dumps(render_call_cases.run(case, monkeypatch.setattr)))
    assert got.get("raised") == want.get("raised")
    assert len(got["calls"]) == len(want["calls"])
    for g, w in zip(got["calls"], want["calls"]):
        assert g["fn"] == w["fn"]
        assert len(g["args"]) == len(w["args"]) == (30 if g["fn"] == "rasterize_gaussians" else 37)
        for i, (ga, wa) in enumerate(zip(g["args"], w["args"])):
            assert ga == wa, "%s: positional argument %d" % (g["fn"], i)
        assert g["kwargs"] == w["kwargs"], g["fn"]
    # the first element of every gradient: which of the 12 results reached the parameter, through which activation
    for key in ("grads", "sink"):
        assert (key in got) == (key in want)
        for name, w in want.get(key, {}).items():
            g = got[key][name]
            print(case, key, name, g, w)
            assert (g is None) == (w is None), name
            assert w is None or g == pytest.approx(w, rel=1e-5, abs=1e-7), name


def _sources():
    for d, _, fs in os.walk(PKG):
        for f in fs:
            if f.endswith(".py"):
                with open(os.path.join(d, f)) as fh:
                    yield os.path.relpath(os.path.join(d, f), PKG), fh.read()


def test_one_settings_builder_and_the_merged_names_are_gone():
    """GaussianRasterizationSettings is constructed by ``view_settings`` and by slice.py (from a slice, not a model) only; the second
    raw autograd function and the private phase keyword of the backward are gone."""
    built = {}
    for path, text in _sources():
        assert "_RasterizeModel" not in text and "_raw_forward_args" not in text and not re.search(r"\b_phase\b", text), path
        n = len(re.findall(r"GaussianRasterizationSettings\(\s*(?!NamedTuple)", text))
        if n:
            built[path] = n
    assert built == {os.path.join("gaussian_renderer", "diff_gaussian_rasterization.py"): 1, "slice.py": 1}
    with open(os.path.join(PKG, "gaussian_renderer", "diff_gaussian_rasterization.py")) as f:
        text = f.read()
    body = text[text.index("def view_settings("):text.index("def time_inputs(")]
    assert "GaussianRasterizationSettings(" in body
