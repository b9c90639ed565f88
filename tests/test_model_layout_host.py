"""CPU: the flat bucket is stated once (fdgs.layout) and still says what it said before it was: every derived table against
tests/golden/model_layout.json (recorded by tests/golden/make_golden_model_layout.py from the commit before fdgs.layout existed), two facts
about the source, and train_host.relayout against plain indexing."""
import glob
import json
import os
import re

import pytest
import torch

import model_layout_cases
from fdgs import harness, importance, layout, synth, train_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "4d-gaussian-splatting_amd")
with open(os.path.join(ROOT, "tests", "golden", "model_layout.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def recorded():
    return json.loads(json.dumps(model_layout_cases.record()))


def test_the_record_covers_the_three_modes():
    assert sorted(GOLDEN["modes"]) == sorted(model_layout_cases.MODES) and [GOLDEN["modes"][m]["M"] for m in model_layout_cases.MODES] == [1, 16, 48]


def test_compress_segments_are_the_recorded_ones(recorded):
    assert recorded["compress.SEGMENTS"] == GOLDEN["compress.SEGMENTS"]


@pytest.mark.parametrize("mode", list(model_layout_cases.MODES))
def test_every_derived_table_is_the_recorded_one(recorded, mode):
    got, want = recorded["modes"][mode], GOLDEN["modes"][mode]
    assert sorted(got) == sorted(want)
    for entry in want:
        assert got[entry] == want[entry], (mode, entry)


def test_layout_tables_agree_with_the_model():
    m = train_host.GaussianParams(synth.make_scene(model_layout_cases.MODES["rot4d_M48"], seed=0), torch.device("cpu"))
    assert m.NAMES == layout.NAMES and layout.NAMES[-1] == "_features"
    assert {n: tuple(p.shape) for n, p in m.params.items()} == layout.shapes(m.P, m.M) and m.row_floats() == layout.row_floats(m.M)
    for n in m.NAMES:
        assert layout.segment(m.flat_grad, m, n).data_ptr() == m.params[n].grad.data_ptr()
        assert layout.BY_KERNEL[layout.BY_NAME[n].kernel].name == n and all(layout.BY_GROUP[g].name == n for g in layout.BY_NAME[n].groups)
    assert layout.used(3, False) == ("_xyz", "_opacity", "_scaling", "_rotation", "_features")
    assert layout.used(4, False) == layout.NAMES[:6] + ("_features",) and layout.used(4, True) == layout.NAMES
    assert m.settings() == layout.settings_of(m) and sorted(m.settings()) == sorted(layout.SETTINGS)
    copy = train_host.GaussianParams.from_raw(layout.raw_of(m), torch.device("cpu"), **m.settings())
    assert torch.equal(copy.flat, m.flat) and copy.settings() == m.settings()


def _package_sources():
    return sorted(glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True))


def test_one_segment_name_is_spelled_out_in_the_table_only():
    """Adding a segment must not mean finding its name by grep: the last one added is a string literal in fdgs.layout, where a call
    passes that one tensor to a kernel (densify's split call; the render path's check that the model has it), and in the compression
    policy tables that stay in compress.py (DEFAULT_BITS, _QUATERNIONS) -- nowhere else."""
    literal = re.compile(r"""["']_rotation_r["']""")
    found = {}
    for path in _package_sources():
        with open(path) as f:
            n = len(literal.findall(f.read()))
        if n:
            found[os.path.relpath(path, PKG)] = n
    allowed = {"layout.py": 1, "densify.py": 1, "pipeline.py": 2, "loss.py": 1, os.path.join("gaussian_renderer", "__init__.py"): 1, "compress.py": 2}
    assert "layout.py" in found
    assert all(found[p] <= allowed.get(p, 0) for p in found), found


def test_an_empty_bucket_is_made_in_one_place():
    needles = ("GaussianParams.__new__", "__new__(GaussianParams")
    me = os.path.abspath(__file__)
    paths = _package_sources() + [p for d in ("tests", "examples", "tools") for p in glob.glob(os.path.join(ROOT, d, "**", "*.py"), recursive=True)]
    paths.append(os.path.join(ROOT, "bench.py"))
    hits = []
    for path in paths:
        if os.path.abspath(path) in (me, os.path.join(PKG, "train_host.py")):
            continue
        with open(path) as f:
            text = f.read()
        hits += [os.path.relpath(path, ROOT) for needle in needles if needle in text]
    assert hits == []


SRC = [6, 0, 0, 3]


def _model(P=7):
    scene = synth.make_scene(synth.SceneConfig("r", P, 32, 32, 3, 2, 0.05, 10.0, True, 4, False), seed=3)
    m = train_host.GaussianParams(scene, torch.device("cpu"))
    o = train_host.FlatAdam(m)
    g = torch.Generator().manual_seed(5)
    o.exp_avg.copy_(torch.randn(m.flat.numel(), generator=g))
    o.exp_avg_sq.copy_(torch.rand(m.flat.numel(), generator=g))
    o.set_lr("_xyz", 3e-5)
    o.step_count = 4
    return m, o


@pytest.mark.parametrize("kind", [None, [0, 0, 0, 0], [0, 1, 2, 0]])
@pytest.mark.parametrize("with_optimizer", [True, False])
def test_relayout_against_plain_indexing(kind, with_optimizer):
    """P = 7 -> rows [6, 0, 0, 3]: every parameter row is the old row src[j]; the moments are carried where kind is 0 (or None) and
    start at zero for kinds 1 and 2, as fdgs_densify_gather documents; the statistics follow; the optimizer keeps its rates."""
    m, o = _model()
    src = torch.tensor(SRC)
    before = {n: m.params[n].detach().clone() for n in m.NAMES}
    moments = {n: (layout.segment(o.exp_avg, m, n).clone(), layout.segment(o.exp_avg_sq, m, n).clone()) for n in m.NAMES}
    dens, contrib = harness.DensificationStats(m.P, torch.device("cpu")), importance.ContributionStats(m.P, torch.device("cpu"))
    dens.xyz_gradient_accum.copy_(torch.arange(7.0).reshape(7, 1))
    dens.t_gradient_accum.copy_(torch.arange(7.0).reshape(7, 1) * 2)
    dens.denom.copy_(torch.arange(7.0).reshape(7, 1) + 1)
    dens.max_radii2D.copy_(torch.arange(7.0) * 3)
    contrib.weight_sum.copy_(torch.arange(7.0))
    old_flat = m.flat
    old = train_host.relayout(m, o if with_optimizer else None, src, None if kind is None else torch.tensor(kind, dtype=torch.uint8),
                              stats=(dens, contrib))
    assert m.P == 4 and m.flat is not old_flat and m.flat.numel() == m.flat_grad.numel() == 4 * m.floats_per_gaussian()
    assert not bool(m.flat_grad.any())
    for n in m.NAMES:
        assert torch.equal(m.params[n].detach(), before[n][src]), n
        assert torch.equal(old[n].detach(), before[n]), n                      # the old views stay alive and untouched
        assert m.params[n].grad.data_ptr() == layout.segment(m.flat_grad, m, n).data_ptr()
        if with_optimizer:
            keep = torch.ones(4, dtype=torch.bool) if kind is None else torch.tensor(kind) == 0
            for got, was in zip((layout.segment(o.exp_avg, m, n), layout.segment(o.exp_avg_sq, m, n)), moments[n]):
                assert torch.equal(got[keep], was[src][keep]), n
                assert not bool(got[~keep].any()), n
    if with_optimizer:
        assert o.exp_avg.numel() == m.flat.numel() and o.step_count == 4
        seg = {s["name"]: s for s in o.named_segments()}
        assert seg["_xyz"]["lr"] == 3e-5 and all(tuple(m.offsets[k]) == (s["begin"], s["end"]) for k, s in seg.items())
    assert torch.equal(dens.xyz_gradient_accum[:, 0], src.float()) and torch.equal(dens.t_gradient_accum[:, 0], src.float() * 2)
    assert torch.equal(dens.denom[:, 0], src.float() + 1) and torch.equal(dens.max_radii2D, src.float() * 3)
    assert contrib.P == 4 and torch.equal(contrib.weight_sum, src.float())
    dens.reset_(4)
    assert dens.denom.shape == (4, 1) and dens.max_radii2D.shape == (4,) and not bool(dens.xyz_gradient_accum.any())
