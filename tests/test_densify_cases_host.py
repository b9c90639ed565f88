"""The classify table of tests/densify_cases.py: every row is exactly on a threshold by construction or MARGIN away from all of
them, every branch of the decision is reached, and the expected flags agree with the numpy oracle of the whole densification where
the two overlap (which rows survive)."""
import numpy as np
import pytest

import densify_cases as dc

CALLS = dc.calls()


@pytest.mark.parametrize("call", [c for _, c in CALLS], ids=[t for t, _ in CALLS])
def test_rows_are_on_a_threshold_exactly_or_a_margin_away(call):
    t = dc.table(call, len(dc._ROWS))
    d, names = dc.distances(call, t)
    bad = (d != 0) & (d < dc.MARGIN)
    assert not bad.any(), [(int(r), names[k], d[r, k]) for r, k in zip(*np.nonzero(bad))]
    # a row that is exactly on a threshold is so through exact fp32 inputs, not through a transcendental that happens to round there
    on = d == 0
    for r, k in zip(*np.nonzero(on)):
        if names[k].startswith("g "):
            assert t["denom"][r, 0] == 1.0 and float(t["xyz_gradient_accum"][r, 0]) == call["max_grad"]
        elif names[k].startswith("smax"):
            assert t["scaling_raw"][r].max() == 0.0 and (call["percent_dense"] * call["extent"] == 1.0 or 0.1 * call["extent"] == 1.0)
        elif names[k].startswith("radius"):
            assert float(t["max_radii2D"][r]) == call["max_screen_size"]
        else:
            raise AssertionError("row %d is exactly on '%s'" % (r, names[k]))
    # ... and such rows exist: on max_grad always, on the limit that is 1.0, on max_screen_size where there is one
    assert on[:, names.index("g vs max_grad")].any()
    if call["percent_dense"] * call["extent"] == 1.0:
        assert on[:, names.index("smax vs small")].any()
    if call["max_screen_size"]:
        assert on[:, names.index("radius vs screen")].any()
        assert on[:, names.index("smax vs big")].any() == (0.1 * call["extent"] == 1.0)


def test_every_branch_is_reached_and_p_sizes_repeat_the_table():
    seen = set()
    both_ways = {"parent_not_child": False, "child_not_parent": False}
    for _, call in CALLS:
        t = dc.table(call, len(dc._ROWS))
        f = dc.expected_flags(call, t)
        seen |= set(int(x) for x in f)
        split = (f & dc.SPLIT) != 0
        both_ways["child_not_parent"] |= bool((split & ((f & dc.PRUNE) == 0) & ((f & dc.PRUNE_CHILD) != 0)).any())
        both_ways["parent_not_child"] |= bool((split & ((f & dc.PRUNE) != 0) & ((f & dc.PRUNE_CHILD) == 0)).any())
        if call["prune_only"]:
            assert not (f & (dc.CLONE | dc.SPLIT)).any()
        if not call["max_screen_size"]:
            assert np.array_equal((f & dc.PRUNE) != 0, (f & dc.PRUNE_CHILD) != 0)     # opacity alone decides both
        for P in dc.P_SIZES:
            tp = dc.table(call, P)
            assert tp["scaling_raw"].shape == (P, 3) and tp["max_radii2D"].shape == (P,)
            assert np.array_equal(dc.expected_flags(call, tp), np.resize(f, P))
    assert all(both_ways.values()), both_ways
    assert {0, dc.CLONE, dc.SPLIT, dc.PRUNE | dc.PRUNE_CHILD, dc.PRUNE, dc.PRUNE_CHILD, dc.SPLIT | dc.PRUNE, dc.SPLIT | dc.PRUNE_CHILD,
            dc.SPLIT | dc.PRUNE | dc.PRUNE_CHILD, dc.CLONE | dc.PRUNE | dc.PRUNE_CHILD} <= seen, sorted(seen)
    assert not any(x & dc.CLONE and x & dc.SPLIT for x in seen)


@pytest.mark.parametrize("call", [c for t, c in CALLS if "-N2" in t], ids=[t for t, _ in CALLS if "-N2" in t])
def test_flags_predict_what_the_densification_oracle_keeps(call):
    """Independent restatements meet: the number of Gaussians oracle/densify_oracle.py leaves equals the count the flags give --
    kept originals + clones + N children per split parent whose children survive."""
    import util  # noqa: F401
    from oracle import densify_oracle as do
    P = len(dc._ROWS)
    t = dc.table(call, P)
    f = dc.expected_flags(call, t)
    rng = np.random.default_rng(0)
    params = {"_xyz": rng.standard_normal((P, 3)), "_features": rng.standard_normal((P, 1, 3)), "_opacity": t["opacity_raw"],
              "_scaling": t["scaling_raw"], "_rotation": rng.standard_normal((P, 4))}
    params = {k: v.astype(np.float32) for k, v in params.items()}
    z = {k: np.zeros_like(v) for k, v in params.items()}
    st = {"params": params, "exp_avg": z, "exp_avg_sq": {k: v.copy() for k, v in z.items()},
          "xyz_gradient_accum": t["xyz_gradient_accum"], "denom": t["denom"], "max_radii2D": t["max_radii2D"]}
    k = int(((f & dc.SPLIT) != 0).sum())
    out = do.densify_and_prune(st, call["max_grad"], call["min_opacity"], call["extent"], call["max_screen_size"],
                               prune_only=call["prune_only"], percent_dense=call["percent_dense"], N=call["N"], rot_4d=False, gaussian_dim=3,
                               samples=np.zeros((k * call["N"], 3), np.float32))
    pruned = (f & dc.PRUNE) != 0
    kept = int((((f & dc.SPLIT) == 0) & ~pruned).sum())
    clones = int((((f & dc.CLONE) != 0) & ~pruned).sum())
    children = call["N"] * int((((f & dc.SPLIT) != 0) & ((f & dc.PRUNE_CHILD) == 0)).sum())
    assert out["params"]["_xyz"].shape[0] == kept + clones + children
