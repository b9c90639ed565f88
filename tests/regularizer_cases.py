"""The inputs the rigid / motion regulariser tests share: plain CPU data and builders, no GPU and no fdgs import, so that the host
proof of the bar (tests/test_regularizer_oracle_host.py) and the GPU tests (tests/test_gpu_regularizers.py) draw the same inputs.

A case is a Case: the six raw tensors of a rot_4d model (float32, CPU) and a neighbour table.
* MODEL cases: the table is the k-NN of the means (regularizer_oracle.knn here, fdgs.knn.knn on the GPU: bit-identical,
  tests/test_gpu_knn.py); they go through fdgs.loss.rigid_motion_loss.
* TABLE cases: a crafted table that no k-NN query returns, fed to the C entries directly; ``mask`` marks the entries the
  kernels skip (an index outside [0, P)).

Every case whose rigid term is alive (``rigid``) is built so that the term it tests cannot silently vanish, asserted here on the
float64 oracle: the median pair weight exp(-100 d2) over the non-empty slots is >= 0.01 (the means sit in a compact box), and
L_rigid carries >= 10 % of each tensor's gradient norm at (g_rigid, g_motion) = (1, 1).  The other cases are those where L_rigid
is 0 by construction (P = 1, k = 1 or a table of self entries: every pair is (i, i); ``initial``: every velocity is 0)."""
import functools

import numpy as np
import torch

import regularizer_oracle as ro

WEIGHTS = ((1.0, 0.0), (0.0, 1.0), (0.7, 0.3))
NAMES = ro.NAMES4 + ("_t", "_xyz")
MEDIAN_D2 = 0.012          # the median neighbour of a compact case weighs exp(-1.2) = 0.30
MEDIAN_D2_FEW = 0.0005     # P <= k: only P - 1 neighbours share the 1 / k, so they sit closer (weight 0.95) to keep L_rigid's share


class Case:
    def __init__(self, name, params, idx, d2, mask=None, rigid=True, zero=False):
        self.name, self.params, self.idx, self.d2, self.mask, self.rigid, self.zero = name, params, idx, d2, mask, rigid, zero
        self.P, self.k = int(idx.shape[0]), int(idx.shape[1])

    def __repr__(self):
        return self.name


def _raw(P, seed, kind):
    """The six raw tensors, drawn as the models of tests/test_gpu_regularizers.py::_model are (fdgs.synth.make_scene with its default
    rot_sigma, restated here in plain torch): quaternions normalize((1, 0, 0, 0) + 0.05 N) times a norm of 0.5 .. 2, scales
    0.05 exp(0.3 N), time extents sqrt(0.2) * 10 exp(0.3 N) with _scaling_t jittered by 0.3 N, t in [-1, 11]; the means in the unit
    box (_compact_means scales them)."""
    g = torch.Generator().manual_seed(1000 * seed + P)
    r = lambda *s: torch.rand(*s, generator=g)
    n = lambda *s: torch.randn(*s, generator=g)
    first = torch.tensor([1.0, 0.0, 0.0, 0.0])
    p = {"_xyz": r(P, 3),
         "_scaling": torch.log(0.05 * torch.exp(0.3 * n(P, 3))),
         "_scaling_t": torch.log(0.2 ** 0.5 * 10.0 * torch.exp(0.3 * n(P, 1))) + 0.3 * n(P, 1),
         "_rotation": torch.nn.functional.normalize(first + 0.05 * n(P, 4), dim=1) * (0.5 + 1.5 * r(P, 1)),
         "_rotation_r": torch.nn.functional.normalize(first + 0.05 * n(P, 4), dim=1) * (0.5 + 1.5 * r(P, 1)),
         "_t": (1.2 * r(P, 1) - 0.1) * 10.0}
    ident = torch.tensor([1.0, 0.0, 0.0, 0.0])
    if kind == "clones":         # a quarter are exact copies of the first quarter: zero velocity differences in both directions
        q = max(P // 4, 1)
        for t in p.values():
            t[P - q:] = t[:q]
    elif kind == "initial":      # the reference's initial state: v = 0 exactly for every Gaussian
        p["_rotation"][:] = ident
        p["_rotation_r"][:] = ident
    elif kind == "half_initial":
        p["_rotation"][::2] = ident
        p["_rotation_r"][::2] = ident
    elif kind == "late_t":       # (t + 0.1f) - t is not 0.1f here
        p["_t"] = torch.where(torch.arange(P)[:, None] % 2 == 0, 40.0 + 3.0 * r(P, 1), -3.0 - r(P, 1))
    elif kind == "thin_time":    # ct is tiny and the velocities are large
        p["_scaling_t"] = -8.0 + 7.0 * r(P, 1)
    elif kind != "compact":
        raise ValueError(kind)
    return {k: v.float().contiguous() for k, v in p.items()}


def _compact_means(p, k):
    """Scales the unit-box means so that the median d2 over the non-empty k-NN slots is MEDIAN_D2; returns the table."""
    xyz = p["_xyz"].numpy()
    _, d2 = ro.knn(xyz, xyz, k)
    live = d2[d2 < ro.EMPTY_D2]
    med = float(np.median(live))
    if med > 0:
        target = MEDIAN_D2 if p["_xyz"].shape[0] > k else MEDIAN_D2_FEW
        p["_xyz"] = (p["_xyz"] * float(np.sqrt(target / med))).contiguous()
    idx, d2 = ro.knn(p["_xyz"].numpy(), p["_xyz"].numpy(), k)
    return torch.from_numpy(idx), torch.from_numpy(d2)


def _norm_share(case):
    """L_rigid's share of each tensor's float64 gradient norm at (1, 1)."""
    both = ro.rigid_motion_with_grads(case.params, case.idx, case.d2, torch.float64, 1.0, 1.0, case.mask)[2]
    only = ro.rigid_motion_with_grads(case.params, case.idx, case.d2, torch.float64, 1.0, 0.0, case.mask)[2]
    return {n: float(only[n].norm() / both[n].norm()) for n in ro.NAMES4}


def _checked(case):
    lr, lm, g = ro.rigid_motion_with_grads(case.params, case.idx, case.d2, torch.float64, 1.0, 1.0, case.mask)
    assert np.isfinite([lr, lm]).all() and all(torch.isfinite(t).all() for t in g.values()), (case, "the float64 statement is not finite")
    if case.zero:
        assert lr == 0 and lm == 0 and all(float(t.abs().max()) == 0 for t in g.values()), (case, lr, lm)
    if not case.rigid:
        assert lr == 0, (case, lr)
        return case
    live = (case.d2 < ro.EMPTY_D2) if case.mask is None else ((case.d2 < ro.EMPTY_D2) & case.mask)
    med = float(torch.exp(-100 * case.d2[live].double()).median())
    assert med >= 0.01, (case, "median pair weight", med)
    share = _norm_share(case)
    assert min(share.values()) >= 0.10, (case, "share of L_rigid in the gradient norms", share)
    return case


def _model(kind, P, k, seed=3):
    p = _raw(P, seed, kind)
    idx, d2 = _compact_means(p, k)
    alive = P > 1 and k > 1 and kind != "initial"
    return Case("%s-P%d-k%d" % (kind, P, k), p, idx, d2, rigid=alive, zero=kind == "initial")


def _table(kind, P, k, seed=2):
    """Crafted tables; the raw tensors are those of the compact model of that size."""
    p = _raw(P, seed, "compact")
    idx, d2 = _compact_means(p, max(k, 2))
    idx, d2 = idx[:, :k].clone(), d2[:, :k].clone()
    g = torch.Generator().manual_seed(77 * P + k)
    mask, alive = None, True
    if kind == "hub":            # every row lists Gaussian 0: one reverse segment of P * k entries
        idx[:] = 0
        d2 = (0.03 * torch.rand(P, k, generator=g)).float()
    elif kind == "repeats":      # the same neighbour twice in a row, with its distance
        idx[:, 2], d2[:, 2] = idx[:, 3], d2[:, 3]
        idx[:, k - 1], d2[:, k - 1] = idx[:, 1], d2[:, 1]
    elif kind == "self_only":
        idx[:] = torch.arange(P)[:, None]
        d2[:] = 0
        alive = False
    elif kind == "foreign":      # about 10 % of the entries name no Gaussian
        bad = torch.tensor([-1, P, P + 7, 2 ** 40])
        hit = torch.rand(P, k, generator=g) < 0.10
        idx = torch.where(hit, bad[torch.randint(0, 4, (P, k), generator=g)], idx)
        mask = ro.valid_entries(idx, P)
        assert 0.05 < float((~mask).float().mean()) < 0.15 and all(bool((idx == b).any()) for b in bad)
    elif kind == "reversed":     # rows in descending distance order
        idx, d2 = idx.flip(1).contiguous(), d2.flip(1).contiguous()
    else:
        raise ValueError(kind)
    return Case("%s-P%d-k%d" % (kind, P, k), p, idx.contiguous(), d2.contiguous(), mask=mask, rigid=alive)


MODEL_SPECS = (
    [("compact", P, k) for P, k in ((1, 1), (1, 8), (2, 1), (2, 8), (5, 8), (5, 20), (20, 20), (21, 20), (21, 8), (255, 8), (255, 20),
                                    (256, 8), (256, 20), (257, 1), (257, 20), (1024, 8), (1024, 20), (1025, 8), (1025, 20))]
    + [("clones", 256, 8), ("clones", 1025, 20), ("initial", 1, 8), ("initial", 257, 20), ("initial", 1024, 8),
       ("half_initial", 21, 20), ("half_initial", 256, 8), ("late_t", 257, 8), ("late_t", 1024, 20), ("thin_time", 255, 20),
       ("thin_time", 1025, 8)])
TABLE_SPECS = [("hub", 257, 1), ("hub", 1024, 8), ("repeats", 256, 8), ("self_only", 255, 8), ("foreign", 256, 8), ("foreign", 1024, 8),
               ("foreign", 1024, 20), ("reversed", 257, 20)]


def spec_id(spec):
    return "%s-P%d-k%d" % spec


@functools.lru_cache(maxsize=None)
def model_case(kind, P, k):
    return _checked(_model(kind, P, k))


@functools.lru_cache(maxsize=None)
def table_case(kind, P, k):
    return _checked(_table(kind, P, k))


def case_of(spec):
    return (table_case if spec in TABLE_SPECS else model_case)(*spec)
