#!/usr/bin/env python3
"""Golden vectors for the time slice (fdgs.slice, tests/slice_oracle.py), produced by the REFERENCE's own functions in float64:

  * scene/gaussian_model.py: get_current_covariance_and_mean_offset / get_covariance / get_cov_t / get_marginal_t (cut out of the
    class as tests/golden/make_golden_pycov.py does) on random raw parameters -- rot_4d on and off, prefilter_var on and off,
    scaling modifier 1 and 0.7;
  * utils/sh_utils.py: eval_shfs_4d(3, D_t, sh, dirs, dirs_t, T) on random coefficients, D_t = 0, 1, 2 (the file is executed in place).

No reference source is copied: this script reads /root/reference at run time.   python tests/golden/make_golden_slice.py
Fixtures: tests/golden/slice/geo_*.npz and tests/golden/slice/sh_t*.npz (P = 64).  tests/test_slice_host.py holds
tests/slice_oracle.py to them.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_pycov import REF, reference_model_class  # noqa: E402

P = 64


def main():
    if not os.path.isdir(REF):
        raise SystemExit("needs /root/reference")
    out_dir = os.path.join(HERE, "slice")
    os.makedirs(out_dir, exist_ok=True)
    Ref = reference_model_class()
    # float64 throughout: the reference's helpers allocate their matrices as ``torch.float`` (looked up when they run)
    torch.set_default_dtype(torch.float64)
    torch.float = torch.float64
    g = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    for rot_4d in (True, False):
        for pv in (-1.0, 0.02):
            for mod in (1.0, 0.7):
                m = Ref.__new__(Ref)
                m.rot_4d, m.gaussian_dim, m.prefilter_var = rot_4d, 4, pv
                m._xyz = rn(P, 3)
                m._scaling = rn(P, 3) * 0.5 - 2.0
                m._scaling_t = rn(P, 1) * 0.5 - 1.0
                m._rotation = rn(P, 4)
                m._rotation_r = rn(P, 4)
                m._t = rn(P, 1) * 0.6
                m.setup_functions()
                ts = 0.3
                d = {"xyz": m._xyz, "scaling": m._scaling, "scaling_t": m._scaling_t, "rotation": m._rotation, "rotation_r": m._rotation_r,
                     "t": m._t, "mod": torch.tensor(mod), "timestamp": torch.tensor(ts), "prefilter_var": torch.tensor(pv),
                     "rot_4d": torch.tensor(rot_4d)}
                if rot_4d:
                    d["cov"], d["mean_offset"] = m.get_current_covariance_and_mean_offset(mod, ts)
                else:
                    d["cov"] = m.get_covariance(mod)   # R^T S^2 R: the Python side's; the kernels build R S^2 R^T (tests/test_slice_host.py)
                d["marginal_t"] = m.get_marginal_t(ts, mod)
                name = "geo_%s_pf%s_mod%s.npz" % ("rot4d" if rot_4d else "dim4", "on" if pv > 0 else "off", ("%g" % mod).replace(".", ""))
                np.savez_compressed(os.path.join(out_dir, name), **{k: v.numpy() for k, v in d.items()})
                print(name, {k: tuple(v.shape) for k, v in d.items() if v.dim()})
    ns = {"__name__": "ref_sh_utils"}
    exec(compile(open(os.path.join(REF, "utils", "sh_utils.py")).read(), "sh_utils.py", "exec"), ns)
    T = 10.0
    for D_t in (0, 1, 2):
        sh = (rn(P, 48, 3) * 0.3).float().double()     # fp32 values, evaluated in float64
        dirs = torch.nn.functional.normalize(rn(P, 3), dim=1)
        dirs_t = rn(P, 1) * 4.0
        colour = ns["eval_shfs_4d"](3, D_t, sh.transpose(1, 2), dirs, dirs_t, T)
        name = "sh_t%d.npz" % D_t
        np.savez_compressed(os.path.join(out_dir, name), sh=sh.float().numpy(), dirs=dirs.numpy(), dirs_t=dirs_t.numpy(),
                            T=np.float64(T), D_t=np.int64(D_t), colour=colour.numpy())
        print(name, tuple(colour.shape))


if __name__ == "__main__":
    sys.exit(main())
