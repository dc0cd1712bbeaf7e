#!/usr/bin/env python3
"""Generate the fixtures of the Allen-Cahn Newton steps (methods IMPL and CN) by running the *reference* (PyMGRIT) where it is
installed. Like make_golden_allen_cahn.py this imports the reference with the size-1 ``mpi4py`` stand-in of ``tests/golden/_mpi_stub``
and writes numbers only:

  tests/golden/allen_cahn_newton.json   parameters of every case and the residual histories of Mgrit(...).solve()
  tests/golden/allen_cahn_newton.npz    the random input states, the reference's step outputs and the solves' last states

Every grid meets the rule of ``linear_solver='pcg'``: theta * dt / eps^2 < 1 (eps = 0.04; the largest is IMPL at dt = 1.25e-3: 0.78).

Usage:  PYMGRIT_REFERENCE=... python tests/golden/make_golden_allen_cahn_newton.py      (PYMGRIT_REFERENCE = the reference checkout; ~1 min)
Nothing here is imported by the product.
"""
import json
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ["PYMGRIT_REFERENCE"]      # the reference checkout (its src/ holds the pymgrit package)
sys.path.insert(0, os.path.join(HERE, "_mpi_stub"))
sys.path.insert(0, os.path.join(REF, "src"))
warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402
from pymgrit.core.mgrit import Mgrit  # noqa: E402
from pymgrit.allen_cahn.allen_cahn import AllenCahn, VectorAllenCahn2D  # noqa: E402

QUIET = 30
T_STOP = 0.01


def one_step(app, u, dt):
    vec = VectorAllenCahn2D(app.nx, app.ny)
    vec.set_values(u.copy())
    return np.asarray(app.step(vec, 0.0, dt).get_values(), dtype=np.float64)


def main():
    meta, arr = {"steps": {}, "solve": {}, "t_stop": T_STOP}, {}
    rng = np.random.default_rng(20240611)
    for nx, nu, dt in ((20, 2, 1e-3), (20, 4, 5e-4), (33, 2, 1.25e-4)):
        key_rand = f"rand_nx{nx}"
        if key_rand not in arr:
            arr[key_rand] = rng.uniform(-1.0, 1.0, size=(nx, nx))
        for method in ("IMPL", "CN"):
            app = AllenCahn(nx=nx, nu=nu, method=method, t_start=0, t_stop=1, nt=2)
            for src, u in (("init", np.asarray(app.initial_guess().get_values())), ("rand", arr[key_rand])):
                name = f"{method.lower()}_{src}_nx{nx}_nu{nu}_dt{dt:g}"
                arr["out_" + name] = one_step(app, u, dt)
                meta["steps"][name] = dict(nx=nx, nu=nu, eps=app.eps, dt=dt, src=src, method=method, newton_tol=app.newton_tol)
    solves = {
        "cn_2lvl_V": dict(method="CN", nts=[33, 9], opts=dict(cycle_type='V', nested_iteration=False)),
        "cn_3lvl_F": dict(method="CN", nts=[33, 17, 9], opts=dict(cycle_type='F', nested_iteration=False)),
        "impl_3lvl_V_nested": dict(method="IMPL", nts=[33, 17, 9], opts=dict(cycle_type='V', nested_iteration=True)),
    }
    for name, rec in solves.items():
        prob = [AllenCahn(nx=32, method=rec["method"], t_start=0, t_stop=T_STOP, nt=nt) for nt in rec["nts"]]
        opts = dict(tol=1e-8, max_iter=12, **rec["opts"])
        mg = Mgrit(problem=prob, logging_lvl=QUIET, **opts)
        out = mg.solve()
        u = np.array([np.asarray(v.get_values()) for v in mg.u[0]])
        meta["solve"][name] = dict(nx=32, method=rec["method"], nts=rec["nts"], opts=opts, conv=[float(c) for c in out["conv"]],
                                   spacetime_norm=float(np.sqrt(np.sum(u * u))))
        arr["last_" + name] = u[-1]
    with open(os.path.join(HERE, "allen_cahn_newton.json"), "w") as f:
        json.dump(meta, f, indent=1)
    np.savez_compressed(os.path.join(HERE, "allen_cahn_newton.npz"), **arr)


if __name__ == "__main__":
    main()
