#!/usr/bin/env python3
"""Generate the Allen-Cahn fixtures by running the *reference* (PyMGRIT) where it is installed.

Like make_golden.py this imports the reference with the size-1 ``mpi4py`` stand-in of ``tests/golden/_mpi_stub`` and writes numbers
only:

  tests/golden/allen_cahn.json   parameters of every case, the reference's own relative residual rho of every stored IMEX step
                                 (rho = norm_inf((I - dt L) x_ref - b) / norm_inf(b), with the reference's sparse matrix), and the
                                 residual histories of Mgrit(...).solve()
  tests/golden/allen_cahn.npz    input states and the reference's step outputs

Usage:  python tests/golden/make_golden_allen_cahn.py      (needs the reference: PYMGRIT_REFERENCE, default as in make_golden.py; ~1 min)
Nothing here is imported by the product.
"""
import json
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PYMGRIT_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(HERE, "_mpi_stub"))
sys.path.insert(0, os.path.join(REF, "src"))
warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402
from pymgrit.core.mgrit import Mgrit  # noqa: E402
from pymgrit.allen_cahn.allen_cahn import AllenCahn, VectorAllenCahn2D  # noqa: E402

QUIET = 30
T_STOP = 0.01     # the solves' time interval [0, T_STOP]; eps = 0.04: dt / eps^2 <= 0.78 on the coarsest grids below


def one_step(app, u, dt):
    vec = VectorAllenCahn2D(app.nx, app.ny)
    vec.set_values(u.copy())
    return np.asarray(app.step(vec, 0.0, dt).get_values(), dtype=np.float64)


def main():
    meta, arr = {"steps": {}, "newton_steps": {}, "solve": {}, "t_stop": T_STOP}, {}
    rng = np.random.default_rng(20240607)
    cases = [(nx, 2, dt) for nx in (32, 48, 63, 64) for dt in (1e-4, 1e-3)] + [(32, 4, 1e-3)]
    for nx, nu, dt in cases:
        app = AllenCahn(nx=nx, nu=nu, method='IMEX', t_start=0, t_stop=1, nt=2)
        key_rand = f"rand_nx{nx}"
        if key_rand not in arr:
            arr[key_rand] = rng.uniform(-1.0, 1.0, size=(nx, nx))
        for src, u in (("init", np.asarray(app.initial_guess().get_values())), ("rand", arr[key_rand])):
            name = f"imex_{src}_nx{nx}_nu{nu}_dt{dt:g}"
            x = one_step(app, u, dt)
            flat = u.flatten()
            b = flat + dt * (1 / app.eps ** 2 * flat * (1.0 - flat ** nu))
            res = (app.id - dt * app.space_disc).dot(x.flatten()) - b
            rho = float(np.linalg.norm(res, np.inf) / np.linalg.norm(b, np.inf))
            arr["out_" + name] = x
            meta["steps"][name] = dict(nx=nx, nu=nu, eps=app.eps, dt=dt, src=src, rho=rho)
    for method in ("IMPL", "CN"):
        app = AllenCahn(nx=32, method=method, t_start=0, t_stop=1, nt=2)
        name = f"{method.lower()}_init_nx32_dt0.001"
        arr["out_" + name] = one_step(app, np.asarray(app.initial_guess().get_values()), 1e-3)
        meta["newton_steps"][name] = dict(nx=32, nu=2, eps=app.eps, dt=1e-3, method=method)
    solves = {
        "imex_2lvl_V": dict(method="IMEX", nts=[33, 9], opts=dict(cycle_type='V', nested_iteration=False)),
        "imex_3lvl_V_nested": dict(method="IMEX", nts=[33, 17, 9], opts=dict(cycle_type='V', nested_iteration=True)),
        "imex_3lvl_F": dict(method="IMEX", nts=[33, 17, 9], opts=dict(cycle_type='F', nested_iteration=False)),
        "imex_2lvl_jump": dict(method="IMEX", nts=[33, 9], opts=dict(cycle_type='V', nested_iteration=False, conv_crit=1)),
        "impl_2lvl_V": dict(method="IMPL", nts=[33, 9], opts=dict(cycle_type='V', nested_iteration=False)),
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
    with open(os.path.join(HERE, "allen_cahn.json"), "w") as f:
        json.dump(meta, f, indent=1)
    np.savez_compressed(os.path.join(HERE, "allen_cahn.npz"), **arr)


if __name__ == "__main__":
    main()
