"""What the GPU parity tests share (test_hip_parity.py and the files that hold other device paths against the parity oracle the same
way): the product hierarchy on the GPU beside the oracle problem, the same random states on both, the bit-exact comparison. A plain
helper like cases.py: no tests, no fixtures."""
import numpy as np
import pytest

import cases


def need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible (HIP path has no CPU fallback)")


def heat_problem(nx, grids, x_end=1.0, a=1.0, forcing=True):
    from pymgrit_amd import Heat1D
    kw = dict(rhs_separable=[(cases.rhs_space, cases.rhs_time)]) if forcing else {}
    return [Heat1D(x_start=0, x_end=x_end, nx=nx, a=a, init_cond=cases.init_cond, t_interval=np.asarray(t), **kw)
            for t in grids]


def advection_problem(nx, grids, c=1.0):
    from pymgrit_amd import Advection1D
    return [Advection1D(c=c, x_start=-1, x_end=1, nx=nx, t_interval=np.asarray(t)) for t in grids]


def make_pair(oracle, kind, nx, grids, transfer=None, x_end=1.0, forcing=True, **opts):
    """(product Mgrit on the GPU, oracle problem) for the same hierarchy; no nested iteration unless asked."""
    from pymgrit_amd import GridTransferAdvection, GridTransferCopy, GridTransferHeat, Mgrit
    opts.setdefault("nested_iteration", False)
    nxs = nx if isinstance(nx, (list, tuple)) else [nx] * len(grids)
    if kind == "heat":
        prob = [heat_problem(n, [t], x_end=x_end, forcing=forcing)[0] for n, t in zip(nxs, grids)]
        specs = [cases.heat_level_spec(n, t, x_end=x_end, forcing=forcing) for n, t in zip(nxs, grids)]
    else:
        prob = [advection_problem(n, [t])[0] for n, t in zip(nxs, grids)]
        specs = [cases.advection_level_spec(n, t) for n, t in zip(nxs, grids)]
    tr = None
    if transfer is not None:
        tr = [GridTransferHeat() if k == 1 else GridTransferAdvection() if k == 2 else GridTransferCopy() for k in transfer]
    mg = Mgrit(prob, transfer=tr, logging_lvl=30, **opts)
    oopts = {k: v for k, v in opts.items() if k != "random_init_guess"}
    op = oracle.OracleProblem(specs, transfer=transfer, variant=1, **oopts)
    return mg, op


def randomize(mg, op, seed=0):
    """same random u, v, g on both sides"""
    rng = np.random.default_rng(seed)
    for lvl in range(mg.lvl_max):
        for name, slabs in (("u", mg.backend.U), ("v", mg.backend.V), ("g", mg.backend.G)):
            if slabs[lvl] is None:
                continue
            ref = op.state(name, lvl)
            ref[:] = rng.standard_normal(ref.shape)
            mg.backend.set_natural(name, lvl, ref)


def assert_state_equal(mg, op, what=("u", "v", "g")):
    import torch
    for lvl in range(mg.lvl_max):
        for name, slabs in (("u", mg.backend.U), ("v", mg.backend.V), ("g", mg.backend.G)):
            if name not in what or slabs[lvl] is None:
                continue
            ref = op.state(name, lvl)
            got = mg.backend.natural(name, lvl)
            assert np.array_equal(got, ref), (name, lvl, np.abs(got - ref).max())
            pad = torch.ones(slabs[lvl].shape[1], dtype=torch.bool, device=slabs[lvl].device)
            pad[mg.backend.perm[lvl]] = False
            # padding positions of a row: unspecified FINITE values (a Phi whose rank-one correction is evaluated in closed form
            # leaves -z0 * w there instead of 0; the kernels zero them between their scans and mask them in the norms)
            assert torch.isfinite(slabs[lvl][:, pad]).all().item(), ("padding positions must stay finite", name, lvl)
