"""What the GPU tests of the 2-D grid transfers share (test_hip_transfer2d.py, test_hip_transfer2d_planes.py and the transfer tests of
the periodic 2-D kinds). A plain helper like cases.py: no tests, no fixtures."""
import numpy as np


def one_step_size(t):
    return len(set(np.diff(np.asarray(t, dtype=np.float64)).view(np.int64).tolist())) == 1


def solve(prob, tr, solver=None, **opts):
    from pymgrit_amd import Mgrit
    mg = (solver or Mgrit)(problem=prob, transfer=tr, logging_lvl=30, **opts)
    conv = np.asarray(mg.solve()["conv"])
    return conv, mg


def fill(mg, seed):
    rng = np.random.default_rng(seed)
    b = mg.backend
    for lvl in range(mg.lvl_max):
        for name, slabs in (("u", b._U), ("v", b.V), ("g", b.G)):
            if slabs[lvl] is not None:
                b.set_natural(name, lvl, rng.uniform(-1.0, 1.0, size=(slabs[lvl].shape[0], b.n[lvl])))


def raw(mg, name, lvl):
    b = mg.backend
    b.sync()
    return {"u": b._U, "v": b.V, "g": b.G}[name][lvl].cpu().numpy()
