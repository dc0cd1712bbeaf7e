"""CPU: the two 2-D library transfers (GridTransferHeat2D, GridTransferAllenCahn; spec: DESIGN.md 3.10) as Python classes.

The yardstick of the operator tests is a dense matrix built here by np.kron from the 1-D stencils: restriction [1 2 1]/4 with injected
ends (or its periodic form) per axis, interpolation [1/2 1 1/2] per axis. The classes sum nine (four) terms in a fixed order, the dense
product sums them in another: at most eight roundings of terms no larger than the input, so the bound is 8 eps max|input|.
"""
import numpy as np
import pytest

import cases
from pymgrit_amd import GridTransferAllenCahn, GridTransferHeat2D
from pymgrit_amd.allen_cahn.allen_cahn import VectorAllenCahn2D
from pymgrit_amd.heat.heat_2d import VectorHeat2D

EPS = np.finfo(np.float64).eps
HEAT_SHAPES = [(5, 7), (17, 21), (67, 35)]
AC_SIZES = [8, 20, 66]


def r1d_rim(nf):
    """1-D restriction of a grid with its end points, nf = 2 nc - 1: the ends injected, [1 2 1]/4 inside"""
    nc = (nf + 1) // 2
    R = np.zeros((nc, nf))
    R[0, 0] = R[-1, -1] = 1.0
    for I in range(1, nc - 1):
        R[I, 2 * I - 1:2 * I + 2] = (0.25, 0.5, 0.25)
    return R


def inj1d(nf):
    nc = (nf + 1) // 2
    R = np.zeros((nc, nf))
    R[np.arange(nc), 2 * np.arange(nc)] = 1.0
    return R


def p1d_rim(nc):
    P = np.zeros((2 * nc - 1, nc))
    for I in range(nc):
        P[2 * I, I] = 1.0
    for I in range(nc - 1):
        P[2 * I + 1, I] = P[2 * I + 1, I + 1] = 0.5
    return P


def r1d_periodic(nf):
    nc = nf // 2
    R = np.zeros((nc, nf))
    for I in range(nc):
        R[I, (2 * I - 1) % nf] += 0.25
        R[I, 2 * I] += 0.5
        R[I, (2 * I + 1) % nf] += 0.25
    return R


def p1d_periodic(nc):
    P = np.zeros((2 * nc, nc))
    for I in range(nc):
        P[2 * I, I] += 1.0
        P[2 * I + 1, I] += 0.5
        P[2 * I + 1, (I + 1) % nc] += 0.5
    return P


def heat_restriction_matrix(nx, ny):
    """full weighting kron(Rx, Ry) on the interior coarse points, injection kron(Ix, Iy) on the rim"""
    full, inj = np.kron(r1d_rim(nx), r1d_rim(ny)), np.kron(inj1d(nx), inj1d(ny))
    nxc, nyc = (nx + 1) // 2, (ny + 1) // 2
    rim = np.zeros((nxc, nyc), dtype=bool)
    rim[0, :] = rim[-1, :] = rim[:, 0] = rim[:, -1] = True
    return np.where(rim.ravel()[:, None], inj, full)


def heat_vec(a):
    v = VectorHeat2D(*a.shape)
    v.set_values(a.copy())
    return v


def ac_vec(a):
    v = VectorAllenCahn2D(*a.shape)
    v.set_values(a.copy())
    return v


@pytest.mark.parametrize("shape", HEAT_SHAPES)
def test_heat2d_operators_against_dense(shape):
    nx, ny = shape
    nxc, nyc = (nx + 1) // 2, (ny + 1) // 2
    rng = np.random.default_rng(100 * nx + ny)
    tr = GridTransferHeat2D()
    f = rng.uniform(-1.0, 1.0, size=(nx, ny))
    got = np.asarray(tr.restriction(heat_vec(f)).get_values())
    want = (heat_restriction_matrix(nx, ny) @ f.ravel()).reshape(nxc, nyc)
    assert got.shape == (nxc, nyc)
    assert np.max(np.abs(got - want)) <= 8 * EPS * np.max(np.abs(f))
    c = rng.uniform(-1.0, 1.0, size=(nxc, nyc))
    got = np.asarray(tr.interpolation(heat_vec(c)).get_values())
    want = (np.kron(p1d_rim(nxc), p1d_rim(nyc)) @ c.ravel()).reshape(nx, ny)
    assert got.shape == (nx, ny)
    assert np.max(np.abs(got - want)) <= 8 * EPS * np.max(np.abs(c))


@pytest.mark.parametrize("nx", AC_SIZES)
def test_allen_cahn_operators_against_dense(nx):
    nc = nx // 2
    rng = np.random.default_rng(7 * nx)
    tr = GridTransferAllenCahn()
    f = rng.uniform(-1.0, 1.0, size=(nx, nx))
    got = np.asarray(tr.restriction(ac_vec(f)).get_values())
    want = (np.kron(r1d_periodic(nx), r1d_periodic(nx)) @ f.ravel()).reshape(nc, nc)
    assert got.shape == (nc, nc)
    assert np.max(np.abs(got - want)) <= 8 * EPS * np.max(np.abs(f))
    c = rng.uniform(-1.0, 1.0, size=(nc, nc))
    got = np.asarray(tr.interpolation(ac_vec(c)).get_values())
    want = (np.kron(p1d_periodic(nc), p1d_periodic(nc)) @ c.ravel()).reshape(nx, nx)
    assert got.shape == (nx, nx)
    assert np.max(np.abs(got - want)) <= 8 * EPS * np.max(np.abs(c))


@pytest.mark.parametrize("shape", HEAT_SHAPES)
def test_heat2d_exact_identities(shape):
    nx, ny = shape
    nxc, nyc = (nx + 1) // 2, (ny + 1) // 2
    tr = GridTransferHeat2D()
    # a constant whose multiples up to 16 k are floating-point numbers goes through exactly (every partial sum is exact) ...
    k = 1.375 + 2.0 ** -30
    assert np.array_equal(tr.interpolation(heat_vec(np.full((nxc, nyc), k))).get_values(), np.full((nx, ny), k))
    assert np.array_equal(tr.restriction(heat_vec(np.full((nx, ny), k))).get_values(), np.full((nxc, nyc), k))
    # ... any other one to the bound of the operator tests (the partial sums 3 k, 12 k ... 15 k round)
    k = 0.3 + 1.0 / 3.0
    assert np.max(np.abs(tr.interpolation(heat_vec(np.full((nxc, nyc), k))).get_values() - k)) <= 8 * EPS * k
    assert np.max(np.abs(tr.restriction(heat_vec(np.full((nx, ny), k))).get_values() - k)) <= 8 * EPS * k
    # a bilinear field a + b x + c y + d x y is reproduced by the bilinear interpolation, and full weighting of it is its own value
    X, Y = np.meshgrid(np.linspace(0, 1, nxc), np.linspace(0, 1, nyc), indexing="ij")
    field = 0.7 - 1.1 * X + 0.4 * Y + 2.3 * X * Y
    back = np.asarray(tr.restriction(tr.interpolation(heat_vec(field))).get_values())
    assert np.max(np.abs(back - field)) <= 8 * EPS * np.max(np.abs(field))


@pytest.mark.parametrize("nx", AC_SIZES)
def test_allen_cahn_exact_identities(nx):
    nc = nx // 2
    tr = GridTransferAllenCahn()
    k = 1.375 + 2.0 ** -30      # (see test_heat2d_exact_identities)
    assert np.array_equal(tr.interpolation(ac_vec(np.full((nc, nc), k))).get_values(), np.full((nx, nx), k))
    assert np.array_equal(tr.restriction(ac_vec(np.full((nx, nx), k))).get_values(), np.full((nc, nc), k))
    k = 0.3 + 1.0 / 3.0
    assert np.max(np.abs(tr.interpolation(ac_vec(np.full((nc, nc), k))).get_values() - k)) <= 8 * EPS * k
    assert np.max(np.abs(tr.restriction(ac_vec(np.full((nx, nx), k))).get_values() - k)) <= 8 * EPS * k
    R, P = np.kron(r1d_periodic(nx), r1d_periodic(nx)), np.kron(p1d_periodic(nc), p1d_periodic(nc))
    assert np.array_equal(R, P.T / 4)      # (entries are multiples of 1/16: exact)
    # ... and the classes ARE these matrices: unit vectors go through without rounding
    for k in (0, nc + 1, nc * nc - 1):
        e = np.zeros(nc * nc)
        e[k] = 1.0
        assert np.array_equal(np.asarray(tr.interpolation(ac_vec(e.reshape(nc, nc))).get_values()).ravel(), P[:, k])
    for k in (0, nx + 1, nx * nx - 1):
        e = np.zeros(nx * nx)
        e[k] = 1.0
        assert np.array_equal(np.asarray(tr.restriction(ac_vec(e.reshape(nx, nx))).get_values()).ravel(), R[:, k])


def test_wrong_shapes_raise():
    h, a = GridTransferHeat2D(), GridTransferAllenCahn()
    for shape in ((6, 7), (7, 8), (16, 20)):
        with pytest.raises(Exception, match=str(shape[0])):
            h.restriction(heat_vec(np.zeros(shape)))
    for shape in ((7, 7), (8, 9)):
        with pytest.raises(Exception, match=str(shape[1])):
            a.restriction(ac_vec(np.zeros(shape)))
    assert h.device_transfer() == 4 and a.device_transfer() == 5


def test_plugin_path_solve_equals_the_user_class():
    """two-level Heat2D 17 x 21 -> 9 x 11 on the host (device_stepper = None): the library class converges like, and computes exactly what,
    the user's Coarsen2D of tests/test_hip_user_transfer.py computes -- the arithmetic is the same"""
    from pymgrit_amd import GridTransfer, Mgrit
    from pymgrit_amd.heat.heat_2d import Heat2D

    class Coarsen2D(GridTransfer):
        def restriction(self, u):
            f = np.asarray(u.get_values())
            nxc, nyc = (f.shape[0] + 1) // 2, (f.shape[1] + 1) // 2
            c = f[::2, ::2].copy()
            c[1:-1, 1:-1] = (4 * f[2:-2:2, 2:-2:2] + 2 * (f[1:-3:2, 2:-2:2] + f[3:-1:2, 2:-2:2] + f[2:-2:2, 1:-3:2] + f[2:-2:2, 3:-1:2]) +
                             f[1:-3:2, 1:-3:2] + f[1:-3:2, 3:-1:2] + f[3:-1:2, 1:-3:2] + f[3:-1:2, 3:-1:2]) / 16
            out = VectorHeat2D(nxc, nyc)
            out.set_values(c)
            return out

        def interpolation(self, u):
            c = np.asarray(u.get_values())
            f = np.zeros((2 * c.shape[0] - 1, 2 * c.shape[1] - 1))
            f[::2, ::2] = c
            f[1::2, ::2] = (c[:-1, :] + c[1:, :]) / 2
            f[::2, 1::2] = (c[:, :-1] + c[:, 1:]) / 2
            f[1::2, 1::2] = (c[:-1, :-1] + c[1:, :-1] + c[:-1, 1:] + c[1:, 1:]) / 4
            out = VectorHeat2D(*f.shape)
            out.set_values(f)
            return out

    def solve(transfer):
        t0 = np.linspace(0, 1, 33)
        prob = [Heat2D(x_start=0, x_end=cases.H2D_X_END, y_start=0, y_end=cases.H2D_Y_END, nx=nx, ny=ny, a=cases.H2D_A,
                       rhs_separable=[(cases.h2d_s0, lambda t: 1.0)], t_interval=t) for (nx, ny), t in (((17, 21), t0), ((9, 11), t0[::2]))]
        for p in prob:
            p.device_stepper = lambda: None
        mg = Mgrit(prob, transfer=[transfer], logging_lvl=30, tol=1e-9, max_iter=8)
        assert type(mg.backend).__name__ == "PluginBackend"
        conv = np.asarray(mg.solve()["conv"])
        return conv, np.array([np.asarray(mg.u[0][i].get_values()) for i in range(33)])
    conv, u = solve(GridTransferHeat2D())
    assert len(conv) <= 8 and conv[-1] < 1e-9, conv
    conv_user, u_user = solve(Coarsen2D())
    assert np.array_equal(conv, conv_user), (conv, conv_user)
    assert np.array_equal(u, u_user)
