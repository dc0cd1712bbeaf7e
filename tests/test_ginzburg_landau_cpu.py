"""GinzburgLandau2D on the host (no GPU): the IMEX step against an independent high-precision Phi that uses no transform
(tests/ginzburg_landau_reference.py: the right-hand side in long double, the 2 nx^2 x 2 nx^2 block system by sparse LU and refinement in
long double), the known answers of the scheme, the state vector, the transfer, the refusals, the device description, a plugin-path
solve and the exports.

Tolerance of one IMEX step, nothing in it measured on the code under test. Errors and norms are 2-norms over BOTH planes (all 2 nx^2
values); EPS = 2^-52, a rounding is at most EPS / 2 relative:

    norm(error) <= (C(nx) + ALLOWANCE) EPS M,      C(nx) = 4 nx + 25,      valid for  rr sqrt(1 + b^2) <= 1 / 4,  rr = dt / dx^2
    M = norm((R, S)),   R = |x| + dt (|x| + q (|x| + |c| |y|)),   S = |y| + dt (|y| + q (|c| |x| + |y|)),   q = x^2 + y^2

M is the majorant of the norm of (r, s), taken as the Burgers and Navier-Stokes tests take theirs: r and s with every term's sign
dropped, so |r| <= R and |s| <= S point by point and so is every intermediate of their evaluation.
  * 4 nx: a product with an orthogonal n x n matrix is off by at most n EPS times the operand's 2-norm (test_allen_cahn_cpu.py derives
    the rule). X = T r T and Y = T s T are two products per plane: off by 2 nx EPS norm(r) and 2 nx EPS norm(s), over both planes
    2 nx EPS norm((r, s)). The join is, per mode, the 2 x 2 block [[Da, Db], [-Db, Da]] of 2-norm sqrt(Da^2 + Db^2) = 1 / sqrt(det)
    <= 1: it carries that error on undamped at most, and norm((Zx, Zy)) <= norm((r, s)). The two products back, per plane:
    2 nx EPS norm((Zx, Zy)). Together 4 nx EPS norm((r, s)) <= 4 nx EPS M.
  * 4: the pointwise map. q = x x + y y: three roundings, 1 EPS relative (all terms positive). c y and x - c y: 1 EPS of |x| + |c| |y|.
    The product with q: 1 + 1 + 1/2 = 2.5 EPS of q (|x| + |c| |y|). The difference with x, the product with dt, the sum with x: 1/2
    each, relative to partial results that R bounds. 4 EPS R at a point, 4 EPS M in the norm; s likewise.
  * 19.5: the table. What enters is the error of the block [[Da, Db], [-Db, Da]] in the 2-norm, sqrt(dDa^2 + dDb^2).
    lam_k = (4 / dx^2) sin^2(pi k / nx). Its square and scale are two roundings and 4 / dx^2 a rounded quotient: 2 EPS relative. The sum
    lam_i + lam_j, the product with dt, 1 +: a = 1 + dt mu to 3.5 EPS; b dt and its product with mu: beta to 3.5 EPS; det = a a + beta beta
    to 2 * 3.5 + 1/2 + 1/2 = 8; Da = a / det and Db = beta / det to 3.5 + 8 + 1/2 = 12 EPS relative each, 12 EPS sqrt(Da^2 + Db^2) <= 12 EPS
    for the block. The sine's argument pi k / nx carries up to 1.5 EPS relative (pi, a product, a quotient); for the mirrored modes
    k > nx / 2 that is an ABSOLUTE error of the eigenvalue of up to (4 / dx^2) 3 (pi - phi) sin(phi) cos(phi) EPS, phi = pi (nx - k) / nx,
    at most 14.4 EPS / dx^2 per axis, 29 EPS / dx^2 in mu: dt mu is off by up to 29 rr EPS, the block M = [[a, -beta], [beta, a]] by
    29 rr sqrt(1 + b^2) EPS in the 2-norm and its inverse by that times norm(M^-1)^2 = 1 / det <= 1. With rr sqrt(1 + b^2) <= 1 / 4, which
    every case below asserts: 7.25 EPS. Together 19.25. (The device tables are formed from long-double eigenvalues and are closer.)
  * 1: the join's own arithmetic, X Da + Y Db: two products and a sum, 1/2 each, relative to |X Da| + |Y Db| <= |(X, Y)| sqrt(Da^2 + Db^2).
  Sum: 4 nx + 4 + 19.25 + 1 = 4 nx + 24.25; C(nx) = 4 nx + 25.
  * ALLOWANCE (1): what the reference is off by, EPS norm((r, s)) <= EPS M (ginzburg_landau_reference.py).
numpy does not fuse and neither does the device map. The largest error / bound over all cases of the first test is printed ("RATIO
host_imex: worst") and recorded in DESIGN.md 3.15; it is a record, not a threshold to tune.
"""
import logging

import numpy as np
import pytest

import cases
from ginzburg_landau_reference import ALLOWANCE, LD, ReferenceGinzburgLandau2D, reference_phi, right_hand_side

EPS = cases.EPS


def C(nx):
    return 4 * nx + 25


def make(nx, cls=None, **kw):
    from pymgrit_amd import GinzburgLandau2D
    kw.setdefault("t_start", 0), kw.setdefault("t_stop", 1), kw.setdefault("nt", 2)
    kw.setdefault("L", float(nx))      # dx = 1 for every nx
    return (cls or GinzburgLandau2D)(nx=nx, **kw)


def apply_step(app, w, dt):
    from pymgrit_amd import VectorGinzburgLandau2D
    vec = VectorGinzburgLandau2D(app.nx)
    vec.set_values(np.array(w, dtype=np.float64).reshape(2, app.nx, app.nx))
    return np.asarray(app.step(vec, 0.0, dt).get_values())


def majorant(w, dt, c):
    """M of the module docstring, evaluated by this file's own formula"""
    x, y = np.abs(w[0]), np.abs(w[1])
    q = x * x + y * y
    R = x + dt * (x + q * (x + abs(c) * y))
    S = y + dt * (y + q * (abs(c) * x + y))
    return float(np.sqrt(np.sum(R * R) + np.sum(S * S)))


def table_condition(app, dt):
    """rr sqrt(1 + b^2), which C(nx) wants at most 1 / 4"""
    return dt / app.dx ** 2 * np.sqrt(1.0 + app.b ** 2)


REF_NX = [4, 9, 20, 33, 64, 66, 97]      # the smallest grid, an odd one, K steps (32) and tiles (64) of the device product + 1 / + 2
REF_BC = [(1.5, -0.8), (0.0, 0.0), (-2.0, 0.5)]
REF_DT = [0.1, 0.02, 2.0 ** -6]
WORST = {}


@pytest.mark.parametrize("nx", REF_NX)
def test_host_imex_step_matches_the_high_precision_phi(nx):
    """_step_imex (Hartley table, lam_k, the (Da, Db) table, the float64 map, the join) against reference_phi, which shares none of it:
    a wrong eigenvalue, swapped planes, a wrong sign of Db or of c shows here"""
    rng = np.random.default_rng(1000 * nx)
    worst = 0.0
    for b, c in REF_BC:
        app = make(nx, b=b, c=c)
        for dt in REF_DT:
            assert table_condition(app, dt) <= 0.25
            inputs = [("uniform [-1, 1]^2", rng.uniform(-1.0, 1.0, size=(2, nx, nx))),
                      ("mean 3", 3.0 + rng.uniform(-1.0, 1.0, size=(2, nx, nx))),
                      ("zero", np.zeros((2, nx, nx)))]
            for what, w in inputs:
                got, ref = apply_step(app, w, dt), reference_phi(w, dt, nx, b, c, app.L)
                assert got.shape == ref.shape == (2, nx, nx)
                err, tol = float(np.linalg.norm(got - ref)), (C(nx) + ALLOWANCE) * EPS * majorant(w, dt, c)
                if what == "zero":
                    assert err == 0.0 and tol == 0.0
                    continue
                worst = max(worst, err / tol)
                print(f"RATIO host_imex[nx={nx},b={b},c={c},dt={dt}] {what}: error/bound {err / tol:.4f}")
                assert err <= tol, (nx, b, c, dt, what, err, tol)
    WORST[nx] = worst
    print(f"RATIO host_imex[nx={nx}]: worst error/bound {worst:.4f}")
    print(f"RATIO host_imex: worst error/bound over the sizes so far {max(WORST.values()):.4f}")


def test_the_bound_sees_a_relative_change_of_1e_10_in_b():
    """what the comparison above can see: the host step with b changed by 1e-10 relative misses the reference of the unchanged b by
    more than the bound"""
    nx, dt, b, c = 20, 0.1, 1.5, -0.8
    w = np.random.default_rng(7).uniform(-1.0, 1.0, size=(2, nx, nx))
    app = make(nx, b=b * (1.0 + 1e-10), c=c)
    got, ref = apply_step(app, w, dt), reference_phi(w, dt, nx, b, c, app.L)
    err, tol = float(np.linalg.norm(got - ref)), (C(nx) + ALLOWANCE) * EPS * majorant(w, dt, c)
    print(f"RATIO sensitivity[b]: error/bound {err / tol:.1f}")
    assert err > tol, (err, tol)


def test_right_hand_side_of_the_reference_is_the_formula():
    """the long-double (r, s) at one point, written out from the complex equation: A + dt (A - (1 + i c) |A|^2 A)"""
    nx, dt, c = 5, 0.05, -0.8
    w = np.random.default_rng(3).uniform(-1.0, 1.0, size=(2, nx, nx))
    r, s = right_hand_side(w, dt, c)
    A = w[0][2][3] + 1j * w[1][2][3]
    want = A + dt * (A - (1.0 + 1j * c) * abs(A) ** 2 * A)
    assert abs(float(r[2][3]) - want.real) <= 8 * EPS and abs(float(s[2][3]) - want.imag) <= 8 * EPS


def test_reference_matches_a_dense_complex_solve():
    """nx = 6: the scheme in complex arithmetic -- (I - dt (1 + i b) Lap) A_new = A + dt (A - (1 + i c) |A|^2 A) with Lap a dense 36 x 36
    matrix written out index by index -- and np.linalg.solve. The matrix is normal with singular values in [1, |1 + 8 rr (1 + i b)|], so the
    solve is off by about 8 n EPS cond norm (Gaussian elimination, n = 36) and the right-hand side by a few EPS M:
    allowed (8 n cond + 8 + ALLOWANCE) EPS M"""
    nx, b, c, dt = 6, 1.5, -0.8, 0.1
    w = np.random.default_rng(6).uniform(-1.0, 1.0, size=(2, nx, nx))
    lap = np.zeros((nx * nx, nx * nx))
    for i in range(nx):
        for j in range(nx):
            p = i * nx + j
            lap[p, p] -= 4.0
            for q in (((i + 1) % nx) * nx + j, ((i - 1) % nx) * nx + j, i * nx + (j + 1) % nx, i * nx + (j - 1) % nx):
                lap[p, q] += 1.0
    A = (w[0] + 1j * w[1]).ravel()
    rhs = A + dt * (A - (1.0 + 1j * c) * np.abs(A) ** 2 * A)
    new = np.linalg.solve(np.eye(nx * nx) - dt * (1.0 + 1j * b) * lap, rhs).reshape(nx, nx)      # dx = 1
    ref = reference_phi(w, dt, nx, b, c, float(nx))
    cond = abs(1.0 + 8.0 * dt * (1.0 + 1j * b))
    err, tol = float(np.linalg.norm(np.stack((new.real, new.imag)) - ref)), (8 * nx * nx * cond + 8 + ALLOWANCE) * EPS * majorant(w, dt, c)
    print(f"RATIO reference_vs_dense: error/bound {err / tol:.4f}")
    assert err <= tol, (err, tol)
    assert float(np.linalg.norm(ref - w)) > 1e6 * tol      # (and the step is not the identity at this size)


# ---- known answers -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [4, 33])
def test_zero_state_is_a_fixed_point_exactly(nx):
    app = make(nx, b=1.5, c=-0.8)
    got = apply_step(app, np.zeros((2, nx, nx)), 0.1)
    assert np.array_equal(got, np.zeros((2, nx, nx)))


@pytest.mark.parametrize("nx", [4, 33])
def test_constant_state_moves_by_the_pointwise_map_alone(nx):
    """A = p + i q everywhere: Lap A = 0, mode (0, 0) has Da = 1, Db = 0 and every other mode of a constant is 0 up to the products'
    rounding: Phi = (r, s) of that point within the per-Phi bound -- while the map itself moves the state by far more"""
    app = make(nx, b=1.5, c=-0.8)
    p, q, dt = 0.75, -0.5, 0.1
    w = np.stack((np.full((nx, nx), p), np.full((nx, nx), q)))
    r, s = app._rhs_imex(w[0], w[1], dt)
    m = p * p + q * q
    assert r[0, 0] == p + dt * (p - m * (p - app.c * q)) and s[0, 0] == q + dt * (q - m * (app.c * p + q))
    got = apply_step(app, w, dt)
    err, tol = float(np.linalg.norm(got - np.stack((r, s)))), C(nx) * EPS * majorant(w, dt, app.c)
    print(f"RATIO constant[nx={nx}]: error/bound {err / tol:.4f}")
    assert err <= tol, (err, tol)
    assert float(np.linalg.norm(got - w)) > 1e6 * tol


def plane_wave(nx, p, q, R):
    i1, i2 = np.meshgrid(np.arange(nx), np.arange(nx), indexing="ij")
    return R * np.exp(2j * np.pi * ((p * i1 + q * i2) % nx) / nx)


def plane_wave_answer(A, nx, dx, p, q, R, b, c, dt):
    """A (1 + dt (1 - (1 + i c) R^2)) / (1 + dt mu_pq (1 + i b)), mu_pq from the eigenvalues' definition in long double"""
    mu = float((LD(4) / LD(dx) ** 2) * (np.sin(LD(np.pi) * LD(p) / LD(nx)) ** 2 + np.sin(LD(np.pi) * LD(q) / LD(nx)) ** 2))
    return A * (1.0 + dt * (1.0 - (1.0 + 1j * c) * R * R)) / (1.0 + dt * mu * (1.0 + 1j * b))


@pytest.mark.parametrize("nx", [9, 33])
def test_plane_wave_is_an_eigenfunction(nx):
    """A = R exp(2 pi i (p i1 + q i2) / nx) has |A| = R everywhere and Lap A = -mu_pq A: one step multiplies it by
    (1 + dt (1 - (1 + i c) R^2)) / (1 + dt mu_pq (1 + i b)). b and c differ in size and sign and p != q: with b and c swapped, the sign of
    either flipped, or the axes swapped, the answer moves by orders of magnitude more than the bound, which is asserted.
    The formula's own rounding (a handful of complex operations on numbers of size <= M) is covered by 16 EPS M more"""
    p, q, R, b, c, dt = 2, 3, 0.7, 1.5, -0.8, 0.1
    app = make(nx, b=b, c=c)
    A = plane_wave(nx, p, q, R)
    w = np.stack((A.real, A.imag))
    got = apply_step(app, w, dt)
    got = got[0] + 1j * got[1]
    tol = (C(nx) + 16) * EPS * majorant(w, dt, c)
    err = float(np.linalg.norm(got - plane_wave_answer(A, nx, app.dx, p, q, R, b, c, dt)))
    print(f"RATIO plane_wave[nx={nx}]: error/bound {err / tol:.4f}")
    assert err <= tol, (err, tol)
    for what, wrong in (("b and c swapped", plane_wave_answer(A, nx, app.dx, p, q, R, c, b, dt)),
                        ("sign of b", plane_wave_answer(A, nx, app.dx, p, q, R, -b, c, dt)),
                        ("sign of c", plane_wave_answer(A, nx, app.dx, p, q, R, b, -c, dt)),
                        ("conjugate", np.conj(plane_wave_answer(A, nx, app.dx, p, q, R, b, c, dt))),
                        ("p and q swapped", plane_wave_answer(plane_wave(nx, q, p, R), nx, app.dx, q, p, R, b, c, dt))):
        miss = float(np.linalg.norm(got - wrong))
        print(f"RATIO plane_wave[nx={nx}] {what}: miss/bound {miss / tol:.3e}")
        assert miss > 1e6 * tol, (what, miss, tol)


@pytest.mark.parametrize("nx", [8, 33])
def test_real_limit_follows_allen_cahn(nx):
    """b = c = 0 and a zero imaginary plane: s = 0 exactly, Db = 0 exactly, the imaginary plane stays 0 exactly and the real plane is
    AllenCahn(nu=2, eps=1, method='IMEX') on the same grid (dx = 1 / nx): x + dt (x - x^3), then (I - dt Lap)^-1. Both steps are within
    their own bound of the exact answer: (C(nx) + 4 nx + 8) EPS M (test_allen_cahn_cpu.py: (4 nx + 8) EPS norm_F(b), norm_F(b) <= M)"""
    from pymgrit_amd import AllenCahn, VectorAllenCahn2D
    dt = 0.1 / nx ** 2
    app = make(nx, b=0.0, c=0.0, L=1.0)
    assert table_condition(app, dt) <= 0.25
    ac = AllenCahn(nx=nx, nu=2, eps=1.0, method="IMEX", t_start=0, t_stop=1, nt=2)
    assert ac.dx == app.dx
    u = np.random.default_rng(nx).uniform(-1.0, 1.0, size=(nx, nx))
    w = np.stack((u, np.zeros((nx, nx))))
    got = apply_step(app, w, dt)
    assert np.array_equal(got[1], np.zeros((nx, nx)))
    vec = VectorAllenCahn2D(nx, nx)
    vec.set_values(u.copy())
    want = np.asarray(ac.step(vec, 0.0, dt).get_values())
    err, tol = float(np.linalg.norm(got[0] - want)), (C(nx) + 4 * nx + 8) * EPS * majorant(w, dt, 0.0)
    print(f"RATIO real_limit[nx={nx}]: error/bound {err / tol:.4f}")
    assert err <= tol, (err, tol)
    assert float(np.linalg.norm(want - u)) > 1e3 * tol


def test_dinv_is_the_inverse_of_the_modal_block():
    """[[Da, Db], [-Db, Da]] [[a, -beta], [beta, a]] = I per mode, Da^2 + Db^2 = 1 / det <= 1, and mode (0, 0) has Da = 1, Db = 0"""
    app = make(9, b=1.5, c=-0.8)
    apply_step(app, np.zeros((2, 9, 9)), 0.1)      # (builds the eigenvalues)
    Da, Db = app._dinv(0.1)
    mu = app._lam[:, None] + app._lam[None, :]
    a, beta = 1.0 + 0.1 * mu, 1.5 * 0.1 * mu
    assert Da[0, 0] == 1.0 and Db[0, 0] == 0.0
    assert np.max(np.abs(Da * a + Db * beta - 1.0)) <= 8 * EPS and np.max(np.abs(Db * a - Da * beta)) <= 8 * EPS
    assert np.all(Da * Da + Db * Db <= 1.0)


# ---- the vector, the transfer, the constructor ----------------------------------------------------------------------------------------
def test_vector_interface():
    from pymgrit_amd import Vector, VectorGinzburgLandau2D
    nx = 5
    rng = np.random.default_rng(0)
    a, b = VectorGinzburgLandau2D(nx), VectorGinzburgLandau2D(nx)
    va, vb = rng.normal(size=(2, nx, nx)), rng.normal(size=(2, nx, nx))
    a.set_values(va.copy()), b.set_values(vb.copy())
    assert isinstance(a, Vector) and a.get_values().shape == (2, nx, nx)
    assert np.array_equal((a + b).get_values(), va + vb) and np.array_equal((a - b).get_values(), va - vb)
    assert np.array_equal((a * 2.5).get_values(), va * 2.5)
    assert a.norm() == np.linalg.norm(va.ravel())       # the 2-norm over all 2 nx^2 values
    c = a.clone()
    c.get_values()[0, 0, 0] += 1.0
    assert np.array_equal(a.get_values(), va)            # a clone owns its values
    z = a.clone_zero()
    assert isinstance(z, VectorGinzburgLandau2D) and z.get_values().shape == (2, nx, nx) and not z.get_values().any()
    r = a.clone_rand()
    assert r.get_values().shape == (2, nx, nx) and 0.0 <= r.get_values().min() and r.get_values().max() < 1.0
    z.unpack(np.asarray(a.pack()).copy())
    assert np.array_equal(z.get_values(), va)
    assert np.array_equal(np.asarray(a.pack()).ravel()[:nx * nx], va[0].ravel())      # a device row is [real plane | imaginary plane]


def _vec(values):
    from pymgrit_amd import VectorGinzburgLandau2D
    v = VectorGinzburgLandau2D(values.shape[1])
    v.set_values(values)
    return v


def test_transfer_python_methods():
    """9-point full weighting and bilinear interpolation per plane: the weights of a row sum to 1 (constants are reproduced, each plane
    its own), plane c of the result depends on plane c of the argument alone, and the planes are GridTransferAllenCahn's bit for bit"""
    from pymgrit_amd import GridTransferAllenCahn, GridTransferGinzburgLandau, VectorAllenCahn2D, VectorGinzburgLandau2D
    from pymgrit_amd.core import hip_lib
    tr, one = GridTransferGinzburgLandau(), GridTransferAllenCahn()
    assert tr.device_transfer() == hip_lib.TRANSFER_PERIODIC2D
    nf, nc = 12, 6
    rng = np.random.default_rng(4)
    for method, n_in, n_out in ((tr.restriction, nf, nc), (tr.interpolation, nc, nf)):
        const = np.stack((np.full((n_in, n_in), 0.75), np.full((n_in, n_in), -1.25)))
        out = method(_vec(const))
        assert isinstance(out, VectorGinzburgLandau2D) and out.get_values().shape == (2, n_out, n_out)
        assert np.max(np.abs(out.get_values()[0] - 0.75)) <= 4 * EPS and np.max(np.abs(out.get_values()[1] + 1.25)) <= 4 * EPS
        w = rng.uniform(-1.0, 1.0, size=(2, n_in, n_in))
        base = np.asarray(method(_vec(w.copy())).get_values())
        other = w.copy()
        other[1] = rng.uniform(-1.0, 1.0, size=(n_in, n_in))
        moved = np.asarray(method(_vec(other)).get_values())
        assert np.array_equal(moved[0], base[0]) and not np.array_equal(moved[1], base[1])
        single = getattr(one, method.__name__)
        for c in range(2):
            plane = VectorAllenCahn2D(n_in, n_in)
            plane.set_values(w[c].copy())
            assert np.array_equal(base[c], np.asarray(single(plane).get_values()))
    # the row sums themselves: the image of a unit impulse plane sums to 1 (restriction) / 4 (interpolation, four fine points per coarse)
    unit = np.zeros((2, nf, nf))
    unit[0, 3, 4] = 1.0
    assert abs(float(np.sum(tr.restriction(_vec(unit)).get_values()[0])) - 0.25) <= 4 * EPS      # column sums of full weighting: 1 / 4
    unit = np.zeros((2, nc, nc))
    unit[1, 2, 5] = 1.0
    assert abs(float(np.sum(tr.interpolation(_vec(unit)).get_values()[1])) - 4.0) <= 16 * EPS
    with pytest.raises(Exception, match="GridTransferGinzburgLandau restricts"):
        tr.restriction(_vec(np.zeros((2, 7, 7))))


def test_initial_guess():
    app = make(12, L=6.0)
    w = np.asarray(app.vector_t_start.get_values())
    assert w.shape == (2, 12, 12) and np.array_equal(w, np.asarray(make(12, L=6.0).vector_t_start.get_values()))      # not random
    k = 2.0 * np.pi / 6.0
    for i in range(12):
        for j in range(12):
            x, y = i * app.dx, j * app.dx
            A = 0.1 * (np.cos(k * x) + 1j * np.sin(k * (x + 2.0 * y))) + 0.05 * np.cos(2.0 * k * y)
            assert abs(w[0, i, j] - A.real) <= 4 * EPS and abs(w[1, i, j] - A.imag) <= 4 * EPS, (i, j)
    assert np.abs(w).max() <= 0.2 and np.ptp(w[0]) > 0.1 and np.ptp(w[1]) > 0.1
    own = make(8, init=lambda X, Y: (X + 2.0 * Y) * (1.0 - 0.5j))
    v = np.asarray(own.vector_t_start.get_values())
    assert v[0, 3, 2] == 3.0 + 2.0 * 2.0 and v[1, 3, 2] == -0.5 * (3.0 + 2.0 * 2.0)      # X[i][j] = x_i, Y[i][j] = y_j, dx = 1
    with pytest.raises(Exception, match="init must return"):
        make(8, init=lambda X, Y: np.zeros(3))


def test_constructor_defaults_and_refusals():
    from pymgrit_amd import GinzburgLandau2D
    app = GinzburgLandau2D(t_start=0, t_stop=0.5, nt=3)
    assert (app.nx, app.b, app.c, app.method) == (64, 1.0, -1.2, "IMEX") and app.dx == app.L / 64
    for method in ("IMPL", "EXPL", "nope", None):
        with pytest.raises(Exception, match="Unknown method"):
            make(8, method=method)
    for bad in (0, -4, 8.5, "eight", None):
        with pytest.raises(Exception, match="nx"):
            GinzburgLandau2D(nx=bad, t_start=0, t_stop=1, nt=2)
    for bad in (dict(b=float("nan")), dict(b=float("inf")), dict(c=float("nan")), dict(c=-float("inf")), dict(b="x"), dict(L=0.0),
                dict(L=float("inf"))):
        with pytest.raises(Exception, match="b and c must be finite"):
            make(8, **bad)
    with pytest.raises(Exception, match="init must be a callable"):
        make(8, init=3.0)
    assert make(4).nx == 4 and make(8.0).nx == 8 and isinstance(make(8.0).nx, int)


def test_device_description():
    app = make(20, b=1.5, c=-0.8, L=10.0)
    assert app.device_stepper() == {"kind": "ginzburglandau2d", "n": 800, "nx": 20, "inv_dx2": 1.0 / app.dx ** 2, "b": 1.5, "c": -0.8}


def test_package_exports_and_backend_rows():
    import pymgrit_amd
    from pymgrit_amd.core import backend_hip, hip_lib
    for name in ("GinzburgLandau2D", "VectorGinzburgLandau2D", "GridTransferGinzburgLandau"):
        assert name in pymgrit_amd.__all__ and hasattr(pymgrit_amd, name)
    assert hip_lib.STEPPER_GINZBURGLANDAU2D == 10 and "mgrit_hip_level_ginzburglandau2d" in hip_lib.EXPORTS
    name, _, library_only, own = backend_hip.PERIODIC_2D["ginzburglandau2d"]
    assert name == "Ginzburg-Landau" and library_only is True and own[1] == "GridTransferGinzburgLandau"
    assert "ginzburglandau2d" in backend_hip.HipBackend._DESCRIBE and "ginzburglandau2d" in backend_hip.GRID_2D
    from pymgrit_amd.ginzburg_landau.ginzburg_landau import GinzburgLandau2D
    assert pymgrit_amd.GinzburgLandau2D is GinzburgLandau2D


def test_two_plane_transfer_rules_hold_for_the_kind():
    """_check_periodic refuses for this kind what it refuses for Gray-Scott and Burgers (no GPU needed: the check is plain Python)"""
    import types
    from pymgrit_amd import GridTransfer, GridTransferBurgers, GridTransferCopy, GridTransferGinzburgLandau
    from pymgrit_amd.core.backend_hip import HipBackend
    from pymgrit_amd.core.hip_lib import MgritHipError
    name = "Ginzburg-Landau levels on the HIP engine"

    def stub(nxs):
        return types.SimpleNamespace(desc=[make(nx).device_stepper() for nx in nxs])

    def mg(transfers, **kw):
        return types.SimpleNamespace(comm_time_size=kw.get("ranks", 1), global_conv_crit=kw.get("glob", True), transfer_objects=transfers)

    class Mine(GridTransfer):
        def restriction(self, u):
            return u

        def interpolation(self, u):
            return u
    HipBackend._check_periodic(stub((12, 12)), mg([GridTransferCopy()]), "ginzburglandau2d")
    HipBackend._check_periodic(stub((12, 6)), mg([GridTransferGinzburgLandau()]), "ginzburglandau2d")
    with pytest.raises(MgritHipError, match=name + ".*same nx"):
        HipBackend._check_periodic(stub((12, 6)), mg([Mine()]), "ginzburglandau2d")
    with pytest.raises(MgritHipError, match=name + ": GridTransferCopy only"):
        HipBackend._check_periodic(stub((12, 12)), mg([Mine()]), "ginzburglandau2d")
    with pytest.raises(MgritHipError, match=name + ".*not this application's transfer"):
        HipBackend._check_periodic(stub((12, 6)), mg([GridTransferBurgers()]), "ginzburglandau2d")
    with pytest.raises(MgritHipError, match=name + ": one time rank only"):
        HipBackend._check_periodic(stub((12, 12)), mg([GridTransferCopy()], ranks=2), "ginzburglandau2d")
    with pytest.raises(MgritHipError, match=name + ": the global convergence criteria only"):
        HipBackend._check_periodic(stub((12, 12)), mg([GridTransferCopy()], glob=False), "ginzburglandau2d")


# ---- a plugin-path solve ---------------------------------------------------------------------------------------------------------------
def _host_class():
    from pymgrit_amd import GinzburgLandau2D

    class HostGinzburgLandau2D(GinzburgLandau2D):     # overriding step sends the hierarchy to the plugin path
        def step(self, u_start, t_start, t_stop):
            return super().step(u_start, t_start, t_stop)
    return HostGinzburgLandau2D


def test_plugin_path_solve_converges_and_matches_the_solve_over_the_reference_step():
    """Mgrit over the host step against Mgrit over reference_phi from the initial guess (nx = 12, L = 12, [0, 2], nt 17 / 9 / 5): both reach
    1e-10 within max_iter, the residual histories agree by the project's rule (tests/cases.py)"""
    from pymgrit_amd import Mgrit
    logging.disable(logging.WARNING)
    try:
        ours = Mgrit([make(12, cls=_host_class(), b=1.5, c=-0.8, t_stop=2.0, nt=nt) for nt in (17, 9, 5)], tol=1e-10, max_iter=15, logging_lvl=30)
        ref = Mgrit([make(12, cls=ReferenceGinzburgLandau2D, b=1.5, c=-0.8, t_stop=2.0, nt=nt) for nt in (17, 9, 5)], tol=1e-10, max_iter=15,
                    logging_lvl=30)
        assert type(ours.backend).__name__ == type(ref.backend).__name__ == "PluginBackend"
        conv, rconv = np.asarray(ours.solve()["conv"]), np.asarray(ref.solve()["conv"])
    finally:
        logging.disable(logging.NOTSET)
    norm_u = cases.spacetime_norm([v.get_values() for v in ours.u[0]])
    print(f"solve: {len(rconv)} iterations, conv {rconv}")
    assert len(conv) == len(rconv) < 15 and rconv[-1] < 1e-10, (conv, rconv)
    dev = np.abs(conv - rconv)
    print(f"RATIO solve conv: largest deviation {np.max(dev) / (EPS * norm_u):.2f} units of eps*norm(u) (allowed {cases.BLK_K})")
    assert np.all(dev <= 1e-10 * rconv + cases.BLK_K * EPS * norm_u), (conv, rconv)
    last = np.asarray(ours.u[0][-1].get_values())
    assert float(np.linalg.norm(last - np.asarray(ours.u[0][0].get_values()))) > 1e-3      # (the state moved)
