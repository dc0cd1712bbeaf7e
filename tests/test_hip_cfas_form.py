"""GPU: the two forms of the level-0 way down (include/mgrit_hip.h, mgrit_hip_set_cfas_form / mgrit_hip_cfas_form). With pre-relaxed
C-points and one separable forcing term mgrit_hip_cf_fas keeps the forcing space factor in LDS and q = Phi_{l+1}(C'_j) in
registers (cfasq_kernel); everything else, and everything with the switch off, runs cfas_kernel. Both store the same rows with the
same bits, so every run is compared bit for bit with the same sequence under mgrit_hip_set_cfas_form(h, 0) in the same process,
and against the oracle; which form ran is read from the library after every launch.

Hierarchy: Heat1D, 3 levels, m = 4, nt = 257 (64 level-0 intervals, 16 coarsest steps) at one state size per kernel instance,
nt = 273 (68 intervals: chunks of 16 leave a last chunk of 4) and nt = 1025 (a coarsest level of four blocks). The library's rule
gives levels this small chunks of ONE interval, so the tests ask for chunks of 4 (or 16): the closing C-point then stays in
registers as the next interval's start, as on the levels the form is made for."""
import ctypes as C

import numpy as np
import pytest

import cases
import heat1d_cycles as hc
from heat1d_cycles import SIZES, need_gpu, same, raw_cycle as cycle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ONE = [(cases.rhs_space, cases.rhs_time)]
TWO = cases.BDF_FORCING["two"]
NAME = "mgrit_hip_cf_fas"


def grids(nt):
    t = cases.lin(2, nt)
    return [t, t[::4], t[::16]]


def grids_two_dt():
    """257 points, the step size changes at point 74: inside level-0 interval 18 (points 72..76, the third of the chunk of
    intervals 16..19), and as a step made of both sizes at step 19 of level 1 -- the coarse Phi of that very interval -- and at
    step 5 of level 2: the coefficient set of either level changes inside a chunk"""
    t = np.concatenate((np.linspace(0.0, 1.0, 75), 1.0 + np.linspace(0.0, 2.0, 183)[1:]))
    return [t, t[::4], t[::16]]


def note(lib, h, name, args):
    """behind every mgrit_hip_cf_fas of level 0: (pre_relaxed, mgrit_hip_cfas_form(level 0) after the call, was the stream
    capturing)"""
    if args[1] == 0:
        return int(args[3]), lib.mgrit_hip_cfas_form(h, 0), hc.capturing()


def probe(lib, h):
    return hc.Probe(lib, h, (NAME,), note)


def per_level(terms, n):
    """terms: None, a list of (space, time) pairs for every level, or a TUPLE of such lists, one per level"""
    return list(terms) if isinstance(terms, tuple) else [terms] * n


def problem(nx, terms, tgrids):
    from pymgrit_amd import Heat1D
    return [Heat1D(x_start=0, x_end=1, nx=nx, a=1, init_cond=cases.init_cond, t_interval=np.asarray(t),
                   **(dict(rhs_separable=tm) if tm else {})) for t, tm in zip(tgrids, per_level(terms, len(tgrids)))]


def specs(nx, terms, tgrids):
    x, _ = cases.heat_grid(nx)
    out = []
    for t, terms in zip(tgrids, per_level(terms, len(tgrids))):
        s = cases.heat_level_spec(nx, t, forcing=False)
        if terms:
            s["s"] = np.array([f(x) for f, _ in terms])
            s["tau"] = np.array([[g(tt) for tt in t] for _, g in terms])
        out.append(s)
    return out


def build(nx, terms, tgrids, form, chunk=4, defer=True, comm=None, **kw):
    """a solver whose level-0 passes walk chunks of `chunk` intervals, the form switch set as asked, its library handle probed"""
    mg = hc.build(problem(nx, terms, tgrids), env={"MGRIT_HIP_DEFER": None if defer else "0"}, chunk=chunk, comm=comm, probe=probe,
                  **dict(dict(max_iter=5, tol=0.0), **kw))
    assert mg.backend.lib.mgrit_hip_set_cfas_form(mg.backend.h, form) == 0
    return mg


def cycles(n, *args, **kw):
    mg = build(*args, **kw)
    out = [cycle(mg, it) for it in range(n)]
    out.append([mg.backend.natural("u", 0)])
    return mg, out


def forms(mg):
    return [f for _, f, _ in mg.backend.lib.log]


def pres(mg):
    return [p for p, _, _ in mg.backend.lib.log]


def against_oracle(oracle, mg, out, nx, terms, tgrids, n=5, **kw):
    hc.against_oracle(oracle, mg, out[-1][0], specs(nx, terms, tgrids), n, **kw)


def new_forms(f):
    return len(f) > 0 and all(x in (1, 2) for x in f)


@pytest.mark.parametrize("defer", [True, False], ids=["held", "stored"])
@pytest.mark.parametrize("nx", SIZES)
def test_five_cycles_equal_the_old_kernel_and_the_oracle(oracle, nx, defer):
    need_gpu()
    tg = grids(257)
    mg1, on = cycles(5, nx, ONE, tg, 1, defer=defer)
    mg0, off = cycles(5, nx, ONE, tg, 0, defer=defer)
    same(on, off, (nx, defer))
    # that it happened: the first cycle's C-points are not pre-relaxed, every later way down takes the new form
    assert pres(mg1) == [0, 1, 1, 1, 1] and pres(mg0) == [0, 1, 1, 1, 1]
    f = forms(mg1)
    assert f[0] == 0 and new_forms(f[1:]), f
    assert forms(mg0) == [0] * 5
    held = mg1.backend.lib.mgrit_hip_deferred(mg1.backend.h, 0)
    assert held == -1      # (the way up has cleared it; whether row ce was stored is the switch's business, compared above)
    against_oracle(oracle, mg1, on, nx, ONE, tg)


@pytest.mark.parametrize("terms", [None, TWO], ids=["noforcing", "two_terms"])
@pytest.mark.parametrize("nx", SIZES)
def test_other_forcing_keeps_the_old_kernel(oracle, nx, terms):
    need_gpu()
    tg = grids(257)
    mg, out = cycles(3, nx, terms, tg, 1, max_iter=3)
    assert pres(mg) == [0, 1, 1] and forms(mg) == [0, 0, 0], mg.backend.lib.log
    against_oracle(oracle, mg, out, nx, terms, tg, n=3)


def half_space(x):
    return 0.5 * cases.rhs_space(x)


def double_time(t):
    return 2.0 * cases.rhs_time(t)


@pytest.mark.parametrize("nx", SIZES)
def test_coarse_factor_from_lds_only_where_the_factors_are_equal(oracle, nx):
    """levels 1 and 2 carry half the space factor and twice the time factor: the same forcing, but another vector -- a coarse Phi
    that took the fine level's copy from LDS would be off by a factor of two. Form 1 there, form 2 where the factors are equal"""
    need_gpu()
    tg = grids(257)
    other = (ONE, [(half_space, double_time)], [(half_space, double_time)])
    mg1, on = cycles(4, nx, other, tg, 1, max_iter=4)
    mg0, off = cycles(4, nx, other, tg, 0, max_iter=4)
    same(on, off, nx)
    assert forms(mg1) == [0, 1, 1, 1] and forms(mg0) == [0] * 4
    against_oracle(oracle, mg1, on, nx, other, tg, n=4)
    mg2, _ = cycles(2, nx, ONE, tg, 1, max_iter=2)
    assert forms(mg2) == [0, 2]


@pytest.mark.parametrize("nx", SIZES)
def test_step_size_changes_inside_a_chunk(oracle, nx):
    need_gpu()
    tg = grids_two_dt()
    mg1, on = cycles(4, nx, ONE, tg, 1, max_iter=4)
    mg0, off = cycles(4, nx, ONE, tg, 0, max_iter=4)
    same(on, off, nx)
    assert new_forms(forms(mg1)[1:]) and forms(mg0) == [0] * 4
    against_oracle(oracle, mg1, on, nx, ONE, tg, n=4)


@pytest.mark.parametrize("nx,nt,chunk", [(1022, 273, 16), (16382, 273, 16), (4097, 257, 3), (1022, 1025, 16)])
def test_short_last_chunk(oracle, nx, nt, chunk):
    """68 intervals in chunks of 16 (a last chunk of 4), 64 in chunks of 3 (of 1), 256 in chunks of 16 with a coarsest level that
    is solved block by block"""
    need_gpu()
    tg = grids(nt)
    mg1, on = cycles(4, nx, ONE, tg, 1, chunk=chunk, max_iter=4)
    mg0, off = cycles(4, nx, ONE, tg, 0, chunk=chunk, max_iter=4)
    same(on, off, (nx, nt, chunk))
    assert new_forms(forms(mg1)[1:]) and forms(mg0) == [0] * 4
    against_oracle(oracle, mg1, on, nx, ONE, tg, n=4)


@pytest.mark.parametrize("name", ["F_cycle", "cf_iter2"])
def test_other_cycle_shapes(oracle, name):
    need_gpu()
    kw = {"F_cycle": dict(cycle_type='F'), "cf_iter2": dict(cf_iter=2)}[name]
    tg = grids(257)
    mg1, on = cycles(4, 4097, ONE, tg, 1, max_iter=4, **kw)
    mg0, off = cycles(4, 4097, ONE, tg, 0, max_iter=4, **kw)
    same(on, off, name)
    assert set(forms(mg0)) == {0}
    if name == "cf_iter2":      # a plain C-relaxation stands in front of the pass: never pre-relaxed
        assert set(pres(mg1)) == {0} and set(forms(mg1)) == {0}
    else:
        assert all((f in (1, 2)) == bool(p) for p, f, _ in mg1.backend.lib.log) and any(pres(mg1)), mg1.backend.lib.log
    against_oracle(oracle, mg1, on, 4097, ONE, tg, n=4, **kw)


@pytest.mark.parametrize("blocks", [1, 3])
def test_planned_cycles(blocks):
    """a planned cycle runs launch by launch twice, then as a captured graph: the form is chosen the same way inside a capture"""
    need_gpu()
    tg = grids(257)
    with hc.planned_graph():
        runs = [cycles(5, 4097, ONE, tg, form, **({} if blocks == 1 else dict(plan_blocks=blocks))) for form in (0, 1)]
    (mg0, off), (mg1, on) = runs
    same(on, off, blocks)
    assert set(forms(mg0)) == {0}
    log = mg1.backend.lib.log
    assert all((f in (1, 2)) == bool(p) for p, f, _ in log), log
    assert any(p == 1 and c for p, _, c in log) and any(p == 1 and not c for p, _, c in log), log


def test_loopback_ranks():
    """two ranks: the shard route calls mgrit_hip_cf_fas on a rank's complete intervals"""
    need_gpu()
    from pymgrit_amd.core.comm import run_loopback_ranks
    tg = grids(257)

    def run(form):
        def rank(comm):
            mg = build(1022, ONE, tg, form, comm=comm, max_iter=3)
            assert mg.backend.device_links
            mg.solve()
            mg.backend.sync()
            return mg.backend.lib.log, np.array(mg.conv), [mg.backend.natural(w, lvl) for lvl in (0, 1, 2) for w in "uvg" if w == "u" or lvl]
        world, got = run_loopback_ranks(2, rank)
        world.close()
        return got

    off, on = run(0), run(1)
    for r, ((log0, conv0, st0), (log1, conv1, st1)) in enumerate(zip(off, on)):
        assert np.array_equal(conv0, conv1), (r, conv0, conv1)
        for k, (a, b) in enumerate(zip(st0, st1)):
            assert np.array_equal(a, b), (r, k)
        assert log0 and {f for _, f, _ in log0} == {0}, log0
        assert all((f in (1, 2)) == bool(p) for p, f, _ in log1) and any(p for p, _, _ in log1), log1


def test_switch_environment_and_argument_checks(monkeypatch):
    need_gpu()
    tg = grids(257)
    mg = build(1022, ONE, tg, 1)
    lib, h = mg.backend.lib, mg.backend.h
    null = C.c_void_p(None)
    assert lib.mgrit_hip_cfas_form(null, 0) == -2 and lib.mgrit_hip_cfas_form(h, -1) == -2 and lib.mgrit_hip_cfas_form(h, 99) == -2
    assert lib.mgrit_hip_cfas_form(h, 1) == -1 and lib.mgrit_hip_cfas_form(h, 2) == -1
    assert lib.mgrit_hip_set_cfas_form(null, 1) != 0 and lib.mgrit_hip_set_cfas_form(h, 2) != 0 and lib.mgrit_hip_set_cfas_form(h, -1) != 0
    assert b"form" in lib.mgrit_hip_last_error()
    # the setter between two cycles: off for the third way down, on again for the fourth
    for it, form in enumerate((1, 1, 0, 1)):
        assert lib.mgrit_hip_set_cfas_form(h, form) == 0
        cycle(mg, it)
    f = forms(mg)
    assert f[0] == 0 and f[1] in (1, 2) and f[2] == 0 and f[3] in (1, 2), f
    # MGRIT_HIP_CFAS_FORM=0 where the engine is created: the old kernel until the setter says otherwise
    monkeypatch.setenv("MGRIT_HIP_CFAS_FORM", "0")
    from pymgrit_amd import Mgrit
    mg = Mgrit(problem(1022, ONE, tg), logging_lvl=30, max_iter=3, tol=0.0)
    monkeypatch.delenv("MGRIT_HIP_CFAS_FORM")
    assert mg.backend.lib.mgrit_hip_cfas_form(mg.backend.h, 0) in (-1, 0)
    mg.backend.lib = probe(mg.backend.lib, mg.backend.h)
    for it in range(2):
        cycle(mg, it)
    assert forms(mg) == [0, 0] and pres(mg) == [0, 1]
    assert mg.backend.lib.mgrit_hip_set_cfas_form(mg.backend.h, 1) == 0
    cycle(mg, 2)
    assert forms(mg)[2] in (1, 2)
