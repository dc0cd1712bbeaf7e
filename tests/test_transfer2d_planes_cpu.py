"""CPU: the transfers of the two applications whose state is two planes, GridTransferGrayScott and GridTransferBurgers:
GridTransferAllenCahn's arithmetic on each plane on its own, the plugin path over them, and the rule by which HipBackend._check_periodic
accepts or refuses a Gray-Scott / Burgers hierarchy (the device side: tests/test_hip_transfer2d_planes.py)."""
import types

import numpy as np
import pytest

from pymgrit_amd import (Burgers2D, GrayScott, GridTransfer, GridTransferAllenCahn, GridTransferBurgers, GridTransferCopy,
                         GridTransferGrayScott, Mgrit, VectorAllenCahn2D, VectorBurgers2D, VectorGrayScott2D)

KINDS = {"grayscott": (GridTransferGrayScott, VectorGrayScott2D), "burgers": (GridTransferBurgers, VectorBurgers2D)}


def _vec(cls, values):
    out = cls(values.shape[1])
    out.set_values(values)
    return out


def _plane(values):
    out = VectorAllenCahn2D(*values.shape)
    out.set_values(values)
    return out


@pytest.mark.parametrize("nx", [4, 12, 66])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_each_plane_is_the_allen_cahn_transfer_of_that_plane_alone(kind, nx):
    tr_cls, vec_cls = KINDS[kind]
    tr, one = tr_cls(), GridTransferAllenCahn()
    rng = np.random.default_rng(nx)
    for method, size, out_nx in (("restriction", nx, nx // 2), ("interpolation", nx // 2, nx)):
        values = rng.uniform(-1.0, 1.0, size=(2, size, size))
        got = getattr(tr, method)(_vec(vec_cls, values.copy()))
        assert type(got) is vec_cls and got.nx == out_nx
        res = np.asarray(got.get_values())
        assert res.shape == (2, out_nx, out_nx) and res.dtype == np.float64
        for c in range(2):
            assert np.array_equal(res[c], np.asarray(getattr(one, method)(_plane(values[c].copy())).get_values()))
        for c in range(2):      # another plane c: the other plane of the result keeps every bit
            changed = values.copy()
            changed[c] = rng.uniform(-1.0, 1.0, size=(size, size))
            res2 = np.asarray(getattr(tr, method)(_vec(vec_cls, changed)).get_values())
            assert np.array_equal(res2[1 - c], res[1 - c]) and not np.array_equal(res2[c], res[c])


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_constant_planes_are_kept_exactly(kind):
    tr_cls, vec_cls = KINDS[kind]
    tr = tr_cls()
    for nx in (4, 12, 66):
        for method, size, out_nx in (("restriction", nx, nx // 2), ("interpolation", nx // 2, nx)):
            values = np.stack((np.full((size, size), 0.5), np.full((size, size), -3.0)))
            res = np.asarray(getattr(tr, method)(_vec(vec_cls, values)).get_values())
            assert np.array_equal(res, np.stack((np.full((out_nx, out_nx), 0.5), np.full((out_nx, out_nx), -3.0))))


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_bad_input_raises(kind):
    tr_cls, vec_cls = KINDS[kind]
    tr = tr_cls()

    def holding(values):
        out = vec_cls(4)
        out.set_values(values)
        return out
    for nx in (5, 13):       # odd fine sizes
        with pytest.raises(Exception, match="even periodic fine grids"):
            tr.restriction(_vec(vec_cls, np.zeros((2, nx, nx))))
    for shape in ((8, 8), (1, 8, 8), (3, 8, 8), (2, 8, 6), (2, 64), (2, 2, 8, 8)):
        for method in (tr.restriction, tr.interpolation):
            with pytest.raises(Exception, match=r"\(2, nx, nx\)"):
                method(holding(np.zeros(shape)))


# ---- the plugin path -----------------------------------------------------------------------------------------------------------------
def _host(problems):
    for p in problems:
        p.device_stepper = lambda: None      # as tests/test_hip_transfer2d.py::heat_problem(host=True): the host steppers
    return problems


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_plugin_path_solves_a_spatially_coarsened_hierarchy(kind):
    if kind == "burgers":
        prob = [Burgers2D(nx=nx, t_start=0, t_stop=0.25, nt=nt) for nx, nt in ((16, 17), (8, 5))]
    else:
        prob = [GrayScott(nx=nx, method="IMEX", t_start=0, t_stop=0.5, nt=nt) for nx, nt in ((16, 17), (8, 5))]
    mg = Mgrit(problem=_host(prob), transfer=[KINDS[kind][0]()], logging_lvl=30, nested_iteration=False, max_iter=5, tol=0.0)
    assert type(mg.backend).__name__ == "PluginBackend"
    conv = np.asarray(mg.solve()["conv"])
    print(kind, "residual history", conv)
    assert len(conv) == 5 and np.all(np.isfinite(conv))
    # four coarse intervals: the two-level method is a direct solve at the fourth iteration, the residual is rounding from then on
    assert conv[3] <= 1e-10 * conv[0]
    last = mg.u[0][-1]
    assert type(last) is KINDS[kind][1] and np.asarray(last.get_values()).shape == (2, 16, 16) and np.all(np.isfinite(last.get_values()))


# ---- HipBackend._check_periodic: what a Gray-Scott / Burgers hierarchy is made of ------------------------------------------------------
CHECKED = {"grayscott": ("grayscott2d", "Gray-Scott", GridTransferGrayScott, GridTransferBurgers),
           "burgers": ("burgers2d", "Burgers", GridTransferBurgers, GridTransferGrayScott)}


def _check(kind, nxs, transfers, **mg):
    from pymgrit_amd.core.backend_hip import HipBackend
    stub = types.SimpleNamespace(desc=[{"kind": kind, "nx": nx, "n": 2 * nx * nx} for nx in nxs])
    world = dict(comm_time_size=1, global_conv_crit=True, transfer_objects=list(transfers))
    world.update(mg)
    HipBackend._check_periodic(stub, types.SimpleNamespace(**world), kind)


class UsersTransfer(GridTransfer):      # derives from no library class: a user's own
    def restriction(self, u):
        return u

    def interpolation(self, u):
        return u


@pytest.mark.parametrize("app", sorted(CHECKED))
def test_check_periodic_accepts(app):
    kind, _, own, _ = CHECKED[app]

    class ViaPython(own):      # a subclass: its Python methods between the kernels
        def restriction(self, u):
            return super().restriction(u)

        def interpolation(self, u):
            return super().interpolation(u)
    _check(kind, [12, 12], [GridTransferCopy()])
    _check(kind, [12, 6], [own()])
    _check(kind, [12, 6], [ViaPython()])
    _check(kind, [20, 10, 10], [own(), GridTransferCopy()])
    _check(kind, [20, 20, 10, 5], [GridTransferCopy(), ViaPython(), own()])


@pytest.mark.parametrize("app", sorted(CHECKED))
def test_check_periodic_refuses_by_name(app):
    from pymgrit_amd.core.hip_lib import MgritHipError
    kind, name, own, other = CHECKED[app]
    head = name + " levels on the HIP engine: "
    # a user's own GridTransfer: the wording the applications' tests pin
    with pytest.raises(MgritHipError, match=head + ".*UsersTransfer.*12 and 6.*same nx"):
        _check(kind, [12, 6], [UsersTransfer()])
    with pytest.raises(MgritHipError, match=head + r"GridTransferCopy only.*\(12\).*UsersTransfer"):
        _check(kind, [12, 12], [UsersTransfer()])
    # the other kind's class, and the one-plane class
    for cls in (other, GridTransferAllenCahn):
        with pytest.raises(MgritHipError, match=head + f"{cls.__name__} between levels of nx 12 and 6 is not this application's"):
            _check(kind, [12, 6], [cls()])
        with pytest.raises(MgritHipError, match=head + f"GridTransferCopy only.*not {cls.__name__}"):
            _check(kind, [12, 12], [cls()])
    # the library class between levels whose nx is not halved
    for nxs in ([12, 12], [12, 5], [12, 8], [6, 12]):
        with pytest.raises(MgritHipError, match=head + f"{own.__name__}.*nx_fine = 2 \\* nx_coarse, not nx {nxs[0]} and {nxs[1]}"):
            _check(kind, nxs, [own()])
    with pytest.raises(MgritHipError, match=head + f"{own.__name__}.*not nx 10 and 10"):
        _check(kind, [20, 10, 10], [own(), own()])
    # GridTransferCopy between levels of different nx
    with pytest.raises(MgritHipError, match=head + "GridTransferCopy joins levels of the same nx, not nx 12 and 6"):
        _check(kind, [12, 6], [GridTransferCopy()])
    with pytest.raises(MgritHipError, match=head + "GridTransferCopy joins levels of the same nx, not nx 10 and 5"):
        _check(kind, [20, 10, 5], [own(), GridTransferCopy()])
    # what stays refused as it is, with an accepted spatial coarsening in the hierarchy
    with pytest.raises(MgritHipError, match=head + "one time rank only"):
        _check(kind, [12, 6], [own()], comm_time_size=2)
    with pytest.raises(MgritHipError, match=head + "the global convergence criteria only"):
        _check(kind, [12, 6], [own()], global_conv_crit=False)
    other_kind = CHECKED["burgers" if app == "grayscott" else "grayscott"][0]
    from pymgrit_amd.core.backend_hip import HipBackend
    mixed = types.SimpleNamespace(desc=[{"kind": kind, "nx": 12}, {"kind": other_kind, "nx": 6}])
    with pytest.raises(MgritHipError, match=head + "every level of the hierarchy must be"):
        HipBackend._check_periodic(mixed, types.SimpleNamespace(comm_time_size=1, global_conv_crit=True, transfer_objects=[own()]), kind)


def test_at_mgrit_stays_refused_with_the_library_transfer():
    from pymgrit_amd import AtMgrit
    from pymgrit_amd.core.backend_hip import HipBackend
    from pymgrit_amd.core.hip_lib import MgritHipError
    stub = types.SimpleNamespace(desc=[{"kind": "burgers2d", "nx": nx} for nx in (12, 6)])
    at = AtMgrit.__new__(AtMgrit)      # (no constructor: the check reads the three attributes and the type)
    at.comm_time_size, at.global_conv_crit, at.transfer_objects = 1, True, [GridTransferBurgers()]
    with pytest.raises(MgritHipError, match="Burgers levels on the HIP engine: AT-MGRIT is not supported"):
        HipBackend._check_periodic(stub, at, "burgers2d")


def test_the_classes_are_exported_and_name_the_periodic_device_transfer():
    import pymgrit_amd
    from pymgrit_amd.core import hip_lib
    for name in ("GridTransferGrayScott", "GridTransferBurgers"):
        assert name in pymgrit_amd.__all__ and hasattr(pymgrit_amd, name)
        assert getattr(pymgrit_amd, name)().device_transfer() == hip_lib.TRANSFER_PERIODIC2D
