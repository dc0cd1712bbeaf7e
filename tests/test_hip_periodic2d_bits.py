"""The periodic 2-D device paths (Allen-Cahn IMEX and Newton-PCG, Gray-Scott IMEX and Newton-BiCGStab, Cahn-Hilliard, Burgers,
Navier-Stokes and Ginzburg-Landau IMEX) against the bits recorded in
tests/golden/periodic2d_bits.json by tests/golden/make_golden_periodic2d_bits.py: every sweep of the fixed cases of
tests/periodic2d_bits.py (its docstring says what they are chosen for; their parameters, grids and the ranges of their states come
from the kinds table, tests/periodic2d_kinds.py) leaves the same bytes in every slab, the same residual norms and the same Newton /
CG counts. The digest of the inputs covers every state uploaded, so a changed table entry fails here as a changed input. Equality only: no tolerance, no case skipped. The tests beside this one (test_hip_allen_cahn*.py,
test_hip_gray_scott*.py, test_hip_cahn_hilliard.py, test_hip_burgers.py, test_hip_navier_stokes.py, test_hip_ginzburg_landau.py) say that the arithmetic is right; this one says that it has not moved."""
import pytest

import cases
import periodic2d_bits as bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = cases.load_json("periodic2d_bits.json")


def test_the_record_covers_every_case():
    assert sorted(GOLDEN["cases"]) == sorted(bits.CASES)


@pytest.mark.parametrize("name", sorted(bits.CASES))
def test_every_sweep_leaves_the_recorded_bits(name):
    assert torch.cuda.is_available()
    want, got = GOLDEN["cases"][name], bits.run_case(name)
    assert got["inputs"] == want["inputs"], f"{name}: the seeded inputs differ from the recorded ones (numpy's generator or the time grids)"
    assert sorted(got["digests"]) == sorted(want["digests"])
    moved = [k for k in got["digests"] if got["digests"][k] != want["digests"][k]]
    print(f"{name}: {len(got['digests'])} digests, {len(moved)} differ")
    assert not moved, (f"{name}: {len(moved)} of {len(got['digests'])} digests differ, the first {moved[:6]}; "
                       f"recorded with '{GOLDEN['hipcc']}', this machine has '{bits.hipcc_version()}'")
