"""run_loopback_ranks hands the caller the failure of a rank, not its consequence: a rank that raises aborts the world's barrier, and a
rank that is still waking up inside that barrier then ends with BrokenBarrierError. Which of the two is rank 0 depends on the scheduler
(seen once on a loaded machine in test_hip_transfer2d.py::test_allen_cahn_on_ranks_stays_refused); the caller's pytest.raises names the
failure."""
import threading

import pytest


def test_the_failure_is_raised_not_the_broken_barrier():
    from pymgrit_amd.core.comm import run_loopback_ranks

    def target(comm):
        if comm.rank == 0:
            raise threading.BrokenBarrierError      # what rank 0 ends with when rank 1 fails while rank 0 leaves the barrier
        raise ValueError("one time rank only")
    with pytest.raises(ValueError, match="one time rank only"):
        run_loopback_ranks(2, target, timeout=10)


def test_a_broken_barrier_alone_is_still_raised():
    from pymgrit_amd.core.comm import run_loopback_ranks

    def target(comm):
        raise threading.BrokenBarrierError
    with pytest.raises(threading.BrokenBarrierError):
        run_loopback_ranks(2, target, timeout=10)
