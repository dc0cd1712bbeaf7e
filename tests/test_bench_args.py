"""bench.py refuses arguments it cannot honour before anything touches a GPU: no timed step, or --dump-outputs on a run of
several processes."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("extra,message", [(["--steps", "0"], "--steps must be at least 1"),
                                           (["--gpus", "2", "--dump-outputs", "d"], "--dump-outputs: one GPU"),
                                           (["--emulate-solve", "4", "--dump-outputs", "d"], "--dump-outputs: one GPU")])
def test_bench_refuses(tmp_path, extra, message):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, capture_output=True, text=True, timeout=120,
                       cwd=tmp_path)
    assert r.returncode == 2 and message in r.stderr, r.stderr[-2000:]
    assert not os.listdir(tmp_path)
