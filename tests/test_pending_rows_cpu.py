"""CPU: the ledger of unstored rows (pymgrit_amd/csrc/pending_rows.h) through its stand-alone check program
(tests/host/pending_rows_check.cpp), built with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer (runtimes linked in)
and run as a process of its own: the settle order against the order written out by hand at 2, 3 and 4 levels, the waiting rules on
scripted event sequences, the list predicates against brute force on 20000 random lists, the records' invariants on random event
sequences."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ledger_check_program_under_host_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "pending_rows_check")
    # the sanitizer runtimes linked into the program, so that it needs nothing of the process that starts it: GCC and clang spell that
    # differently
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True, timeout=60).stdout.lower()
    static = ["-static-libsan"] if "clang" in version else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all"] + static + ["-I", os.path.join(ROOT, "pymgrit_amd", "csrc"),
                            os.path.join(ROOT, "tests", "host", "pending_rows_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")      # (the leak check needs ptrace, which a container may not grant; every access is still checked)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and run.stdout.startswith("ok"), (run.stdout[-2000:], run.stderr[-3000:])
