"""The parts of the record tests' harness (heat1d_cycles.py) that decide whether those tests can see a difference at all: the
comparison, the probe and the environment of an engine's creation. No GPU, no library."""
import os
import types

import numpy as np
import pytest

import heat1d_cycles as hc

torch = pytest.importorskip("torch")
VAR = "HEAT1D_CYCLES_CPU_TEST_VARIABLE"


def next_up(x):
    return np.nextafter(x, np.inf)


def nested():
    return [[np.array([1.0, 2.0]), torch.tensor([3.0, 4.0], dtype=torch.float64)], [np.array([5.0])], np.array([6.0, 7.0])]


def test_same_passes_on_equal_nested_mixtures():
    hc.same(nested(), nested(), "equal")
    hc.same([], [], "empty")


def differs(a, b):
    with pytest.raises(AssertionError):
        hc.same(a, b, "differs")
    with pytest.raises(AssertionError):
        hc.same(b, a, "differs")


def test_same_fails_on_one_bit_in_an_array_leaf():
    b = nested()
    b[0][0][1] = next_up(b[0][0][1])
    differs(nested(), b)
    differs([np.array([1.0])], [np.array([next_up(1.0)])])


def test_same_fails_on_one_bit_in_a_tensor_leaf():
    b = nested()
    b[0][1][0] = float(next_up(3.0))
    assert b[0][1][0].item() != 3.0
    differs(nested(), b)
    differs([torch.tensor([1.0], dtype=torch.float64)], [torch.tensor([float(next_up(1.0))], dtype=torch.float64)])


def test_same_fails_on_a_length_mismatch_at_the_top_level():
    differs(nested(), nested()[:-1])
    differs(nested(), nested() + [np.array([8.0])])


def test_same_fails_on_a_length_mismatch_in_a_nested_list():
    b = nested()
    b[0] = b[0][:-1]
    differs(nested(), b)
    b = nested()
    b[1].append(np.array([5.0]))
    differs(nested(), b)


def stub():
    calls = []
    lib = types.SimpleNamespace(calls=calls, constant=7,
                                watched=lambda *args: calls.append(("watched", args)) or 11,
                                other=lambda *args: calls.append(("other", args)) or 13)
    return lib


def test_probe_logs_the_watched_name_after_the_call_and_returns_its_result():
    lib = stub()
    seen = []

    def note(lib_, h, name, args):
        seen.append(list(lib_.calls))        # what the library had been asked when the note was taken
        return name, h, args
    probe = hc.Probe(lib, "handle", ("watched",), note)
    assert probe.other(1, 2) == 13 and probe.log == [] and seen == []
    assert probe.watched(3, 4) == 11
    assert probe.log == [("watched", "handle", (3, 4))]
    assert seen == [[("other", (1, 2)), ("watched", (3, 4))]]
    assert lib.calls == [("other", (1, 2)), ("watched", (3, 4))]


def test_probe_passes_other_attributes_through_untouched():
    lib = stub()
    probe = hc.Probe(lib, "handle", ("watched",), lambda *a: a)
    assert probe.other is lib.other and probe.constant == 7 and probe.calls is lib.calls
    assert probe.watched is not lib.watched
    with pytest.raises(AttributeError):
        probe.missing


def test_probe_logs_nothing_when_note_returns_none():
    lib = stub()
    probe = hc.Probe(lib, "handle", ("watched",), lambda lib_, h, name, args: (name, args) if args[0] == 0 else None)
    assert probe.watched(1) == 11 and probe.log == []
    assert probe.watched(0) == 11 and probe.log == [("watched", (0,))]
    assert len(lib.calls) == 2


@pytest.fixture
def variable(monkeypatch):
    monkeypatch.delenv(VAR, raising=False)
    return VAR


def test_engine_env_restores_a_set_variable_when_the_body_raises(variable):
    os.environ[variable] = "before"
    with pytest.raises(RuntimeError):
        with hc.engine_env({variable: "inside"}):
            assert os.environ[variable] == "inside"
            raise RuntimeError
    assert os.environ[variable] == "before"


def test_engine_env_restores_an_unset_variable_when_the_body_raises(variable):
    with pytest.raises(RuntimeError):
        with hc.engine_env({variable: "inside"}):
            assert os.environ[variable] == "inside"
            raise RuntimeError
    assert variable not in os.environ


def test_engine_env_none_unsets_the_variable_inside_the_block(variable):
    os.environ[variable] = "before"
    with hc.engine_env({variable: None}):
        assert variable not in os.environ
    assert os.environ[variable] == "before"
    del os.environ[variable]
    with hc.engine_env({variable: None}):
        assert variable not in os.environ
    assert variable not in os.environ
    with hc.engine_env(()):
        pass


def test_engine_env_of_two_ranks_at_once_leaves_the_state_the_first_found(variable):
    """two holders of the same variable that overlap, as the engines of two loopback ranks do: the first to come is the first to go"""
    first, second = hc.engine_env({variable: "inside"}), hc.engine_env({variable: "inside"})
    first.__enter__()
    second.__enter__()
    first.__exit__(None, None, None)
    assert os.environ[variable] == "inside"      # (the second rank's engine is still being made)
    second.__exit__(None, None, None)
    assert variable not in os.environ
