"""tests/test_gpu_unwritten_outputs.py WITHOUT a GPU, and the guard of its tables.

  * the tables of tests/unwritten.py against include/xclim_hip.h: every non-const pointer parameter of every compute entry point
    is an output operand of the tables or is listed as exempt, the exempt list names nothing but operands whose header comment
    says the caller's values are kept, and every compute entry point is reached by a programme of the sweep;
  * ``MockDevice.empty`` is zero-filled by default and poisoned when asked (SimDevice and ReplayDevice inherit it);
  * the mechanism tests and the sweep on the host simulation: the helpers of the GPU module on the SimDevice of
    tests/test_hostsim_cpu.py, and the module itself in a child pytest, four workers where pytest-xdist is installed.

What the simulation run leaves out (the GPU runs everything): the lengths x widths grids of the dense and of the grouped
programme are cut to five pairs in which every length and every width occurs (so every entry point of this library runs at every
width there, not at every width x length pair); the strided cases run at 65 cells only, those of more than 60 s on fibers
(the 31-day sliding-window trainings) not at all — xh_eqm_train_window / xh_dqm_train_window run in the "window_training"
programme at 3 cells; xh_adapt_freq (rocPRIM) and the chill and BIO1-BIO19 units (simulation libraries of their own:
tests/test_hostsim_units_cpu.py, which re-runs their poisoned GPU modules) are not in this
library."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tools"))

import stridedabi as S  # noqa: E402
import test_gpu_unwritten_outputs as G  # noqa: E402
import unwritten as U  # noqa: E402
from poisoned import POISON, pattern, unwritten  # noqa: E402
from test_hostsim_cpu import _child_run, sim  # noqa: E402,F401  (the module-scoped simulation device)

NOT_IN_THE_SHARED_SIMULATION = {"xh_adapt_freq", "xh_chill_hourly", "xh_chill_daily", "xh_bioclim"}
SIM_DENSE_SHAPES = [(1, 257), (7, 65), (366, 63), (800, 1), (1030, 3)]


# ------------------------------------------------------------------------------------------------ the tables
def output_parameters(path=S.HEADER):
    """{entry point: [names of its non-const pointer parameters]} of the header (the context aside): what a call can write."""
    return {name: [n for text, n in decl[1:] if "*" in text and "const" not in text.split("*")[0]]
            for name, decl in S.header_declarations(path).items()}


def test_plumbing_and_compute_entry_points_partition_the_header():
    assert U.PLUMBING <= set(S.PROTOS)
    assert len(U.compute_entry_points()) == len(S.PROTOS) - len(U.PLUMBING) >= 92
    assert {"xh_resample_reduce", "xh_bioclim", "xh_fill_synthetic"} <= set(U.compute_entry_points())


def test_every_output_parameter_is_swept_or_listed():
    params = output_parameters()
    assert params["xh_season"] == ["start_out", "end_out", "len_out"] and params["xh_bioclim"] == ["outputs", "which_out", "count_out"]
    assert params["xh_threshold_count"] == ["count_out", "valid_out"] and params["xh_spell_mask_multi"] == ["out"]
    for name in U.compute_entry_points():
        swept = {o.ptr for o in U.outputs_of(name)}
        listed = {op for (n, op) in U.EXEMPT if n == name}
        assert not (swept & listed), (name, swept & listed)
        assert params[name], f"{name}: a compute entry point without an output?"
        assert swept | listed == set(params[name]), (name, sorted(set(params[name]) - swept - listed), sorted((swept | listed) - set(params[name])))
    assert not (set(U.DENSE) - set(U.compute_entry_points()))


def test_only_operands_the_header_leaves_to_the_caller_are_exempt():
    """EXEMPT is a condition, not a measurement: each entry quotes the words of the entry point's header comment that leave part
    of the operand to the caller, and is an "rw" operand of tests/stridedabi.py (whose padded replay keeps the caller's values)."""
    header = re.sub(r"\s+", " ", re.sub(r"\n\s*\*(?!/)", " ", open(S.HEADER).read()))   # (comment lines joined, their leading stars dropped)
    rw = {(n, op.ptr) for n, ops in S.TABLE.items() for op in ops if op.mode == "rw"}
    assert set(U.EXEMPT) == rw
    for (name, operand), words in U.EXEMPT.items():
        assert operand in S.PROTOS[name]
        at = header.index(f"int {name}(")
        # (the block comment above the prototype — or above the pair of prototypes it documents; `/* host */` notes are not it)
        comment = [c for c in re.findall(r"/\*.*?\*/", header[:at]) if len(c) > 80][-1]
        assert words in comment, f"{name}.{operand}: the header comment does not say {words!r}"


@pytest.mark.parametrize("name", sorted(U.DENSE))
def test_dense_entry_names_parameters_of_the_prototype(name):
    params = S.PROTOS[name][1:]
    for out in U.DENSE[name]:
        assert out.ptr in params and (out.stride is None or out.stride in params), (name, out)
        for expr in (out.rows, out.width, out.dtype):
            if isinstance(expr, str) and expr not in S._DTYPES:
                names = set(compile(expr, name, "eval").co_names)
                assert names <= set(params), f"{name}: {expr!r} uses {sorted(names - set(params))}"
    assert not ({o.ptr for o in U.DENSE[name]} & {op.ptr for op in S.TABLE.get(name, ())}), "an operand belongs to one table"


def test_every_compute_entry_point_is_reached_by_a_programme():
    """The `reaches` of the strided cases and the declared reaches of this sweep's own programmes (each asserted in every run
    of its programme) are, together, every compute entry point of the header."""
    reached = set(G.DENSE_REACHES) | set(G.GROUPED_REACHES)
    for names in G.NEW_UNIT_REACHES.values():
        reached |= names
    assert set(G.NEW_UNIT_REACHES) <= set(G.NEW_UNIT_NAMES) == set(G.new_unit_programmes())
    # the programmes of the sweep's own module alone reach every compute entry point, at every width and length of the issue;
    # the strided cases (four cells and more, their own lengths) come on top
    assert reached == set(U.compute_entry_points()), (sorted(set(U.compute_entry_points()) - reached), sorted(reached - set(U.compute_entry_points())))
    assert set(G.WIDTHS) == {1, 3, 63, 65, 257} and set(G.LENGTHS) >= {1, 7, 366, 800} and any(1024 < T < 1100 for T in G.LENGTHS)
    assert {T for T, _ in SIM_DENSE_SHAPES} == set(G.LENGTHS) and {C for _, C in SIM_DENSE_SHAPES} == set(G.WIDTHS)
    seg = G.periods_with_gaps(800)
    assert seg[0] == seg[1] and seg[2] == seg[3] and seg[-2] == seg[-1] and (np.diff(seg) > 0).sum() == 3


# ------------------------------------------------------------------------------------------------ the mock allocator
def test_mock_empty_is_zero_by_default_and_poisoned_when_asked(tmp_path):
    from mock_device import MockDevice

    dev = MockDevice()
    assert dev.poison_empty is None
    for dtype in G.DTYPES:
        a = dev.empty((8, 37), dtype)
        assert a._alloc == a.nbytes and (a.get() == 0).all()
    dev.poison_empty = POISON
    for dtype in G.DTYPES:
        a = dev.empty((8, 37), dtype)
        assert (a.get() == pattern(dtype)).all() and unwritten(a.get()).all()
        assert (dev.wrap(a.ptr, (a._alloc,), np.uint8).get() == POISON).all()
        assert (dev.empty((1,), dtype)._alloc == 16) and (dev.zeros((8, 37), dtype).get() == 0).all()
        assert (dev.to_device(np.full(5, 3, dtype)).get() == 3).all()
    dev.poison_empty = None
    assert (dev.empty((3,), np.float64).get() == 0).all()


def test_replay_device_empty_keeps_its_exact_sizes_and_the_poison(sim):
    from tests.hostsim import simdevice

    dev = simdevice.ReplayDevice(sim.path, "no driver is started here", "no case directory either")
    a = dev.empty((3,), np.int32)
    assert dev._exact[a.ptr] == 12 and a._alloc == 16 and (a.get() == 0).all()
    dev.poison_empty = POISON
    b = dev.empty((5, 7), np.float32)
    assert dev._exact[b.ptr] == 140 and unwritten(b.get()).all()
    b.free()
    assert b.ptr == 0 and len(dev._exact) == 1


# ------------------------------------------------------------------------------------------------ on the simulation
def test_allocator_poisons_on_the_simulation(sim, monkeypatch):
    G.check_allocator_reuses_and_poisons(sim, monkeypatch)


def test_a_skipped_store_is_seen_on_the_simulation(sim, rng, monkeypatch):
    first, second = G.check_skipped_store_is_seen(sim, rng, monkeypatch)
    assert np.isfinite(first).any() and unwritten(second).all()
    assert not np.array_equal(first, second, equal_nan=True)


def test_the_watch_sees_an_output_that_is_not_written(sim, rng, monkeypatch):
    """The sweep's own check, on a no-op: an entry point that answers XH_OK without launching fails the watch, naming the operand."""
    monkeypatch.setattr(sim, "poison_empty", POISON)
    x, seg = G._reduction_inputs(rng)
    d = sim.to_device(x)
    real = sim.call
    monkeypatch.setattr(sim, "call", lambda name, *a: 0 if name == "xh_resample_reduce" else real(name, *a), raising=False)
    with U.watch(sim, monkeypatch):
        with pytest.raises(AssertionError, match=r"xh_resample_reduce: 111 of 111 elements of out \(3 x 37 float32\) were not written"):
            G.K.resample_reduce(sim, d, "mean", seg)


@pytest.mark.parametrize("T,C", SIM_DENSE_SHAPES)
def test_dense_outputs_are_written_on_the_simulation(sim, rng, monkeypatch, T, C):
    G.check_dense_programme(sim, rng, monkeypatch, T, C)


@pytest.mark.parametrize("T,C", SIM_DENSE_SHAPES)
def test_grouped_and_table_outputs_are_written_on_the_simulation(sim, rng, monkeypatch, T, C):
    G.check_grouped_programme(sim, rng, monkeypatch, T, C, rocprim=False)   # (xh_adapt_freq: rocPRIM, the GPU's)


def test_the_sweep_module_on_the_simulation(sim):
    """tests/test_gpu_unwritten_outputs.py in a child pytest on the simulation: the strided cases at 65 cells, the programmes of
    the newest units at every width (the module's docstring lists what is left out)."""
    cases = G.strided_cases()
    slow = ("eqm_doy_window", "dqm_doy_window")
    left_out = [n for n in cases if "xh_adapt_freq" in cases[n].reaches or n in slow]
    ids = [f"tests/test_gpu_unwritten_outputs.py::test_outputs_of_the_strided_cases_are_written[{n}-65]" for n in sorted(cases) if n not in left_out]
    units = [n for n in G.NEW_UNIT_NAMES if not (G.NEW_UNIT_REACHES.get(n, set()) & NOT_IN_THE_SHARED_SIMULATION)]
    ids += [f"tests/test_gpu_unwritten_outputs.py::test_outputs_of_the_newest_units_are_written[{n}-{C}]" for n in units
            for C in (G.WIDTHS if n != "window_training" else (3,))]
    ids += ["tests/test_gpu_unwritten_outputs.py::test_allocator_reuses_and_poisons", "tests/test_gpu_unwritten_outputs.py::test_a_skipped_store_is_seen"]
    reached = set(G.DENSE_REACHES) | (set(G.GROUPED_REACHES) - {"xh_adapt_freq"}) | {e for n in units for e in G.NEW_UNIT_REACHES.get(n, ())} | {e for n in cases if n not in left_out for e in cases[n].reaches}
    assert reached == set(U.compute_entry_points()) - NOT_IN_THE_SHARED_SIMULATION, sorted(set(U.compute_entry_points()) - NOT_IN_THE_SHARED_SIMULATION - reached)
    _child_run(sim, ids, at_least=len(ids))
