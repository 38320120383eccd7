"""The launch plans of xclim_amd/sdba.py against tests/golden/sdba_plans.json (recorded by tests/golden/make_sdba_plans.py
BEFORE the module's group-major plumbing was shared): for every train / adjust / adapt_freq call of the case matrix — the three
mappings x the groupings x two calendars x interp / extrapolation / grouped_nearest / detrend, member axes, 40 nodes,
adapt_freq, the refusals and the forced fall-backs — the same ``xh_*`` entry points in the same order with the same scalar
arguments, host tables and NULL / shared pointers, the same number and bytes of uploads and downloads, the same exception or
warning, byte for byte.  Runs on tools/mock_device.MockDevice: the kernels are no-ops, the host planning is the real one."""

import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def recorder():
    spec = importlib.util.spec_from_file_location("make_sdba_plans", os.path.join(GOLDEN, "make_sdba_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def stored():
    with open(os.path.join(GOLDEN, "sdba_plans.json")) as f:
        return json.load(f)


def test_the_case_matrix_is_the_recorded_one(recorder, stored):
    assert sorted(recorder.cases()) == sorted(stored)
    assert {cid.split("/")[1] for cid in stored} == {"EQM", "QDM", "DQM", "DQM+", "DQM*", "adapt_freq"}   # (all compared below)
    assert len(stored) > 800 and sum(p["error"] is not None for p in stored.values()) > 300


@pytest.mark.parametrize("calendar", ["noleap", "standard"])
@pytest.mark.parametrize("what", ["EQM", "QDM", "DQM+", "DQM*", "adapt_freq"])
def test_launch_plans_are_the_recorded_ones(recorder, stored, calendar, what):
    mine = {cid for cid in stored if cid.split("/")[0] == calendar and (cid.split("/")[1] == what or cid.split("/")[1] + "+" == what)}
    assert mine
    got = recorder.build(only=mine)
    bad = {cid: (got[cid], stored[cid]) for cid in sorted(mine) if got[cid] != stored[cid]}
    assert not bad, f"{len(bad)} of {len(mine)} plans differ; the first, as (now, recorded): {next(iter(bad.items()))}"
