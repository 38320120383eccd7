"""The guard of tests/test_gpu_strided_abi.py (no GPU): every entry point of include/xclim_hip.h with a stride parameter
has an entry in the table of tests/stridedabi.py, every entry names parameters its prototype has, and every entry is
reached by a padded case.  A new entry point or a new stride parameter fails here, on any machine, until it has one."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import stridedabi as S  # noqa: E402


def strided_entry_points():
    return {name: [p for p in params[1:] if S.STRIDE_NAME.match(p)] for name, params in S.PROTOS.items()
            if any(S.STRIDE_NAME.match(p) for p in params[1:])}


def test_the_header_parses():
    assert len(S.PROTOS) >= 113, len(S.PROTOS)
    assert S.PROTOS["xh_threshold_count_doy"][:6] == ["ctx", "x", "T", "C", "st", "sc"]
    assert S.PROTOS["xh_fire_weather"][-4:] == ["outputs", "st_out", "season_mask_out", "winter_pr_out"]
    assert "xh_memcpy2d" in S.PROTOS and "xh_last_error" in S.PROTOS


def test_every_strided_entry_point_is_in_the_table():
    have = strided_entry_points()
    assert not (set(S.TABLE) & set(S.EXEMPT)), "an entry point is either tested or exempt"
    missing = sorted(set(have) - set(S.TABLE) - set(S.EXEMPT))
    assert not missing, f"entry points with a stride parameter and no padded case: {missing}"
    stale = sorted((set(S.TABLE) | set(S.EXEMPT)) - set(have))
    assert not stale, f"listed, but without a stride parameter in the header: {stale}"


def test_only_plumbing_is_exempt():
    """Entry points that move bytes and compute nothing may be exempt, each with its reason."""
    plumbing = {"xh_memcpy2d"}
    assert set(S.EXEMPT) <= plumbing, sorted(set(S.EXEMPT) - plumbing)
    assert all(isinstance(r, str) and r for r in S.EXEMPT.values())


@pytest.mark.parametrize("name", sorted(S.TABLE))
def test_table_entry_names_parameters_of_the_prototype(name):
    params = S.PROTOS[name][1:]
    ops = S.TABLE[name]
    assert ops
    for op in ops:
        for p in (op.ptr, op.stride, op.minor):
            assert p is None or p in params, f"{name}: no parameter {p!r} in {params}"
        assert op.mode in ("r", "w", "rw")
        for expr in (op.rows, op.width, op.dtype, op.ptrs):   # the sizes are written over the parameter names too
            if isinstance(expr, str) and expr not in S._DTYPES:
                names = set(compile(expr, name, "eval").co_names)
                assert names <= set(params), f"{name}: {expr!r} uses {sorted(names - set(params))}"
    # every stride parameter of the prototype belongs to an operand (the cell stride as the time-minor axis of one)
    covered = {op.stride for op in ops} | {op.minor for op in ops}
    for p in strided_entry_points()[name]:
        assert p in covered or p == "sc", f"{name}: stride parameter {p} has no operand"


def test_only_the_column_entry_points_have_a_time_minor_form():
    """The entry points the header names as taking st == 1, sc >= T: their operands carry `minor`, no other does."""
    column = {"xh_quantile_series", "xh_eqm_train", "xh_qdm_adjust", "xh_quantile_cells", "xh_adapt_freq", "xh_nan_quantile",
              "xh_nan_quantile_f64"}
    assert {n for n, ops in S.TABLE.items() if any(op.minor for op in ops)} == column
    header = open(S.HEADER).read()
    intro = header[:header.index("#ifndef XCLIM_HIP_H")]
    for n in column - {"xh_nan_quantile_f64"}:
        assert n in intro, f"{n}: not named among the column kernels in the header's conventions"


def test_every_table_entry_is_reached_by_a_padded_case():
    import test_gpu_strided_abi as G

    reached = set()
    for c in G.CASES.values():
        assert c.reaches, c.name
        reached |= set(c.reaches)
    assert reached == set(S.TABLE), (sorted(set(S.TABLE) - reached), sorted(reached - set(S.TABLE)))
    # and every case runs at one of the cell counts at least, under every pad list that fits it
    assert {C for _, C, _, _ in G._PADDED} >= {67, 260}
    assert {n for n, *_ in G._PADDED} == set(G.CASES)
