"""Boundary adapter: the callables that slot into xclim in place of the reference's hot-path functions.

Two tiers, as the reference resolves its own hot path:

* **tier 2 — ``xr.apply_ufunc`` callees** (numpy in, numpy out; no xarray needed, tested on the GPU in
  tests/test_gpu_patch.py):

  - :func:`cumsum_reset_np` replaces ``xclim.indices.run_length._cumsum_reset_np`` (run_length.py:143-151, called at
    :209-216): the core dim arrives LAST, possibly as a non-contiguous view of the ``(time, lat, lon)`` array; the callee
    MUTATES ``arr`` and returns it.
  - :func:`calc_perc` replaces ``xclim.core.utils.calc_perc`` (core/utils.py:279-323, imported at call time by
    ``percentile_doy``, core/calendar.py:441, 469-479): ``(…, stack_dim)`` strided view -> ``(…, nper)``.

* **tier 1 — module attributes** (same-signature functions on ``xr.DataArray``, xclim_amd/xr_adapter.py):
  :func:`install` replaces them in every module that holds them (``rl.*`` through the module object, the generic /
  calendar functions also in the index modules that imported them by name, ``calc_perc`` at its definition).  xarray is
  not installable in the build environment, so the wrappers take what they need from xarray / xclim through an ``Env``
  and are EXECUTED in tests/test_gpu_adapter.py against a small DataArray stand-in (tests/fakexr.py) installed into
  stand-in modules with the reference's import structure; with the real packages:
  ``python -c "import xclim_amd.patch as p; print(p.install())"``.

``percentile_doy`` keeps a ``__wrapped__`` attribute because ``bootstrap_func`` calls ``percentile_doy.__wrapped__``
(core/bootstrapping.py:195).
"""

from __future__ import annotations

import numpy as np

from . import kernels as K
from . import utils as _hutl
from ._capi import get_device

__all__ = ["cumsum_reset_np", "calc_perc", "install", "uninstall", "real_env"]


# ---- tier 2 --------------------------------------------------------------------------------------------------------
def cumsum_reset_np(arr: np.ndarray, index: str, one=None, *, device=None) -> np.ndarray:
    """Drop-in for ``run_length._cumsum_reset_np(arr, index, one)`` (run_length.py:143-151).

    ``arr``: binary (0 / 1) values, integer or float dtype, core dim on the LAST axis, leading dims arbitrary, possibly a
    non-contiguous view.  ``index``: "last" (forward) or "first" (backward).  ``one`` is only the dtype-carrying
    constant of the numba version and is ignored.  The result is written into ``arr`` (its dtype) and ``arr`` is
    returned, like the reference.  The transposed view xarray hands over (time moved last on a ``(time, lat, lon)``
    array) is uploaded without a host-side copy: moving the axis back gives the C-contiguous ``(T, C)`` layout the
    kernel wants.
    """
    if index not in ("first", "last"):
        raise ValueError(f"index must be 'first' or 'last', got {index!r}")
    if arr.ndim == 0 or arr.shape[-1] == 0 or arr.size == 0:
        return arr
    dev = device or get_device()
    tfirst = np.moveaxis(arr, -1, 0)  # (T, ...) view
    T = tfirst.shape[0]
    flat = np.ascontiguousarray(tfirst).reshape(T, -1)  # no copy when `arr` is the transposed view of a C-ordered array
    if flat.dtype in (np.bool_, np.uint8):
        m = K.mask_to_f32(dev, dev.to_device(flat.view(np.uint8)))
    else:
        m = dev.to_device(flat, dtype=np.float32)
    out = K.cumsum_reset(dev, m, index).get().reshape(tfirst.shape)
    tfirst[...] = out.astype(arr.dtype, copy=False)  # writes through the view into `arr`
    return arr


def calc_perc(arr: np.ndarray, percentiles=None, alpha: float = 1.0, beta: float = 1.0, copy: bool = True, *, device=None):
    """Drop-in for ``core.utils.calc_perc`` (core/utils.py:279-323): percentiles along the last axis of a possibly strided
    ``(…, N)`` view, percentile axis LAST in the result, float64.  ``copy`` is accepted and irrelevant: the input is never
    modified (the reference sorts a copy unless told otherwise)."""
    return _hutl.calc_perc(arr, percentiles, alpha, beta, copy, device=device)


# ---- tier 1 (needs xarray + xclim) ----------------------------------------------------------------------------------
_saved: dict = {}

# reference module -> names imported BY NAME there (/root/reference/src/xclim/indices/_threshold.py:25-36,
# _multivariate.py:13, 22-24, _simple.py:10, _hydrology.py:14, _anuclim.py:26, core/bootstrapping.py:17, indices/stats.py:23);
# a name is only replaced where the module really holds it (hasattr), so the table may list more than a version imports
_GENERIC_NAMES = ("threshold_count", "count_occurrences", "domain_count", "select_resample_op", "spell_length_statistics",
                  "cumulative_difference", "compare", "season", "first_day_threshold_reached", "bivariate_count_occurrences")
_BY_NAME = {
    "xclim.indices.generic": _GENERIC_NAMES,
    "xclim.indices._threshold": _GENERIC_NAMES,
    "xclim.indices._multivariate": _GENERIC_NAMES + ("percentile_doy", "resample_doy"),
    "xclim.indices._simple": _GENERIC_NAMES,
    "xclim.indices._hydrology": _GENERIC_NAMES,
    "xclim.indices._anuclim": _GENERIC_NAMES,
    "xclim.indices._agro": _GENERIC_NAMES + ("percentile_doy", "resample_doy"),
    "xclim.indices._conversion": _GENERIC_NAMES,
    "xclim.indicators.generic._stats": ("select_resample_op",),   # indicators/generic/_stats.py:6
    "xclim.ensembles._robustness": ("compare",),                  # ensembles/_robustness.py:24
    "xclim.core.calendar": ("percentile_doy", "resample_doy"),
    "xclim.core.bootstrapping": ("percentile_doy",),
    "xclim.indices.stats": ("percentile_doy",),
    # rl.* is always reached through the module object: patching the module attributes is enough (gen:37, _threshold.py:25)
    "xclim.indices.run_length": ("rle", "rle_statistics", "longest_run", "windowed_run_events", "windowed_run_count",
                                 "first_run", "last_run", "season_length", "resample_and_rl"),
    "xclim.core.utils": ("calc_perc",),
}


# the standardized indices: stats.py defines both; _agro.py (SPI / SPEI) and _hydrology.py (SSI / SGI) import
# standardized_index by name (indices/_agro.py:36, indices/_hydrology.py:16)
_SI_MODULE = "xclim.indices.stats"
_SI_NAMES = ("standardized_index", "standardized_index_fit_params")
_SI_BY_NAME = {"xclim.indices.stats": _SI_NAMES, "xclim.indices._agro": ("standardized_index",),
               "xclim.indices._hydrology": ("standardized_index",)}

# the distribution fits: stats.py defines the six; indicators/generic/_stats.py:7-8 imports ``fit as _fit`` and
# ``frequency_analysis`` by name.  module -> {attribute there: function of stats.FIT_ADAPTED}
_FIT_BY_NAME = {"xclim.indices.stats": {n: n for n in ("fit", "parametric_quantile", "parametric_cdf", "parametric_pdf", "fa",
                                                       "frequency_analysis")},
                "xclim.indicators.generic._stats": {"_fit": "fit", "frequency_analysis": "frequency_analysis"}}

_FIRE_MODULE = "xclim.indices.fire._cffwis"
_FIRE_NAMES = ("_fire_weather_calc", "_fire_season")
_FFDI_MODULE = "xclim.indices.fire._ffdi"
_FFDI_NAMES = ("_keetch_byram_drought_index", "_griffiths_drought_factor")
_CHILL_MODULE = "xclim.indices._agro"
_CHILL_NAME = "_chill_portion_one_season"  # indices/_agro.py:1442-1465, called by name at :1473
# PET and the water budget: water_budget calls potential_evapotranspiration by module-global name (converters.py:2718); the
# three indicators hold the function objects as a staticmethod ``compute`` on their classes (core/indicator.py:515-517,
# indicators/convert/_conversion.py:418-470)
# the ANUCLIM quarter and seasonality functions: public functions of _anuclim.py (:104-442) that xclim.indices re-exports
# (indices/__init__.py: ``from ._anuclim import *``) and the anuclim.yml indicators reach through that namespace
_ANUCLIM_MODULES = ("xclim.indices._anuclim", "xclim.indices")
_AGRO_MODULES = ("xclim.indices._agro", "xclim.indices")   # indices/__init__.py: ``from ._agro import *``
_HYDRO_MODULES = ("xclim.indices._hydrology", "xclim.indices")   # indices/__init__.py: ``from ._hydrology import *``
_PET_MODULE = "xclim.indices.converters"
_PET_NAMES = ("potential_evapotranspiration", "water_budget")
_THERMAL_NAMES = ("saturation_vapor_pressure", "mean_radiant_temperature", "universal_thermal_climate_index")
_THERMAL_MODULES = ("xclim.indices.converters", "xclim.indices", "xclim.indices._conversion")
_THERMAL_INDICATORS = {"xclim.indicators.convert._conversion": ("universal_thermal_climate_index", "mean_radiant_temperature")}
# indicators/convert/_conversion.py:66-413: the Converter indicators whose ``compute`` is one of humidity.ADAPTED
_HUMIDITY_INDICATORS = {"xclim.indicators.convert._conversion": (
    "humidex", "heat_index", "wind_speed_from_vector", "wind_vector_from_speed", "wind_power_potential", "relative_humidity_from_dewpoint",
    "relative_humidity", "specific_humidity", "specific_humidity_from_dewpoint", "dewpoint_from_specific_humidity", "vapor_pressure",
    "vapor_pressure_deficit", "wind_chill_index")}
_PET_INDICATORS = {"xclim.indicators.convert._conversion": ("potential_evapotranspiration", "water_budget_from_tas",
                                                           "water_budget")}


def real_env():
    """The :class:`xr_adapter.Env` of an installation that has xarray and xclim."""
    import xarray as xr
    from xclim.core.calendar import build_climatology_bounds
    from xclim.core.units import convert_units_to, pint2cfattrs, to_agg_units, units2pint

    from .xr_adapter import Env

    def finish_select_resample_op(out, da, op, out_units):  # the tail of indices/generic.py:118-125
        if out_units is not None:
            return out.assign_attrs(units=out_units)
        if op in ("std", "var"):
            out.attrs.update(pint2cfattrs(units2pint(out.attrs["units"]), is_difference=True))
        return to_agg_units(out, da, op)

    return Env(xr.DataArray, convert_units_to, to_agg_units, finish_select_resample_op, build_climatology_bounds,
               difference_attrs=lambda u: pint2cfattrs(units2pint(u), is_difference=True))


def install(env=None, modules=None) -> list[str]:
    """Replace the reference's hot-path functions (SURVEY.md §8b resolution rules); returns the patched names.

    ``env`` / ``modules``: dependency injection for the tests (tests/test_gpu_adapter.py installs the wrappers into
    stand-in modules with the reference's import structure, because xarray / xclim are not installable there);
    by default the real packages are used.  Functions the HIP path does not serve are forwarded to the saved originals."""
    import importlib

    from . import agro, analog, anuclim, compound, dataflags, ensembles, grid, hydrology, partitioning, phase, rainseason
    from .xr_adapter import make_wrappers

    env = env or real_env()

    def resolve(modname):
        if modules is not None:
            return modules.get(modname)
        try:
            return importlib.import_module(modname)
        except ImportError:
            return None

    orig = {}  # the reference's own functions, for the calls the HIP path forwards
    for modname in ("xclim.indices.generic", "xclim.indices.run_length", "xclim.core.calendar", "xclim.core.utils"):
        mod = resolve(modname)
        for name in _BY_NAME[modname]:
            if mod is not None and hasattr(mod, name):
                orig.setdefault(name, _saved.get((modname, name), getattr(mod, name)))
    nbu = resolve("xsdba.nbutils")
    if nbu is not None and hasattr(nbu, "quantile"):  # the original behind the wrapper's forwards (other dims, float64 fields)
        orig["sdba_quantile"] = _saved.get(("xsdba.nbutils", "quantile"), nbu.quantile)
    sut = resolve("xsdba.utils")
    if sut is not None and hasattr(sut, "interp_on_quantiles"):
        orig["sdba_interp_on_quantiles"] = _saved.get(("xsdba.utils", "interp_on_quantiles"), sut.interp_on_quantiles)
    wrappers = make_wrappers(env, orig)
    _cleanups.append(wrappers.pop("_clear_valid_cache"))
    wrappers["_cumsum_reset_np"] = cumsum_reset_np
    done = []

    def patch(modname, attr, fn):
        mod = resolve(modname)
        if mod is not None and hasattr(mod, attr):
            _saved.setdefault((modname, attr), getattr(mod, attr))
            setattr(mod, attr, fn)
            done.append(f"{modname}.{attr}")

    def install_mirror(modnames, mirror, *extra):
        """The functions ``mirror.ADAPTED`` replaced where they are defined (``modnames[0]``, which must hold every one of them) and,
        by identity, where the other modules re-export them.  ``extra``: attributes of the defining module (None where it has none)
        that ``mirror.make_adapters`` takes after the originals."""
        defining = resolve(modnames[0])
        if defining is None or not all(hasattr(defining, n) for n in mirror.ADAPTED):
            return
        origs = {n: _saved.get((modnames[0], n), getattr(defining, n)) for n in mirror.ADAPTED}
        adapters = mirror.make_adapters(env, origs, *(getattr(defining, x, None) for x in extra))
        for modname in modnames:
            m = resolve(modname)
            for name in mirror.ADAPTED:
                if m is not None and _saved.get((modname, name), getattr(m, name, None)) is origs[name]:
                    patch(modname, name, adapters[name])

    for modname, names in _BY_NAME.items():
        for name in names:
            patch(modname, name, wrappers[name])
    patch("xclim.indices.run_length", "_cumsum_reset_np", cumsum_reset_np)
    # the missing-value check of Indicator._postprocess (core/indicator.py:1522-1549): a METHOD of MissingAny
    miss_mod = resolve("xclim.core.missing")
    # ... and of the other registered methods (:325-512; MissingTwoSteps.__call__ :352-393 for wmo / pct / at_least_n).  Each
    # class is patched where it DEFINES __call__ semantics of its own; the base classes stay untouched (custom subclasses
    # registered by users keep the reference's code)
    for cname in ("MissingAny", "MissingSomeButNotAll", "MissingWMO", "MissingPct", "AtLeastNValid"):
        cls = getattr(miss_mod, cname, None) if miss_mod is not None else None
        key = f"{cname}.__call__"
        if cls is not None and key in wrappers:
            if ("xclim.core.missing", key) not in _saved:
                # (the function found on the class — possibly inherited; uninstall() removes the override again)
                _saved[("xclim.core.missing", key)] = cls.__dict__.get("__call__", _INHERITED)
            own = _saved[("xclim.core.missing", key)]
            # what the wrapper forwards to: the class's own function, or the one it inherits (MissingBase / MissingTwoSteps)
            orig[key] = own if own is not _INHERITED else next(b.__dict__["__call__"] for b in cls.__mro__[1:] if "__call__" in b.__dict__)
            cls.__call__ = wrappers[key]
            done.append(f"xclim.core.missing.{key}")
    # Indicator.__call__ (core/indicator.py:865-944): parse -> compute (the index, its percentile / resample helpers) ->
    # missing-value check (:1522-1549), all on the same DataArrays and without user code in between: ONE scope of
    # device-resident inputs (Device.keep_inputs) per call, dropped when the call returns
    ind_mod = resolve("xclim.core.indicator")
    icls = getattr(ind_mod, "Indicator", None) if ind_mod is not None else None
    if icls is not None:
        if ("xclim.core.indicator", "Indicator.__call__") not in _saved:
            _saved[("xclim.core.indicator", "Indicator.__call__")] = icls.__call__
        icall = _saved[("xclim.core.indicator", "Indicator.__call__")]

        def _indicator_call(self, *args, **kwds):
            with get_device().keep_inputs():
                return icall(self, *args, **kwds)

        _indicator_call.__wrapped__ = icall
        _indicator_call.__doc__ = icall.__doc__
        icls.__call__ = _indicator_call
        done.append("xclim.core.indicator.Indicator.__call__")
    # xsdba (third party, re-exported by src/xclim/sdba.py:10): the per-cell multi-quantile entry point; xsdba's own
    # modules reach it through the module object (``nbu.quantile``), so the one attribute is enough
    patch("xsdba.nbutils", "quantile", wrappers["sdba_quantile"])
    # qm_adjust / qdm_adjust reach the factor interpolation as ``u.interp_on_quantiles`` (module object): group="time" -> xh_eqm_adjust
    patch("xsdba.utils", "interp_on_quantiles", wrappers["sdba_interp_on_quantiles"])
    # the fire weather system: fire_weather_ufunc / fire_season reach these two by module-global name (through
    # xr.apply_ufunc / map_blocks), so every public fire function and indicator is served through them
    fmod = resolve(_FIRE_MODULE)
    if fmod is not None and all(hasattr(fmod, n) for n in _FIRE_NAMES):
        from .fire import make_adapters

        fire = make_adapters(*(_saved.get((_FIRE_MODULE, n), getattr(fmod, n)) for n in _FIRE_NAMES))
        for name in _FIRE_NAMES:
            patch(_FIRE_MODULE, name, fire[name])
    # the McArthur system: the public KBDI / DF functions (and their indicators) reach the two gufuncs by module-global name
    # inside xr.apply_ufunc; mcarthur_forest_fire_danger_index is one xarray expression and stays xclim's
    dmod = resolve(_FFDI_MODULE)
    if dmod is not None and all(hasattr(dmod, n) for n in _FFDI_NAMES):
        from .ffdi import make_adapters as ffdi_adapters

        ffdi = ffdi_adapters(*(_saved.get((_FFDI_MODULE, n), getattr(dmod, n)) for n in _FFDI_NAMES))
        for name in _FFDI_NAMES:
            patch(_FFDI_MODULE, name, ffdi[name])
    # chill portions: chill_portions reaches _chill_portion_one_season by module-global name inside xr.apply_ufunc (through
    # resample_map); chill_units and make_hourly_temperature are xarray expressions and stay xclim's
    amod = resolve(_CHILL_MODULE)
    if amod is not None and hasattr(amod, _CHILL_NAME):
        from .chill import make_adapters as chill_adapters

        orig_chill = _saved.get((_CHILL_MODULE, _CHILL_NAME), getattr(amod, _CHILL_NAME))
        patch(_CHILL_MODULE, _CHILL_NAME, chill_adapters(orig_chill)[_CHILL_NAME])
    # the period-index mirrors, all installed the same way
    # BIO4, BIO8-BIO11 and BIO15-BIO19: one launch of xh_bioclim each
    install_mirror(_ANUCLIM_MODULES, anuclim)
    # the six period functions of the viticulture / agroclimatic unit (huglin_index ... effective_growing_degree_days): one launch
    # each.  corn_heat_units and qian_weighted_mean_average are lazy xarray expressions and stay xclim's
    install_mirror(_AGRO_MODULES, agro, "_gather_lat")
    # rain_season and hardiness_zones, the last two functions of _agro.py: one launch of xh_rain_season; the period minimum +
    # xh_rolling_zones.  Replaced only where both are present
    install_mirror(_AGRO_MODULES, rainseason)
    # the streamflow and snow-melt functions of _hydrology.py (base_flow_index ... base_flow_index_seasonal_ratio); sen_slope also
    # where pymannkendall is absent (it no longer needs it).  runoff_ratio is unit conversion around two means and stays xclim's,
    # as do lag_snowpack_flow_peaks and the snd_max / snw_max family (select_resample_op, served by the generic wrappers)
    install_mirror(_HYDRO_MODULES, hydrology)
    # data_flags of core/dataflags.py: the whole list of checks of a variable in one launch; ecad_compliant calls it through the
    # module global and is thereby served
    install_mirror(("xclim.core.dataflags",), dataflags, "xarray", "VARIABLES", "_REGISTRY", "DataQualityException")
    # the snow / rain partition and its period indices, defined in three modules: the two approximations of converters.py
    # (_multivariate.py imports them by name), six functions of _multivariate.py and the four snowfall indices of _threshold.py
    install_mirror(("xclim.indices.converters", "xclim.indices", "xclim.indices._multivariate"), phase.converters)
    install_mirror(("xclim.indices._multivariate", "xclim.indices"), phase.multivariate)
    install_mirror(("xclim.indices._threshold", "xclim.indices"), phase.threshold)
    # the compound percentile-day counts, blowing_snow and water_cycle_intensity of _multivariate.py and
    # degree_days_exceedance_date of _threshold.py: xarray expressions that reach no replaced generic / run_length function, one
    # launch each here
    install_mirror(("xclim.indices._multivariate", "xclim.indices"), compound.multivariate)
    install_mirror(("xclim.indices._threshold", "xclim.indices"), compound.threshold)
    # sea_ice_area / sea_ice_extent of _threshold.py and jetstream_metric_woollings of _synoptic.py: what reduces across the grid
    # (xarray.dot, cf.mean and rolling().construct().dot() in the reference), one or two launches each here
    install_mirror(("xclim.indices._threshold", "xclim.indices"), grid.threshold)
    install_mirror(("xclim.indices._synoptic", "xclim.indices"), grid.synoptic)
    # spatial_analogs of analog.py: one launch with a lane per candidate cell instead of a Python call per cell
    install_mirror(("xclim.analog",), analog)
    # robustness_fractions and robustness_coefficient of ensembles/_robustness.py: one launch per test instead of a scipy call per
    # (cell, realization); robustness_categories is a handful of xarray comparisons and stays xclim's
    install_mirror(("xclim.ensembles._robustness", "xclim.ensembles"), ensembles, "xr", "gen_call_string", "SIGNIFICANCE_TESTS")
    # hawkins_sutton, lafferty_sriver and general_partition of ensembles/_partitioning.py: one launch fits every series where polyfit
    # makes one Python call per series with a NaN; ensemble_mean_std_max_min of ensembles/_base.py rides on the same unit
    install_mirror(("xclim.ensembles._partitioning", "xclim.ensembles"), partitioning, "xr")
    install_mirror(("xclim.ensembles._base", "xclim.ensembles"), partitioning.base_mirror, "xr", "update_history")
    cmod = resolve(_PET_MODULE)
    if cmod is not None and all(hasattr(cmod, n) for n in _PET_NAMES):
        from .converters import make_adapters as pet_adapters

        origs = {n: _saved.get((_PET_MODULE, n), getattr(cmod, n)) for n in _PET_NAMES}
        pet = pet_adapters(env, origs["potential_evapotranspiration"], origs["water_budget"],
                           getattr(cmod, "_gather_lat", None))
        for name in _PET_NAMES:
            patch(_PET_MODULE, name, pet[name])
        by_orig = {id(origs[n]): pet[n] for n in _PET_NAMES}
        for modname, names in _PET_INDICATORS.items():
            imod = resolve(modname)
            for name in names:
                cls = type(getattr(imod, name, None))
                own = cls.__dict__.get("compute") if imod is not None else None
                if isinstance(own, staticmethod) and id(own.__func__) in by_orig and cls not in _saved_compute:
                    _saved_compute[cls] = own
                    cls.compute = staticmethod(by_orig[id(own.__func__)])
                    done.append(f"{modname}.{name}.compute")
    # thermal comfort: the three functions of converters.py, by identity where xclim.indices and xclim.indices._conversion re-export
    # them, and the ``compute`` of the two Converter indicators that hold them (as the PET indicators above)
    if cmod is not None and all(hasattr(cmod, n) for n in _THERMAL_NAMES):
        from .thermal import make_adapters as thermal_adapters

        origs = {n: _saved.get((_PET_MODULE, n), getattr(cmod, n)) for n in _THERMAL_NAMES}
        th = thermal_adapters(env, origs, getattr(cmod, "_gather_lat", None), getattr(cmod, "_gather_lon", None))
        for modname in _THERMAL_MODULES:
            m = resolve(modname)
            for name in _THERMAL_NAMES:
                if m is not None and _saved.get((modname, name), getattr(m, name, None)) is origs[name]:
                    patch(modname, name, th[name])
        by_orig = {id(origs[n]): th[n] for n in _THERMAL_NAMES}
        for modname, names in _THERMAL_INDICATORS.items():
            imod = resolve(modname)
            for name in names:
                cls = type(getattr(imod, name, None))
                own = cls.__dict__.get("compute") if imod is not None else None
                if isinstance(own, staticmethod) and id(own.__func__) in by_orig and cls not in _saved_compute:
                    _saved_compute[cls] = own
                    cls.compute = staticmethod(by_orig[id(own.__func__)])
                    done.append(f"{modname}.{name}.compute")
    # the humidity, heat-stress and wind conversions: the twelve functions of converters.py (only where it holds all of them), by
    # identity where xclim.indices and xclim.indices._conversion re-export them, and the ``compute`` of the Converter indicators that
    # hold them (both relative_humidity indicators hold the one function)
    from . import humidity

    if cmod is not None and all(hasattr(cmod, n) for n in humidity.ADAPTED):
        origs = {n: _saved.get((_PET_MODULE, n), getattr(cmod, n)) for n in humidity.ADAPTED}
        hum = humidity.make_adapters(env, origs)
        for modname in _THERMAL_MODULES:
            m = resolve(modname)
            for name in humidity.ADAPTED:
                if m is not None and _saved.get((modname, name), getattr(m, name, None)) is origs[name]:
                    patch(modname, name, hum[name])
        by_orig = {id(origs[n]): hum[n] for n in humidity.ADAPTED}
        for modname, names in _HUMIDITY_INDICATORS.items():
            imod = resolve(modname)
            for name in names:
                cls = type(getattr(imod, name, None))
                own = cls.__dict__.get("compute") if imod is not None else None
                if isinstance(own, staticmethod) and id(own.__func__) in by_orig and cls not in _saved_compute:
                    _saved_compute[cls] = own
                    cls.compute = staticmethod(by_orig[id(own.__func__)])
                    done.append(f"{modname}.{name}.compute")
    # SPI / SPEI / SSI / SGI: the forms the device does not serve go to the saved originals
    smod = resolve(_SI_MODULE)
    if smod is not None and all(hasattr(smod, n) for n in _SI_NAMES):
        from .stats import make_adapters as si_adapters

        si = si_adapters(env, *(_saved.get((_SI_MODULE, n), getattr(smod, n)) for n in _SI_NAMES))
        for modname, names in _SI_BY_NAME.items():
            for name in names:
                patch(modname, name, si[name])
    # fit, the parametric functions, fa and frequency_analysis, and the two names the generic indicators import
    if smod is not None and all(hasattr(smod, n) for n in _FIT_BY_NAME[_SI_MODULE]):
        from .stats import make_fit_adapters

        fits = make_fit_adapters(env, {n: _saved.get((_SI_MODULE, n), getattr(smod, n)) for n in _FIT_BY_NAME[_SI_MODULE]})
        for modname, names in _FIT_BY_NAME.items():
            for attr, name in names.items():
                patch(modname, attr, fits[name])
    _saved_modules.update({} if modules is None else modules)
    return done


_INHERITED = object()  # marker in _saved: the class did not define the attribute itself (uninstall deletes the override)
_saved_modules: dict = {}
_saved_compute: dict = {}  # indicator class -> its original staticmethod compute
_cleanups: list = []  # per install(): drops the valid-count cache of its wrappers


def uninstall() -> None:
    import importlib

    for (modname, attr), fn in _saved.items():
        mod = _saved_modules.get(modname) or importlib.import_module(modname)
        if "." in attr:  # a method: "Class.name"
            cname, meth = attr.split(".")
            if fn is _INHERITED:
                delattr(getattr(mod, cname), meth)
            else:
                setattr(getattr(mod, cname), meth, fn)
        else:
            setattr(mod, attr, fn)
    for cls, fn in _saved_compute.items():
        cls.compute = fn
    _saved_compute.clear()
    _saved.clear()
    _saved_modules.clear()
    for fn in _cleanups:
        fn()
    _cleanups.clear()
