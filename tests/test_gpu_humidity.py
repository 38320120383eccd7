"""The humidity, heat-stress and wind unit on the GPU (xh_air_moisture, xh_wind_map) against the numpy restatement
(tests/humiditycpu.py), which tests/test_humidity_cpu.py holds against the reference's own code, and against the reference's
recorded results themselves (tests/golden/humidity_vectors.npz).

Tolerances (none taken from what the device gives):
  float64 fields   heat_index and vapor_pressure equal the recorded reference bit for bit, and so do every NaN / mask pattern,
                   every clip decision, the calm and north directions and the plateaus and the branch choice of the power factor;
                   everything else is within 1e-12 x the sum of the absolute terms of the value (humiditycpu's ``scale``), the
                   bound of the hydrology, agro and chill units.
  float32 fields   within one float32 ulp of the float64 restatement rounded once (plus the float64 bound), the decisions identical
                   on the fixtures; the thresholds the reference compares with the raw field are rounded to float32 first.
  fused            on float64 fields the fused launch equals the single-output launches bit for bit; on float32 fields it is held
                   to the restatement of the composition, which does not round hurs to float32 in between.
Measured on the MI355X: MEASURED below (the largest |d| / (1e-12 scale) over the float64 vectors, per output)."""
import numpy as np
import pytest

import humiditycases as HCS
import humiditycpu as HC
from poisoned import poisoned_outputs, unwritten  # noqa: F401
from xclim_amd import _capi
from xclim_amd import humidity as H
from xclim_amd import kernels as K
from xclim_amd._capi import DeviceArray

pytestmark = pytest.mark.gpu

# the largest |device - restatement| / (1e-12 scale) measured on the MI355X over the float64 vectors: 1 is the asserted bound
# (tdps: below the 5e-5 the report rounds at; 0.0: equal bit for bit)
MEASURED = {"esat": 0.0004, "vp": 0.0, "vpd": 0.0002, "hurs": 0.0039, "huss": 0.0018, "huss_dew": 0.0036, "tdps": 0.00005, "humidex": 0.0002,
            "heat_index": 0.0, "from_uv": 0.0002, "to_uv": 0.0001, "chill": 0.0001, "power": 0.0006}


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_air_moisture_on_the_recorded_vectors(dev, tag):
    dtype = HCS.DTYPES[tag]
    worst = {}
    for key, output, names, kw in HCS.AIR_CASES:
        ref = HCS.VECTORS[f"{tag}/air/{key}"]
        got = H.air_moisture(**HCS.air_fields(tag, names), outputs=(output,), device=dev, **kw)[output]
        val, scale = HCS.restated(tag, names, output, kw)
        exact = ref if tag == "f64" and output in HCS.BIT_IDENTICAL else None
        w = HCS.check(got, val, scale, dtype, key, bit_identical_to=exact)
        worst[output] = max(worst.get(output, 0.0), w)
        if "exact/" in key and tag == "f32":   # (on a bound the reference's float32 route is not the yardstick: the restatement is)
            continue
        # ... and the recorded reference itself: its NaN / mask pattern and clip decisions, and for float64 its values
        assert np.array_equal(np.isnan(got), np.isnan(ref)), key
        for plateau in (0.0, 100.0):
            assert np.array_equal(got == plateau, np.asarray(ref) == plateau), (key, plateau)
        if tag == "f64":
            ok = np.isfinite(ref)
            assert np.all(np.abs(got - ref)[ok] <= 1e-12 * scale[ok]), key
    print(f"air moisture {tag}: worst |d| / (1e-12 scale)", {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_wind_map_on_the_recorded_vectors(dev, tag):
    dtype = HCS.DTYPES[tag]
    got = HCS.wind_mirror(H, tag, device=dev)
    worst = {}
    for key, (val, scale) in HCS.wind_restated(tag).items():
        ref = np.asarray(HCS.VECTORS[f"{tag}/wind/{key}"])
        w = HCS.check(got[key], val, scale, dtype, key)
        op = key.replace("exact/", "").split("/")[0]
        worst[op] = max(worst.get(op, 0.0), w)
        if "exact/" in key and tag == "f32":
            continue
        assert np.array_equal(np.isnan(got[key]), np.isnan(ref)), key
        for plateau in (0.0, 1.0, 360.0):   # calm, north, and the plateaus and the branch choice of the power factor
            assert np.array_equal(got[key] == plateau, ref == plateau), (key, plateau)
        if tag == "f64":
            ok = np.isfinite(ref)
            assert np.all(np.abs(got[key] - ref)[ok] <= 1e-12 * scale[ok]), key
    assert isinstance(H.uas_vas_to_sfcwind(np.ones((1, 2)), np.ones((1, 2)), device=dev), H.SFCWIND)
    assert H.sfcwind_to_uas_vas(np.ones((1, 2)), np.ones((1, 2)), device=dev)._fields == ("uas", "vas")
    print(f"wind {tag}: worst |d| / (1e-12 scale)", {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_the_fused_launch(dev, tag):
    dtype = HCS.DTYPES[tag]
    f = HCS.air_fields(tag, HCS.FUSED_FIELDS)
    fused = H.air_moisture(**f, outputs=HCS.FUSED_OUTPUTS, device=dev)
    exp = HC.air_moisture(outputs=HCS.FUSED_OUTPUTS, thr32=tag == "f32", **{k: v.astype(np.float64) for k, v in f.items()})
    hurs = H.relative_humidity(f["tas"], tdps=f["tdps"], device=dev)
    single = {"hurs": hurs, "huss": H.specific_humidity(f["tas"], hurs, f["ps"], device=dev), "humidex": H.humidex(f["tas"], tdps=f["tdps"], device=dev),
              "heat_index": H.heat_index(f["tas"], hurs, device=dev)}
    for o in HCS.FUSED_OUTPUTS:
        HCS.check(fused[o], *exp[o], dtype, f"fused {o}")
        ref = np.asarray(HCS.VECTORS[f"{tag}/air/fused/{o}"])
        assert np.array_equal(np.isnan(fused[o]), np.isnan(ref)), o
        if tag == "f64":   # the unrounded hurs of the launch IS the float64 hurs of the single launch
            np.testing.assert_array_equal(fused[o], single[o], err_msg=o)
            ok = np.isfinite(ref)
            assert np.all(np.abs(fused[o] - ref)[ok] <= 1e-12 * exp[o][1][ok]), o
    # hurs from huss and ps feeds the same outputs, and a given hurs field wins over the computable one
    g = HCS.air_fields(tag, dict(tas="tas", huss="huss", ps="ps"))
    outs = ("hurs", "vpd", "humidex", "heat_index")
    got = H.air_moisture(**g, outputs=outs, invalid_values="mask", device=dev)
    exp = HC.air_moisture(outputs=outs, invalid_values="mask", thr32=tag == "f32", **{k: v.astype(np.float64) for k, v in g.items()})
    for o in outs:
        HCS.check(got[o], *exp[o], dtype, f"fused from huss {o}")
    g = HCS.air_fields(tag, dict(tas="tas", tdps="tdps", hurs="hurs"))
    got = H.air_moisture(**g, outputs=("hurs", "heat_index"), device=dev)
    np.testing.assert_array_equal(got["heat_index"], H.heat_index(g["tas"], g["hurs"], device=dev))
    np.testing.assert_array_equal(got["hurs"], H.relative_humidity(g["tas"], tdps=g["tdps"], device=dev))


# ---- the shapes: 3 rows by C cells, padded row views, a base pointer off the 16-byte grid ------------------------------------------
def _fields(R, C, rng, dtype):
    tas = rng.uniform(240, 320, (R, C))
    f = dict(tas=tas, tdps=tas - rng.uniform(0, 15, (R, C)), hurs=rng.uniform(1, 99, (R, C)), huss=rng.uniform(1e-4, 0.03, (R, C)),
             ps=rng.uniform(6e4, 1.05e5, (R, C)))
    return {k: v.astype(dtype) for k, v in f.items()}


def _view(dev, flat, off, R, ld):
    v = DeviceArray(dev, flat.ptr + off * flat.dtype.itemsize, (R, ld), flat.dtype, owner=False)
    v._owner = flat
    return v


def _padded(dev, a, ld, off):
    """The (R, C) host array as a (R, ld) device view that begins ``off`` elements into its buffer; every element of the buffer
    outside the (R, C) block is 1e30."""
    R, C = a.shape
    host = np.full(R * ld + off + 4, 1e30, a.dtype)
    host[off:off + R * ld].reshape(R, ld)[:, :C] = a
    return _view(dev, dev.to_device(host), off, R, ld)


def _output(dev, R, ld, off, dtype):
    flat = dev.empty((R * ld + off + 4,), dtype)   # (poisoned by the module's fixture)
    return flat, _view(dev, flat, off, R, ld)


def _written(flat, off, R, C, ld):
    """The (R, C) block of a downloaded output buffer, after asserting that nothing outside it was written and all of it was."""
    host = flat.get()
    block = host[off:off + R * ld].reshape(R, ld)
    mask = np.zeros(host.shape, bool)
    mask[off:off + R * ld].reshape(R, ld)[:, :C] = True
    assert unwritten(host[~mask]).all(), "an element outside the (R, C) block was written"
    assert not unwritten(block[:, :C]).any(), "an element of the (R, C) block was not written"
    return block[:, :C].copy()


@pytest.mark.parametrize("C", [1, 3, 4, 5, 65, 130])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_output_alone_and_all_together_on_padded_and_offset_views(dev, C, dtype):
    R = 3
    rng = np.random.default_rng(100 + C)
    f = _fields(R, C, rng, dtype)
    f["tas"][-1, -1] = np.nan
    exp = HC.air_moisture(**{k: v.astype(np.float64) for k, v in f.items()}, thr32=dtype == np.float32)
    dense = K.air_moisture(dev, {k: dev.to_device(v) for k, v in f.items()}, HC.OUTPUTS)   # ld = C: 16-byte lanes where C allows
    for o in HC.OUTPUTS:
        HCS.check(dense[o].get(), *exp[o], dtype, f"dense {o}")
    lane = 16 // np.dtype(dtype).itemsize
    for ld, ldo, off in ((C + 3, C + 3, 0), (C + lane, C + 2 * lane, 0), (C + lane, C + lane, 1)):
        d = {k: _padded(dev, v, ld, off) for k, v in f.items()}
        bufs = {o: _output(dev, R, ldo, off, dtype) for o in HC.OUTPUTS}
        K.air_moisture(dev, d, HC.OUTPUTS, C_=C, ld=ld, outs={o: v for o, (_, v) in bufs.items()}, ld_out=ldo)
        for o in HC.OUTPUTS:   # the same numbers on every path, padding and everything around the block untouched
            np.testing.assert_array_equal(_written(bufs[o][0], off, R, C, ldo), dense[o].get(), err_msg=f"{o} ld={ld} off={off}")
        for o in HC.OUTPUTS:   # every subset of size 1: what it needs and nothing else is passed, the rest is NULL
            need = {"esat": ("tas",), "vp": ("huss", "ps"), "vpd": ("tas", "hurs"), "hurs": ("tas", "tdps"), "huss": ("tas", "hurs", "ps"),
                    "huss_dew": ("tdps", "ps"), "tdps": ("huss", "ps"), "humidex": ("tas", "tdps"), "heat_index": ("tas", "hurs")}[o]
            flat, view = _output(dev, R, ldo, off, dtype)
            K.air_moisture(dev, {k: d[k] for k in need}, (o,), C_=C, ld=ld, outs={o: view}, ld_out=ldo)
            np.testing.assert_array_equal(_written(flat, off, R, C, ldo), dense[o].get(), err_msg=f"{o} alone ld={ld} off={off}")


@pytest.mark.parametrize("C", [1, 3, 4, 5, 65, 130])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_wind_map_on_padded_and_offset_views(dev, C, dtype):
    R = 3
    rng = np.random.default_rng(200 + C)
    a, b = rng.uniform(-12, 12, (R, C)).astype(dtype), rng.uniform(0.2, 12, (R, C)).astype(dtype)
    lane = 16 // np.dtype(dtype).itemsize
    calls = [("from_uv", (0, 1), [0.5], ()), ("to_uv", (0, 1), None, ()), ("chill", (0,), None, ("celsius", "mask_invalid")),
             ("power", (0,), [3.5, 13.0, 25.0], ()), ("from_uv", (1,), [0.5], ()), ("to_uv", (0,), None, ())]
    for op, outputs, par, flags in calls:
        dense = K.wind_map(dev, op, dev.to_device(a), dev.to_device(b), par, flags=flags, outputs=outputs)
        for ld, ldo, off in ((C + 3, C + 3, 0), (C + lane, C + 2 * lane, 0), (C + lane, C + lane, 1)):
            bufs = {o: _output(dev, R, ldo, off, dtype) for o in outputs}
            K.wind_map(dev, op, _padded(dev, a, ld, off), _padded(dev, b, ld, off), par, flags=flags, outputs=outputs, C_=C, ld=ld,
                       outs={o: v for o, (_, v) in bufs.items()}, ld_out=ldo)
            for o in outputs:
                np.testing.assert_array_equal(_written(bufs[o][0], off, R, C, ldo), dense[o].get(), err_msg=f"{op} {o} ld={ld} off={off}")
    one = K.wind_map(dev, "power", dev.to_device(a), None, [3.5, 13.0, 25.0])[0].get()   # no density field: NULL, never read
    val, scale, _ = HC.wind_power_potential(a.astype(np.float64), thr32=dtype == np.float32)
    HCS.check(one, val, scale, dtype, "power without density")


def test_argument_errors(dev):
    x = dev.to_device(np.full((3, 4), 290.0, np.float32))
    needs = {"esat": "e_sat needs tas", "vp": "vapor_pressure needs huss and ps", "vpd": "vapor_pressure_deficit needs tas and hurs",
             "hurs": "relative_humidity needs tas and tdps", "huss": "specific_humidity needs tas, ps and hurs",
             "huss_dew": "specific_humidity_from_dewpoint needs tdps and ps", "tdps": "dewpoint_from_specific_humidity needs huss and ps",
             "humidex": "humidex needs tas and tdps", "heat_index": "heat_index needs tas and hurs"}
    for o, msg in needs.items():   # an output whose inputs are missing: XH_ERR_ARG before anything is launched
        lone = {"hurs": x} if o in ("esat", "hurs", "humidex") else {"tas": x}
        if o in ("vpd", "heat_index", "huss"):
            lone = {"ps": x}
        out = dev.empty((3, 4), np.float32)
        with pytest.raises(Exception, match=msg):
            K.air_moisture(dev, lone, (o,), outs={o: out})
        assert unwritten(out.get()).all()
    with pytest.raises(Exception, match="bohren98: tas and tdps"):
        K.air_moisture(dev, {"tas": x, "huss": x, "ps": x}, ("hurs",), rh_method="bohren98")
    with pytest.raises(Exception, match="needs time-major rows"):
        K.air_moisture(dev, {"tas": x}, ("esat",), C_=4, ld=3)
    with pytest.raises(Exception, match="NULL field"):
        K.wind_map(dev, "from_uv", x, None, [0.5])
    with pytest.raises(Exception, match="one output"):
        K.wind_map(dev, "chill", x, x, None, outputs=(0, 1))
    with pytest.raises(Exception, match="cut_in < rated"):
        K.wind_map(dev, "power", x, None, [13.0, 3.5, 25.0])
    assert _capi.UNIT_DEFINES["xclim_hip_humidity.h"]["XH_AM_NOUT"] == len(HC.OUTPUTS)


def test_known_answers_on_the_device(dev):
    a = HCS.KNOWN["test_humidex"]
    tas, tdps = np.array([a["tas_degC"]], float), np.array([a["tdps_degC"]], float)
    np.testing.assert_array_almost_equal(H.humidex(tas, tdps, units="degC", device=dev)[0], a["expected"], a["decimal"])
    hurs = H.relative_humidity(tas, tdps, method="bohren98", units="degC", device=dev)
    np.testing.assert_array_almost_equal(H.humidex(tas + 273.15, hurs=hurs, device=dev)[0] - 273.15, a["expected"], a["decimal"])
    a = HCS.KNOWN["test_heat_index"]
    got = H.heat_index(np.array([a["tas_degC"]], float), np.array([a["hurs"]], float), units="degC", device=dev)[0]
    np.testing.assert_array_equal(got, np.array([np.nan if v is None else v for v in a["reference"]]))
    a = HCS.KNOWN["test_wind_chill"]
    got = H.wind_chill_index(np.array([a["tas_K"]]), np.array([a["sfcWind_kmh"]], float), wind_units="km/h", device=dev)[0]
    np.testing.assert_allclose(got, np.array([np.nan if v is None else v for v in a["expected"]]), rtol=a["rtol"])
    a = HCS.KNOWN["TestWindConversion"]
    w, d = H.uas_vas_to_sfcwind(np.array([a["uas_kmh"]]) * (1 / 3.6), np.array([a["vas_kmh"]]) * (1 / 3.6), device=dev)
    assert np.all(np.around(w[0], 10) == np.around(a["expected_wind"], 10)) and np.all(np.around(d[0], 10) == np.around(a["expected_dir"], 10))
    a = HCS.KNOWN["test_dewpoint_from_specific_humidity"]
    for m in a["reference"]:
        got = H.dewpoint_from_specific_humidity(np.array([a["huss"]]), np.array([a["ps_Pa"]]), method=m, device=dev)[0]
        np.testing.assert_allclose(got, np.array([np.nan if v is None else v for v in a["expected"]]), atol=a["atol"], rtol=a["rtol"])
