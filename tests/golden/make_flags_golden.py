"""Records what the data-quality-flag tests need from the reference (run once, with the reference's checkout at hand):

    python tests/golden/make_flags_golden.py /path/to/reference

* tests/golden/flags_defaults.json: the ``data_flags`` entries of the reference's ``src/xclim/data/variables.yml`` with the
  canonical units of their variables (settings only), read with yaml.
* tests/golden/flags_known_answers.json: the known answers of the reference's ``tests/test_flags.py`` as recipes (how each
  series is built) and recorded results.  The ERA5 case (``test_era5_ecad_qc_flag``) needs the data file
  ``ERA5/daily_surface_cancities_1990-1993.nc`` of the reference's test data, which is not available here: it is left out.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

# tests/test_flags.py of the reference.  A temperature series is ``offset + 273.15 + sin(2 pi arange(rows) / 366)`` in K, daily from
# 1971-01-01 on the standard calendar; "swap": tasmin and tasmax exchange their values; "set_celsius": rows [lo, hi) become
# value + 273.15.  A precipitation series is ``zeros(365)`` in kg m-2 s-1; "add_mm" / "set_mm": v / 3600 / 24 added to / stored in rows
# [lo, hi); "set": the value itself.
KNOWN = {
    "source": "tests/test_flags.py",
    "axis": {"start": "1971-01-01", "calendar": "standard"},
    "temperature_offsets": {"tas": 0, "tasmax": 10, "tasmin": -10},
    "tas_clean": {
        "test": "test_tas_temperature_flags", "variable": "tas", "units": "K", "rows": 366 * 3,
        "always": {"temperature_extremely_high": False, "temperature_extremely_low": False, "values_repeating_for_5_or_more_days": False,
                   "outside_5_standard_deviations_of_climatology": False},
        "cases": [{"dropped": ["tasmin"], "expected": {"tas_exceeds_tasmax": False, "tas_below_tasmin": None}},
                  {"dropped": ["tasmax"], "expected": {"tas_exceeds_tasmax": None, "tas_below_tasmin": False}},
                  {"dropped": [], "expected": {"tas_exceeds_tasmax": False, "tas_below_tasmin": False}}]},
    "tas_suspicious": {
        "test": "test_suspicious_tas_data", "variable": "tas", "units": "K", "rows": 366 * 7, "swap": True,
        "set_celsius": {"tas": [[5, 6, 58], [600, 610, 80], [950, 951, -95]]},
        "expected": {"temperature_extremely_high": True, "temperature_extremely_low": True, "values_repeating_for_5_or_more_days": True,
                     "outside_5_standard_deviations_of_climatology": True, "tas_exceeds_tasmax": True, "tas_below_tasmin": True}},
    "pr_clean": {
        "test": "test_pr_precipitation_flags", "variable": "pr", "units": "kg m-2 s-1", "rows": 365,
        "steps": [["add_mm", 0, 365, 1], ["add_mm", 0, 7, 10], ["add_mm", 358, 365, 11]],
        "expected": {"negative_accumulation_values": False, "very_large_precipitation_events": False,
                     "values_eq_5_repeating_for_5_or_more_days": False, "values_eq_1_repeating_for_10_or_more_days": True}},
    "pr_suspicious": {
        "test": "test_suspicious_pr_data", "variable": "pr", "units": "kg m-2 s-1", "rows": 365,
        "steps": [["set", 8, 9, -1e-6], ["set_mm", 120, 121, 301], ["set_mm", 121, 141, 1], ["set_mm", 200, 300, 5]],
        "expected": {"negative_accumulation_values": True, "very_large_precipitation_events": True,
                     "values_eq_1_repeating_for_10_or_more_days": True, "values_eq_5_repeating_for_5_or_more_days": True}},
    "raises": {
        "test": "test_raises", "variable": "tasmax", "units": "K", "rows": 366 * 3, "present": ["tasmax", "tasmin"],
        "message": "Data quality flags indicate suspicious values. Flags raised are:\n  - ",
        "match": "Maximum temperature values found below minimum temperatures."},
    "names": {
        "test": "test_names", "flags": {"values_op_thresh_repeating_for_n_or_more_days": {"op": "==", "n": 5, "thresh": "-5.1 mm d-1"}},
        "name": "values_eq_minus5point1_repeating_for_5_or_more_days"},
    "specific_discharge": {
        "test": "test_variable_specific_discharge", "variable": "qspec", "units": "m s-1", "rows": 365, "fill": 10.0, "row": 300,
        "dtype": "float64", "cases": [{"value": 100.0000001, "thresh": "100 m/s", "flagged": True},
                                      {"value": 99.9999999, "thresh": "100 m/s", "flagged": False}],
        "description": "One or multiple specific qspec found in excess of {thresh}."},
    "left_out": {"test_era5_ecad_qc_flag": "needs ERA5/daily_surface_cancities_1990-1993.nc of the reference's test data, which is not available"},
}


def main(reference):
    import yaml

    table = yaml.safe_load(open(os.path.join(reference, "src", "xclim", "data", "variables.yml")))["variables"]
    defaults = {var: {"canonical_units": entry["canonical_units"], "data_flags": entry["data_flags"]}
                for var, entry in table.items() if "data_flags" in entry}
    with open(os.path.join(HERE, "flags_defaults.json"), "w") as f:
        json.dump(defaults, f, indent=1, sort_keys=True)
        f.write("\n")
    with open(os.path.join(HERE, "flags_known_answers.json"), "w") as f:
        json.dump(KNOWN, f, indent=1)
        f.write("\n")
    print(f"{len(defaults)} variables with data_flags; {len(KNOWN) - 4} groups of known answers")


if __name__ == "__main__":
    main(sys.argv[1])
