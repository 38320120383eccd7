/* xclim_hip_humidity.h — the C ABI of the humidity, heat-stress and wind unit (xclim_amd/csrc/humidity.hip), exported by
 * libxclimhip.so next to the entry points of xclim_hip.h, which this header includes for the context, the return codes and the
 * conventions.  ctypes prototypes: xclim_amd/_capi.py UNIT_SIGNATURES; checked by tests/test_abi_units_cpu.py.
 *
 * The unit is the middle of xclim.indices.converters (converters.py:75-223, 272-387, 606-1084, 1659-1744, 2797-2902): the humidity
 * conversions, humidex and the heat index as ONE element-wise launch that reads up to five fields once and writes any subset of
 * nine results, and the four wind functions as one operation per launch.  All arithmetic is float64 on the widened values in
 * the reference's order of operations; a float32 result is rounded once; nothing intermediate is stored.  The e_sat methods,
 * cases and thresholds are those of xclim_hip_thermal.h (XH_ESAT_*), evaluated by the same device header (csrc/esat.h). */
#ifndef XCLIM_HIP_HUMIDITY_H
#define XCLIM_HIP_HUMIDITY_H

#include "../xclim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the outputs of xh_air_moisture: the index of each in outs[] */
#define XH_AM_ESAT 0        /* saturation_vapor_pressure(tas) [Pa] */
#define XH_AM_VP 1          /* vapor_pressure(huss, ps) [Pa] */
#define XH_AM_VPD 2         /* vapor_pressure_deficit(tas, hurs) [Pa] */
#define XH_AM_HURS 3        /* relative_humidity(tas, tdps) or (tas, huss, ps) [%]; tdps wins when both are given */
#define XH_AM_HUSS 4        /* specific_humidity(tas, hurs, ps) [1] */
#define XH_AM_HUSS_DEW 5    /* specific_humidity_from_dewpoint(tdps, ps) [1] */
#define XH_AM_TDPS 6        /* dewpoint_from_specific_humidity(huss, ps) [K, whatever `celsius` says] */
#define XH_AM_HUMIDEX 7     /* humidex(tas, tdps) when tdps is given, otherwise humidex(tas, hurs=hurs) [the unit of tas] */
#define XH_AM_HEAT_INDEX 8  /* heat_index(tas, hurs) [the unit of tas]; NaN unless tas > 20 degC */
#define XH_AM_NOUT 9

/* rh_method: the ratio of two saturation pressures (or of the vapour pressure to one), or Bohren and Albrecht's exponential */
#define XH_RH_ESAT 0
#define XH_RH_BOHREN98 1

/* invalid_values of relative_humidity (0 .. 100 %) and of specific_humidity (0 .. q_sat) */
#define XH_INVALID_NONE 0
#define XH_INVALID_CLIP 1 /* np.clip: a NaN stays NaN */
#define XH_INVALID_MASK 2 /* NaN outside the range */

/* dew_method: the Magnus coefficients of dewpoint_from_specific_humidity; dew_ice != 0 takes the ice variant */
#define XH_DEW_TETENS30 0
#define XH_DEW_WMO08 1
#define XH_DEW_BUCK81 2
#define XH_DEW_AERK96 3

/* the operations of xh_wind_map */
#define XH_WIND_FROM_UV 0 /* uas_vas_to_sfcwind: a = uas, b = vas [m s-1]; out0 = speed, out1 = direction [degree] */
#define XH_WIND_TO_UV 1   /* sfcwind_to_uas_vas: a = sfcWind [m s-1], b = sfcWindfromdir [degree]; out0 = uas, out1 = vas */
#define XH_WIND_CHILL 2   /* wind_chill_index: a = tas, b = sfcWind; out0 [degC] */
#define XH_WIND_POWER 3   /* wind_power_potential: a = wind_speed, b = air_density [kg m-3] or NULL; out0 [1] */
#define XH_WIND_NOPS 4
/* flags of xh_wind_map */
#define XH_WIND_CELSIUS 1      /* wind chill: tas is in degC (otherwise K, minus 273.15 on load) */
#define XH_WIND_KMH 2          /* wind chill: sfcWind is in km/h (otherwise m s-1, times 3.6 on load) */
#define XH_WIND_US 4           /* wind chill: method "US" (otherwise "CAN", with the slow-wind equation below 5 km/h) */
#define XH_WIND_MASK_INVALID 8 /* wind chill: NaN outside the method's validity range */
#define XH_WIND_NPAR 3

/* xh_air_moisture: any subset of the nine results above for every sample of (R, C) fields, one launch.  Lanes run along the
 * cells, 16 bytes per lane where every given field and requested output allows it (base pointer, row pitch and C multiples of
 * 4 float32 or 2 float64), one element per lane otherwise; rows blockIdx.y, blockIdx.y + gridDim.y, ...
 *
 *   R, C, ld, f64   the fields: DEVICE, all float32 or all float64 (f64 != 0), row pitch ld >= C.
 *   tas, tdps       temperatures, K, or degC with celsius != 0: then v + 273.15 on load where K is needed (otherwise v - 273.15
 *                   where degC is needed).  hurs [%], huss [kg/kg], ps [Pa].  Any of the five may be NULL; a NULL field is never read.
 *   method, kase, ice_thresh, water_thresh, interp_power   saturation_vapor_pressure's, as xh_esat takes them (thresholds in K).
 *                   On float32 fields with celsius == 0 the two thresholds are rounded to float32 first, as numpy >= 2 compares.
 *   rh_method       XH_RH_*; XH_RH_BOHREN98 needs tdps.  invalid_rh, invalid_q: XH_INVALID_* for XH_AM_HURS and XH_AM_HUSS.
 *   dew_method, dew_ice   XH_DEW_*, read by XH_AM_TDPS only.
 *   outs            HOST array of XH_AM_NOUT DEVICE pointers of the fields' dtype, NULL where a result is not asked for; at
 *                   least one.  ld_out >= C is the row pitch of every output.
 *
 * Needs (XH_ERR_ARG otherwise, before anything is launched): ESAT tas; VP huss, ps; VPD tas and RH; HURS tas and tdps, or tas,
 * huss and ps; HUSS tas, ps and RH; HUSS_DEW tdps, ps; TDPS huss, ps; HUMIDEX tas and tdps, or tas and RH; HEAT_INDEX tas and
 * RH.  "RH" is the field hurs when it is given; otherwise it is the value XH_AM_HURS has in this launch (after invalid_rh,
 * before any rounding to float32), whether or not that output is asked for, and needs what XH_AM_HURS needs.
 *
 * A NaN in a field a sample reads gives NaN in every output that depends on it.  Every element (r, c < C) of a requested output
 * is written, nothing beyond column C of a row and nothing of an output that is not asked for.  R == 0 or C == 0 launches
 * nothing. */
int xh_air_moisture(xh_ctx* ctx, int64_t R, int64_t C, int64_t ld, int f64, const void* tas, const void* tdps, const void* hurs,
                    const void* huss, const void* ps, int celsius, int method, int kase, double ice_thresh, double water_thresh,
                    double interp_power, int rh_method, int invalid_rh, int invalid_q, int dew_method, int dew_ice,
                    void* const* outs, int64_t ld_out);

/* xh_wind_map: one of the XH_WIND_* operations on every sample of (R, C) fields, one launch of the same shape.
 *
 *   a, b            DEVICE fields of one dtype, row pitch ld >= C; b may be NULL for XH_WIND_POWER only.
 *   par             HOST, XH_WIND_NPAR float64: XH_WIND_FROM_UV [calm_wind_thresh, m s-1]; XH_WIND_POWER [cut_in, rated, cut_out]
 *                   in the unit of a, cut_in < rated.  On float32 fields these are rounded to float32 first.  May be NULL for
 *                   the other two operations.
 *   out0, out1      DEVICE, the fields' dtype, row pitch ld_out >= C.  The two-output operations take either or both; the
 *                   others take out0 and refuse out1.
 *
 * XH_WIND_FROM_UV: hypot(uas, vas); (270 - degrees(atan2(vas, uas))) % 360 with the sign of the divisor, 360 where that rounds
 * (half to even) to 0, 0 where the speed (as it is written) is below the threshold.  XH_WIND_TO_UV: m = (-dir + 270) % 360,
 * speed cos(radians(m)), speed sin(radians(m)).  XH_WIND_CHILL: V = v ** 0.16, 13.12 + 0.6215 t - 11.37 V + 0.3965 t V; "CAN"
 * below 5 km/h: t + v (-1.59 + 0.1345 t) / 5; masked unless t <= 0 ("CAN") or v > 4.828032 and t <= 10 ("US").
 * XH_WIND_POWER: v = a (b / 1.225) ** (1 / 3); 0 below cut_in, (v^3 - cut_in^3) / (rated^3 - cut_in^3) below rated, 1 below
 * cut_out, 0 from there on and for a NaN.  Written elements and errors as xh_air_moisture. */
int xh_wind_map(xh_ctx* ctx, int op, int64_t R, int64_t C, int64_t ld, int f64, const void* a, const void* b, const double* par,
                int flags, void* out0, void* out1, int64_t ld_out);

#ifdef __cplusplus
}
#endif
#endif /* XCLIM_HIP_HUMIDITY_H */
