// esat.h — saturation vapour pressure [Pa] of a temperature in K (indices/converters.py:390-603), float64, device only.
//
// The eight methods of saturation_vapor_pressure over water and over ice, and its three cases: all water, the binary switch at
// ice_thresh (tas > thresh is water), and the interpolation alpha = ((tas - T_i) / (T_w - T_i)) ** interp_power between the two
// thresholds.  Terms are added in the reference's order; tas**2 is tas * tas as numpy squares it, tas**3 and tas**4 are repeated
// products where numpy calls pow (within two ulp of a term that is below 1e-2 of the exponent).  "ecmwf" is buck81 over water
// and aerk96 over ice.  A NaN temperature gives NaN in every case.
#pragma once

#include <cmath>

#include "../../include/units/xclim_hip_thermal.h"  // the XH_ESAT_* methods and cases
#include "common.h"


// A exp(B (T - 273.16) / (T + C)), the Auguste-Roche-Magnus form of tetens30, wmo08, buck81 and aerk96
__device__ __forceinline__ double xh_esat_magnus(double t, double A, double B, double C) { return A * exp(B * (t - 273.16) / (t + C)); }

// ITS-90 over water (converters.py:432-442): the one UTCI uses
__device__ __forceinline__ double xh_esat_its90_water(double t) {
  const double t2 = t * t;
  return exp(-2836.5744 / t2 + -6028.076559 / t + 19.54263612 + -2.737830188e-2 * t + 1.6261698e-5 * t2 + 7.0229056e-10 * (t2 * t) +
             -1.8680009e-13 * (t2 * t2) + 2.7150305 * log(t));
}

__device__ __forceinline__ double xh_esat_water(double t, int method) {
  switch (method) {
    case XH_ESAT_SONNTAG90:
      return 100 * exp(-6096.9385 / t + 16.635794 + -2.711193e-2 * t + 1.673952e-5 * (t * t) + 2.433502 * log(t));
    case XH_ESAT_GOFFGRATCH46: {
      const double Tb = 373.16, eb = 101325;
      return eb * pow(10.0, -7.90298 * ((Tb / t) - 1) + 5.02808 * log10(Tb / t) + -1.3817e-7 * (pow(10.0, 11.344 * (1 - t / Tb)) - 1) +
                                8.1328e-3 * (pow(10.0, -3.49149 * ((Tb / t) - 1)) - 1));
    }
    case XH_ESAT_ITS90:
      return xh_esat_its90_water(t);
    case XH_ESAT_TETENS30:
      return xh_esat_magnus(t, 610.78, 17.269388, -35.86);
    case XH_ESAT_WMO08:
      return xh_esat_magnus(t, 611.2, 17.62, -30.04);
    case XH_ESAT_AERK96:
      return xh_esat_magnus(t, 610.94, 17.625, -30.12);
    default:  // buck81, and ecmwf over water
      return xh_esat_magnus(t, 611.21, 17.502, -32.19);
  }
}

__device__ __forceinline__ double xh_esat_ice(double t, int method) {
  switch (method) {
    case XH_ESAT_SONNTAG90:
      return 100 * exp(-6024.5282 / t + 24.7219 + 1.0613868e-2 * t + -1.3198825e-5 * (t * t) + -0.49382577 * log(t));
    case XH_ESAT_GOFFGRATCH46: {
      const double Tp = 273.16, ep = 611.73;
      return ep * pow(10.0, -9.09718 * ((Tp / t) - 1) + -3.56654 * log10(Tp / t) + 0.876793 * (1 - t / Tp));
    }
    case XH_ESAT_ITS90: {
      const double t2 = t * t;
      return exp(-5866.6426 / t + 22.32870244 + 1.39387003e-2 * t + -3.4262402e-5 * t2 + 2.7040955e-8 * (t2 * t) + 6.7063522e-1 * log(t));
    }
    case XH_ESAT_TETENS30:
      return xh_esat_magnus(t, 610.78, 21.8745584, -7.66);
    case XH_ESAT_WMO08:
      return xh_esat_magnus(t, 611.2, 22.46, -0.54);
    case XH_ESAT_BUCK81:
      return xh_esat_magnus(t, 611.15, 22.542, 0.32);
    default:  // aerk96, and ecmwf over ice
      return xh_esat_magnus(t, 611.21, 22.587, 0.7);
  }
}

// saturation_vapor_pressure (converters.py:585-600); t_ice, t_water and power are read only by the cases that have them
__device__ __forceinline__ double xh_esat_of(double t, int method, int kase, double t_ice, double t_water, double power) {
  if (kase == XH_ESAT_WATER) return xh_esat_water(t, method);
  const double w = xh_esat_water(t, method), i = xh_esat_ice(t, method);
  if (kase == XH_ESAT_BINARY) return t > t_ice ? w : i;
  if (t < t_ice) return i;
  if (t > t_water) return w;
  const double alpha = pow((t - t_ice) / (t_water - t_ice), power);
  return alpha * w + (1 - alpha) * i;
}
