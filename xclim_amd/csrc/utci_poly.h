// utci_poly.h — the UTCI regression polynomial (Bröde et al. 2012, the operational procedure UTCI_a002): 210 coefficients of
// degree six in Ta [degC], va [m s-1], D_Tmrt = Tmrt - Ta [K] and Pa [kPa]; UTCI = Ta + sum c Ta^i va^j D^k Pa^l.
//
// XH_UTCI_TERMS(X) lists X(c, i, j, k, l) in the published order, which is the nest order Pa, D, va, Ta with every exponent
// ascending and all 210 monomials of degree <= 6 present: the flat index of a term is its rank in that enumeration.  The kernel
// takes the coefficients as a flat array and tests/thermalcpu.py parses the rows, so the table exists once.
#pragma once

#include <cmath>

#define XH_UTCI_NTERMS 210
#define XH_UTCI_TERMS(X) \
  X(6.07562052e-1, 0, 0, 0, 0) \
  X(-2.27712343e-2, 1, 0, 0, 0) \
  X(8.06470249e-4, 2, 0, 0, 0) \
  X(-1.54271372e-4, 3, 0, 0, 0) \
  X(-3.24651735e-6, 4, 0, 0, 0) \
  X(7.32602852e-8, 5, 0, 0, 0) \
  X(1.35959073e-9, 6, 0, 0, 0) \
  X(-2.25836520e0, 0, 1, 0, 0) \
  X(8.80326035e-2, 1, 1, 0, 0) \
  X(2.16844454e-3, 2, 1, 0, 0) \
  X(-1.53347087e-5, 3, 1, 0, 0) \
  X(-5.72983704e-7, 4, 1, 0, 0) \
  X(-2.55090145e-9, 5, 1, 0, 0) \
  X(-7.51269505e-1, 0, 2, 0, 0) \
  X(-4.08350271e-3, 1, 2, 0, 0) \
  X(-5.21670675e-5, 2, 2, 0, 0) \
  X(1.94544667e-6, 3, 2, 0, 0) \
  X(1.14099531e-8, 4, 2, 0, 0) \
  X(1.58137256e-1, 0, 3, 0, 0) \
  X(-6.57263143e-5, 1, 3, 0, 0) \
  X(2.22697524e-7, 2, 3, 0, 0) \
  X(-4.16117031e-8, 3, 3, 0, 0) \
  X(-1.27762753e-2, 0, 4, 0, 0) \
  X(9.66891875e-6, 1, 4, 0, 0) \
  X(2.52785852e-9, 2, 4, 0, 0) \
  X(4.56306672e-4, 0, 5, 0, 0) \
  X(-1.74202546e-7, 1, 5, 0, 0) \
  X(-5.91491269e-6, 0, 6, 0, 0) \
  X(3.98374029e-1, 0, 0, 1, 0) \
  X(1.83945314e-4, 1, 0, 1, 0) \
  X(-1.73754510e-4, 2, 0, 1, 0) \
  X(-7.60781159e-7, 3, 0, 1, 0) \
  X(3.77830287e-8, 4, 0, 1, 0) \
  X(5.43079673e-10, 5, 0, 1, 0) \
  X(-2.00518269e-2, 0, 1, 1, 0) \
  X(8.92859837e-4, 1, 1, 1, 0) \
  X(3.45433048e-6, 2, 1, 1, 0) \
  X(-3.77925774e-7, 3, 1, 1, 0) \
  X(-1.69699377e-9, 4, 1, 1, 0) \
  X(1.69992415e-4, 0, 2, 1, 0) \
  X(-4.99204314e-5, 1, 2, 1, 0) \
  X(2.47417178e-7, 2, 2, 1, 0) \
  X(1.07596466e-8, 3, 2, 1, 0) \
  X(8.49242932e-5, 0, 3, 1, 0) \
  X(1.35191328e-6, 1, 3, 1, 0) \
  X(-6.21531254e-9, 2, 3, 1, 0) \
  X(-4.99410301e-6, 0, 4, 1, 0) \
  X(-1.89489258e-8, 1, 4, 1, 0) \
  X(8.15300114e-8, 0, 5, 1, 0) \
  X(7.55043090e-4, 0, 0, 2, 0) \
  X(-5.65095215e-5, 1, 0, 2, 0) \
  X(-4.52166564e-7, 2, 0, 2, 0) \
  X(2.46688878e-8, 3, 0, 2, 0) \
  X(2.42674348e-10, 4, 0, 2, 0) \
  X(1.54547250e-4, 0, 1, 2, 0) \
  X(5.24110970e-6, 1, 1, 2, 0) \
  X(-8.75874982e-8, 2, 1, 2, 0) \
  X(-1.50743064e-9, 3, 1, 2, 0) \
  X(-1.56236307e-5, 0, 2, 2, 0) \
  X(-1.33895614e-7, 1, 2, 2, 0) \
  X(2.49709824e-9, 2, 2, 2, 0) \
  X(6.51711721e-7, 0, 3, 2, 0) \
  X(1.94960053e-9, 1, 3, 2, 0) \
  X(-1.00361113e-8, 0, 4, 2, 0) \
  X(-1.21206673e-5, 0, 0, 3, 0) \
  X(-2.18203660e-7, 1, 0, 3, 0) \
  X(7.51269482e-9, 2, 0, 3, 0) \
  X(9.79063848e-11, 3, 0, 3, 0) \
  X(1.25006734e-6, 0, 1, 3, 0) \
  X(-1.81584736e-9, 1, 1, 3, 0) \
  X(-3.52197671e-10, 2, 1, 3, 0) \
  X(-3.36514630e-8, 0, 2, 3, 0) \
  X(1.35908359e-10, 1, 2, 3, 0) \
  X(4.17032620e-10, 0, 3, 3, 0) \
  X(-1.30369025e-9, 0, 0, 4, 0) \
  X(4.13908461e-10, 1, 0, 4, 0) \
  X(9.22652254e-12, 2, 0, 4, 0) \
  X(-5.08220384e-9, 0, 1, 4, 0) \
  X(-2.24730961e-11, 1, 1, 4, 0) \
  X(1.17139133e-10, 0, 2, 4, 0) \
  X(6.62154879e-10, 0, 0, 5, 0) \
  X(4.03863260e-13, 1, 0, 5, 0) \
  X(1.95087203e-12, 0, 1, 5, 0) \
  X(-4.73602469e-12, 0, 0, 6, 0) \
  X(5.12733497e0, 0, 0, 0, 1) \
  X(-3.12788561e-1, 1, 0, 0, 1) \
  X(-1.96701861e-2, 2, 0, 0, 1) \
  X(9.99690870e-4, 3, 0, 0, 1) \
  X(9.51738512e-6, 4, 0, 0, 1) \
  X(-4.66426341e-7, 5, 0, 0, 1) \
  X(5.48050612e-1, 0, 1, 0, 1) \
  X(-3.30552823e-3, 1, 1, 0, 1) \
  X(-1.64119440e-3, 2, 1, 0, 1) \
  X(-5.16670694e-6, 3, 1, 0, 1) \
  X(9.52692432e-7, 4, 1, 0, 1) \
  X(-4.29223622e-2, 0, 2, 0, 1) \
  X(5.00845667e-3, 1, 2, 0, 1) \
  X(1.00601257e-6, 2, 2, 0, 1) \
  X(-1.81748644e-6, 3, 2, 0, 1) \
  X(-1.25813502e-3, 0, 3, 0, 1) \
  X(-1.79330391e-4, 1, 3, 0, 1) \
  X(2.34994441e-6, 2, 3, 0, 1) \
  X(1.29735808e-4, 0, 4, 0, 1) \
  X(1.29064870e-6, 1, 4, 0, 1) \
  X(-2.28558686e-6, 0, 5, 0, 1) \
  X(-3.69476348e-2, 0, 0, 1, 1) \
  X(1.62325322e-3, 1, 0, 1, 1) \
  X(-3.14279680e-5, 2, 0, 1, 1) \
  X(2.59835559e-6, 3, 0, 1, 1) \
  X(-4.77136523e-8, 4, 0, 1, 1) \
  X(8.64203390e-3, 0, 1, 1, 1) \
  X(-6.87405181e-4, 1, 1, 1, 1) \
  X(-9.13863872e-6, 2, 1, 1, 1) \
  X(5.15916806e-7, 3, 1, 1, 1) \
  X(-3.59217476e-5, 0, 2, 1, 1) \
  X(3.28696511e-5, 1, 2, 1, 1) \
  X(-7.10542454e-7, 2, 2, 1, 1) \
  X(-1.24382300e-5, 0, 3, 1, 1) \
  X(-7.38584400e-9, 1, 3, 1, 1) \
  X(2.20609296e-7, 0, 4, 1, 1) \
  X(-7.32469180e-4, 0, 0, 2, 1) \
  X(-1.87381964e-5, 1, 0, 2, 1) \
  X(4.80925239e-6, 2, 0, 2, 1) \
  X(-8.75492040e-8, 3, 0, 2, 1) \
  X(2.77862930e-5, 0, 1, 2, 1) \
  X(-5.06004592e-6, 1, 1, 2, 1) \
  X(1.14325367e-7, 2, 1, 2, 1) \
  X(2.53016723e-6, 0, 2, 2, 1) \
  X(-1.72857035e-8, 1, 2, 2, 1) \
  X(-3.95079398e-8, 0, 3, 2, 1) \
  X(-3.59413173e-7, 0, 0, 3, 1) \
  X(7.04388046e-7, 1, 0, 3, 1) \
  X(-1.89309167e-8, 2, 0, 3, 1) \
  X(-4.79768731e-7, 0, 1, 3, 1) \
  X(7.96079978e-9, 1, 1, 3, 1) \
  X(1.62897058e-9, 0, 2, 3, 1) \
  X(3.94367674e-8, 0, 0, 4, 1) \
  X(-1.18566247e-9, 1, 0, 4, 1) \
  X(3.34678041e-10, 0, 1, 4, 1) \
  X(-1.15606447e-10, 0, 0, 5, 1) \
  X(-2.80626406e0, 0, 0, 0, 2) \
  X(5.48712484e-1, 1, 0, 0, 2) \
  X(-3.99428410e-3, 2, 0, 0, 2) \
  X(-9.54009191e-4, 3, 0, 0, 2) \
  X(1.93090978e-5, 4, 0, 0, 2) \
  X(-3.08806365e-1, 0, 1, 0, 2) \
  X(1.16952364e-2, 1, 1, 0, 2) \
  X(4.95271903e-4, 2, 1, 0, 2) \
  X(-1.90710882e-5, 3, 1, 0, 2) \
  X(2.10787756e-3, 0, 2, 0, 2) \
  X(-6.98445738e-4, 1, 2, 0, 2) \
  X(2.30109073e-5, 2, 2, 0, 2) \
  X(4.17856590e-4, 0, 3, 0, 2) \
  X(-1.27043871e-5, 1, 3, 0, 2) \
  X(-3.04620472e-6, 0, 4, 0, 2) \
  X(5.14507424e-2, 0, 0, 1, 2) \
  X(-4.32510997e-3, 1, 0, 1, 2) \
  X(8.99281156e-5, 2, 0, 1, 2) \
  X(-7.14663943e-7, 3, 0, 1, 2) \
  X(-2.66016305e-4, 0, 1, 1, 2) \
  X(2.63789586e-4, 1, 1, 1, 2) \
  X(-7.01199003e-6, 2, 1, 1, 2) \
  X(-1.06823306e-4, 0, 2, 1, 2) \
  X(3.61341136e-6, 1, 2, 1, 2) \
  X(2.29748967e-7, 0, 3, 1, 2) \
  X(3.04788893e-4, 0, 0, 2, 2) \
  X(-6.42070836e-5, 1, 0, 2, 2) \
  X(1.16257971e-6, 2, 0, 2, 2) \
  X(7.68023384e-6, 0, 1, 2, 2) \
  X(-5.47446896e-7, 1, 1, 2, 2) \
  X(-3.59937910e-8, 0, 2, 2, 2) \
  X(-4.36497725e-6, 0, 0, 3, 2) \
  X(1.68737969e-7, 1, 0, 3, 2) \
  X(2.67489271e-8, 0, 1, 3, 2) \
  X(3.23926897e-9, 0, 0, 4, 2) \
  X(-3.53874123e-2, 0, 0, 0, 3) \
  X(-2.21201190e-1, 1, 0, 0, 3) \
  X(1.55126038e-2, 2, 0, 0, 3) \
  X(-2.63917279e-4, 3, 0, 0, 3) \
  X(4.53433455e-2, 0, 1, 0, 3) \
  X(-4.32943862e-3, 1, 1, 0, 3) \
  X(1.45389826e-4, 2, 1, 0, 3) \
  X(2.17508610e-4, 0, 2, 0, 3) \
  X(-6.66724702e-5, 1, 2, 0, 3) \
  X(3.33217140e-5, 0, 3, 0, 3) \
  X(-2.26921615e-3, 0, 0, 1, 3) \
  X(3.80261982e-4, 1, 0, 1, 3) \
  X(-5.45314314e-9, 2, 0, 1, 3) \
  X(-7.96355448e-4, 0, 1, 1, 3) \
  X(2.53458034e-5, 1, 1, 1, 3) \
  X(-6.31223658e-6, 0, 2, 1, 3) \
  X(3.02122035e-4, 0, 0, 2, 3) \
  X(-4.77403547e-6, 1, 0, 2, 3) \
  X(1.73825715e-6, 0, 1, 2, 3) \
  X(-4.09087898e-7, 0, 0, 3, 3) \
  X(6.14155345e-1, 0, 0, 0, 4) \
  X(-6.16755931e-2, 1, 0, 0, 4) \
  X(1.33374846e-3, 2, 0, 0, 4) \
  X(3.55375387e-3, 0, 1, 0, 4) \
  X(-5.13027851e-4, 1, 1, 0, 4) \
  X(1.02449757e-4, 0, 2, 0, 4) \
  X(-1.48526421e-3, 0, 0, 1, 4) \
  X(-4.11469183e-5, 1, 0, 1, 4) \
  X(-6.80434415e-6, 0, 1, 1, 4) \
  X(-9.77675906e-6, 0, 0, 2, 4) \
  X(8.82773108e-2, 0, 0, 0, 5) \
  X(-3.01859306e-3, 1, 0, 0, 5) \
  X(1.04452989e-3, 0, 1, 0, 5) \
  X(2.47090539e-4, 0, 0, 1, 5) \
  X(1.48348065e-3, 0, 0, 0, 6)

// The coefficients live in constant memory under an external name, so that the compiler reads them through the scalar cache
// (s_load, 16 dwords at a time, one SGPR operand per fma) and cannot turn them into 210 literals: kept as literals they are hoisted
// out of the row loop into 400 vector registers and the kernel runs at one wave per SIMD.  Include this header in ONE unit.
#define XH_UTCI_COEF(c, i, j, k, l) c,
__constant__ double xh_utci_coef[XH_UTCI_NTERMS] = {XH_UTCI_TERMS(XH_UTCI_COEF)};
#undef XH_UTCI_COEF

namespace xh_utci {

// monomials of degree <= d in n variables: C(d + n, n)
constexpr int count(int d, int n) {
  int r = 1;
  for (int q = 1; q <= n; ++q) r = r * (d + q) / q;
  return d < 0 ? 0 : r;
}
// the flat index of Ta^0 va^j D^k Pa^l
constexpr int base(int l, int k, int j) {
  int b = 0;
  for (int q = 0; q < l; ++q) b += count(6 - q, 3);
  for (int q = 0; q < k; ++q) b += count(6 - l - q, 2);
  for (int q = 0; q < j; ++q) b += count(6 - l - k - q, 1);
  return b;
}
static_assert(base(6, 0, 0) == XH_UTCI_NTERMS - 1 && base(0, 0, 1) == 7 && base(0, 1, 0) == 28 && base(1, 0, 0) == 84, "nest order");

// Horner in Ta inside va inside D inside Pa, one fma per coefficient: 209 fma for 210 terms, against about 800 multiplications
// and additions of the sum written term by term.  Indices are template arguments, so every coefficient is read at a constant,
// wave-uniform address.
template <int L, int K, int J, int I>
__device__ __forceinline__ double in_ta(const double* tab, double ta) {
  const double c = tab[base(L, K, J) + I];
  if constexpr (I == 6 - L - K - J)
    return c;
  else
    return fma(in_ta<L, K, J, I + 1>(tab, ta), ta, c);
}
template <int L, int K, int J>
__device__ __forceinline__ double in_va(const double* tab, double ta, double va) {
  if constexpr (J == 6 - L - K)
    return in_ta<L, K, J, 0>(tab, ta);
  else
    return fma(in_va<L, K, J + 1>(tab, ta, va), va, in_ta<L, K, J, 0>(tab, ta));
}
template <int L, int K>
__device__ __forceinline__ double in_dt(const double* tab, double ta, double va, double dt) {
  if constexpr (K == 6 - L)
    return in_va<L, K, 0>(tab, ta, va);
  else
    return fma(in_dt<L, K + 1>(tab, ta, va, dt), dt, in_va<L, K, 0>(tab, ta, va));
}
template <int L>
__device__ __forceinline__ double in_pa(const double* tab, double ta, double va, double dt, double pa) {
  if constexpr (L == 6)
    return in_dt<L, 0>(tab, ta, va, dt);
  else
    return fma(in_pa<L + 1>(tab, ta, va, dt, pa), pa, in_dt<L, 0>(tab, ta, va, dt));
}

// _utci (converters.py:2155-2376): Ta [degC], va [m s-1], dt = Tmrt - Ta [K], pa [kPa]
__device__ __forceinline__ double utci(double ta, double va, double dt, double pa) {
  const double* tab = xh_utci_coef;
#if defined(__HIP_DEVICE_COMPILE__)
  // the table's address passes through an (empty) statement the optimizer cannot see through, once per call: the loads stay
  // with their fma.  Left visible, all 210 are hoisted out of the caller's row loop into 420 scalar registers, which are then
  // kept in vector lanes and fetched back by two v_readlane per coefficient.
  asm volatile("" : "+s"(tab));
#endif
  return ta + in_pa<0>(tab, ta, va, dt, pa);
}

}  // namespace xh_utci
