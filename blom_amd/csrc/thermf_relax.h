// What the surface forcing routines of two experiment families share (stage_thermf_cesm.hip: cesm/mod_thermf_cesm.F90;
// stage_thermf_ben02.hip: ben02/mod_thermf_ben02.F90): the cubic interpolation in time of phy/mod_intp1d.F90 over five levels of a
// climatology or of the 48-level relaxation fluxes, and the column walk of the relaxation under the hybrid coordinates.  The two
// reference routines hold the same text for them (cesm :218-242, :279-303; ben02 :477-498, :535-556).
#pragma once
#include "blomgpu_internal.h"

#define NLEV_RLX 48      // levels of tflxap sflxap tflxdi sflxdi (phy/mod_forcing.F90:95-100)

// phy/mod_intp1d.F90:29-52
__device__ inline double intp1d_cesm(double d1, double d2, double d3, double d4, double d5, double x) {
  const double a1 = -3. / 7., a2 = -15. / 7., a3 = 3. / 2., b1 = 4. / 7., b2 = -16. / 7., b3 = 15. / 7., b4 = -5. / 7., b5 = 2. / 7.,
               c1 = -1. / 7., c2 = 9. / 14;
  const double a = a1 * (d1 + d5) + a2 * d3 + a3 * (d2 + d4);
  const double b = b1 * d1 + b2 * d2 + b3 * d3 + b4 * d4 + b5 * d5;
  const double cc = c1 * (d1 + d4) + c2 * (d2 + d3);
  return (a * x + b) * x + cc;
}
__device__ inline double intp5(gcd_t a, size_t np, int l1, int l2, int l3, int l4, int l5, double x) {
  return intp1d_cesm(a[(size_t)(l1 - 1) * np], a[(size_t)(l2 - 1) * np], a[(size_t)(l3 - 1) * np], a[(size_t)(l4 - 1) * np],
                     a[(size_t)(l5 - 1) * np], x);
}

// The column walk of the hybrid coordinate, :218-242 (x = temp, with t0deg added at the exit) and :279-303 (x = saln): the fractions of the
// relaxation flux that pass the kk+1 interfaces, and the mean of x over the relaxation depth.  Fortran leaves the loop at the first
// interface whose fraction turns negative (level k), having added x(k)*frac(k) (+ t0deg), and zeroes the interfaces k+1 .. kk+1; a
// column shallower than the relaxation depth never leaves it: nothing is zeroed and t0deg is never added.  Every interface is
// written exactly once here, with the value the two Fortran loops leave there.  The planes are level-major: a wavefront's store
// of a level is contiguous.  COLUMN_U levels of dp and x are requested before the first is used.
__device__ inline double rs_walk(gcd_t dp, gcd_t x, gd_t frac, size_t np, int kk, double dprsi, bool add_t0deg) {
  double cur = 1., mean = 0.;
  frac[0] = 1.;
  bool out = false;
  for (int k0 = 0; k0 < kk; k0 += COLUMN_U) {
    const int nu = kk - k0 < COLUMN_U ? kk - k0 : COLUMN_U;
    double d[COLUMN_U], v[COLUMN_U];
    if (!out) {
#pragma unroll
      for (int u = 0; u < COLUMN_U; u++)
        if (u < nu) { d[u] = dp[(size_t)(k0 + u) * np]; v[u] = x[(size_t)(k0 + u) * np]; }
    }
#pragma unroll
    for (int u = 0; u < COLUMN_U; u++) {
      if (u >= nu) break;
      double next = 0.;
      if (!out) {
        next = cur - d[u] * dprsi;
        if (next < 0.) {
          mean = mean + v[u] * cur;
          if (add_t0deg) mean = mean + T0DEG;
          out = true;
          next = 0.;
        } else {
          mean = mean + v[u] * (cur - next);
        }
        cur = next;
      }
      frac[(size_t)(k0 + u + 1) * np] = next;
    }
  }
  return mean;
}
