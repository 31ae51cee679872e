// The physical and numerical constants the kernels share: the values of the reference's phy/mod_constants.F90:31-56, under the upper-case
// names the kernels use.  The ONE definition of each (tests/test_shared_definitions.py); a stage's own parameters (DPEPS of cppm, remap,
// diffus and diazlv, EPSIL of finlyr, ...) are the reference's module-private values and stay with the stage.
#pragma once

constexpr double GRAV = 9.806;          // gravitational acceleration [m s-2]
constexpr double SPCIFH = 3990.;        // specific heat capacity of sea water [J kg-1 K-1]
constexpr double T0DEG = 273.15;        // 0 degrees Celsius [K]
constexpr double ALPHA0 = 1.e-3;        // reference specific volume [m3 kg-1]
constexpr double RHO0 = 1.e3;           // reference density [kg m-3]
constexpr double PI_BLOM = 3.1415926536;   // the reference's ten-digit pi
constexpr double EPSILPL = 1.e-14;      // small pressure times length
constexpr double EPSILP = 1.e-12;       // small pressure
constexpr double EPSILT = 1.e-11;       // small time
constexpr double SPVAL = 1.e33;         // the large "no value" number
// lengths as pressures [kg m-1 s-2]: one metre, centimetre, millimetre, micrometre of water
constexpr double ONEM = 9806.;
constexpr double ONECM = 98.06;
constexpr double ONEMM = 9.806;
constexpr double ONEMU = .009806;
constexpr double G2KG = 1.e-3, KG2G = 1.e3;   // grams to kilograms and back
