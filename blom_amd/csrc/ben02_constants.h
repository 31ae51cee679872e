// The parameters of the forced ocean-ice experiment's slab thermodynamics, stated once: the nineteen data statements of the
// reference's ben02/mod_thdysi.F90:60-78 and the two parameters of ben02/mod_ben02.F90:119, :216, under upper-case names
// (stage_thermf_ben02.hip).  constants.h holds what every stage shares (phy/mod_constants.F90).
#pragma once

constexpr double ALBI_F = .70;          // max albedo over ice []
constexpr double ALBI_M = .60;          // max albedo over melting ice []
constexpr double ALBS_F = .85;          // albedo over snow []
constexpr double ALBS_M = .75;          // albedo over melting snow []
constexpr double RHOICE = 906.;         // density of ice [kg m-3]
constexpr double RHOSNW = 330.;         // density of snow [kg m-3]
constexpr double RKICE = 2.04;          // ice conductivity [W m-1 K-1]
constexpr double RKSNW = .31;           // snow conductivity [W m-1 K-1]
constexpr double FUSI = 3.02e8;         // heat of fusion of ice [J m-3]
constexpr double FUSS = 1.10e8;         // heat of fusion of snow [J m-3]
constexpr double FICE_MAX = .995;       // maximum fractional ice cover []
constexpr double TICE_M = 273.05;       // melting point of ice [K]
constexpr double TSNW_M = 273.15;       // melting point of snow [K]
constexpr double HICE_NHMN = .50;       // min. ice thickness northern hemisphere [m]
constexpr double HICE_SHMN = .30;       // min. ice thickness southern hemisphere [m]
constexpr double SAGETS = 2.e-7;        // snow aging timescale [s-1]
constexpr double SICE = 6.;             // salinity of sea ice [g kg-1]
constexpr double CWI = 0.006;           // ice-ocean heat transfer coefficient []
constexpr double CUC = 1.e3;            // heat flux of under-cooled water per kelvin [W m-2 K-1]
constexpr double RHOWAT = 1024.;        // density of sea water [kg m-3]
constexpr int NRFETS = 7;               // e-folding time scale of the runoff reservoir [days]
