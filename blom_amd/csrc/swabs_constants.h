// The constants of mod_swabs (phy/mod_swabs.F90:96-183), once: the shortwave absorption of the two spectral bands.
//   Jerlov, N. G., 1968: Optical Oceanography. Elsevier, 194 pp.
//   Paulson, C. A., and J. J. Simpson, 1977: Irradiance Measurements in the Upper Ocean. J. Phys. Oceanogr., 7, 952-956.
//   Morel, A., and D. Antoine, 1994: Heating Rate within the Upper Ocean in Relation to Its Bio-Optical State. J. Phys. Oceanogr., 24,
//     1652-1665.
//   Ohlmann, J. C., 2003: Ocean Radiant Heating in Climate Models. J. Climate, 16, 1337-1352.
//   Sweeney, C., et al., 2005: Impacts of Shortwave Penetration Depth on Large-Scale Ocean Circulation and Heat Transport.
//     J. Phys. Oceanogr., 35, 1103-1118.
#pragma once

namespace swabs {
// Paulson and Simpson's (1977) fit to the data of Jerlov (1968), water types I, IA, IB, II, III (:104-107): fraction of the infrared and
// long visible wavelengths, and the attenuation lengths [m] of the two bands
constexpr double ps77_irfc[5] = {.58, .62, .67, .77, .78};
constexpr double ps77_al1[5] = {.35, .60, 1.00, 1.50, 1.40};
constexpr double ps77_al2[5] = {23.00, 20.00, 17.00, 14.00, 7.90};
// the modified Morel and Antoine (1994) parameterization (:120-128): the infrared fraction of Sweeney et al. (2005), and the polynomials in
// log10 of the chlorophyll concentration of the short band's fraction and of the two attenuation lengths
constexpr double ma94_irfc = .43;
constexpr double ma94_v2[6] = {.679, -.008, -.132, -.038, .017, .007};
constexpr double ma94_z1[6] = {1.540, -.197, .166, -.252, -.055, .042};
constexpr double ma94_z2[6] = {7.925, -6.644, 3.662, -1.815, -.218, .502};
// Ohlmann (2003), Table 1a (:131-174): chlorophyll concentration [mg m-3] and the parameters A1, A2, B1 [m-1], B2 [m-1]
constexpr int nval_tab1a = 31, nval_lut = 401;
constexpr double chl_tab1a[nval_tab1a] = {.001, .005, .01, .02, .03, .05, .10, .15, .20, .25, .30, .35, .40, .45, .50, .60,
                                          .70,  .80,  .90, 1.00, 1.50, 2.00, 2.50, 3.00, 4.00, 5.00, 6.00, 7.00, 8.00, 9.00, 10.00};
constexpr double a1_tab1a[nval_tab1a] = {0.4421,  0.4451,  0.4488,  0.4563,  0.4622,  0.4715,  0.4877,  0.4993,  0.5084,  0.5159, 0.5223,
                                         0.5278,  0.5326,  0.5369,  0.5408,  0.5474,  0.5529,  0.5576,  0.5615,  0.5649,  0.5757, 0.5802,
                                         0.5808,  0.5788,  0.56965, 0.55638, 0.54091, 0.52442, 0.50766, 0.49110, 0.47505};
constexpr double a2_tab1a[nval_tab1a] = {0.2981,  0.2963,  0.2940,  0.2894,  0.2858,  0.2800,  0.2703,  0.2628,  0.2571,  0.2523, 0.2481,
                                         0.2444,  0.2411,  0.2382,  0.2356,  0.2309,  0.2269,  0.2235,  0.2206,  0.2181,  0.2106, 0.2089,
                                         0.2113,  0.2167,  0.23357, 0.25504, 0.27829, 0.30274, 0.32698, 0.35056, 0.37303};
constexpr double b1_tab1a[nval_tab1a] = {0.0287,  0.0301,  0.0319,  0.0355,  0.0384,  0.0434,  0.0532,  0.0612,  0.0681,  0.0743, 0.0800,
                                         0.0853,  0.0902,  0.0949,  0.0993,  0.1077,  0.1154,  0.1227,  0.1294,  0.1359,  0.1640, 0.1876,
                                         0.2082,  0.2264,  0.25808, 0.28498, 0.30844, 0.32932, 0.34817, 0.36540, 0.38132};
constexpr double b2_tab1a[nval_tab1a] = {0.3192,  0.3243,  0.3306,  0.3433,  0.3537,  0.3705,  0.4031,  0.4262,  0.4456,  0.4621, 0.4763,
                                         0.4889,  0.4999,  0.5100,  0.5191,  0.5347,  0.5477,  0.5588,  0.5682,  0.5764,  0.6042, 0.6206,
                                         0.6324,  0.6425,  0.66172, 0.68144, 0.70086, 0.72144, 0.74178, 0.76190, 0.78155};
// the bounds of log10 of the chlorophyll concentration (:180-182)
constexpr double chl10_min = -2., chl10_max = 1.;
}  // namespace swabs
