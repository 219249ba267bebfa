// Vincenty's inverse on WGS84 as postprocess.geodesic_distance_m states it, operation for operation: |d lambda| <
// 1e-12, at most 200 iterations, pi (a + b) / 2 for a pair that does not converge; a lane that has converged stops
// iterating and its length comes from one evaluation at its final lambda.  Shared by bp_uncertainty.hip (the location
// uncertainties) and geometry.hip (source-receiver and template-pair distances): both give the same bits for the
// same pair.  The end points come in as longitude (degrees) and sine / cosine of the REDUCED latitude
// (postprocess.reduced_latitude_sin_cos, computed on the host).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

namespace bpmf {

constexpr double UNC_A = 6378137.0;                    // WGS84 semi-major axis, m
constexpr double UNC_F = 1.0 / 298.257223563;          // flattening
constexpr double UNC_B = (1.0 - UNC_F) * UNC_A;
constexpr double UNC_DEG2RAD = 3.141592653589793 / 180.0;
constexpr double UNC_TOL = 1e-12;
constexpr int UNC_MAX_ITER = 200;

struct VinAt {
    double sin_sig, cos_sig, sig, sin_al, cos2_al, cos_2sm;
};

// `at(lam)` of postprocess.geodesic_distance_m
__device__ __forceinline__ VinAt vin_at(double lam, double su1, double cu1, double su2, double cu2)
{
#pragma clang fp contract(off)
    VinAt v;
    double sl, cl;
    sincos(lam, &sl, &cl);
    v.sin_sig = hypot(cu2 * sl, cu1 * su2 - su1 * cu2 * cl);
    v.cos_sig = su1 * su2 + cu1 * cu2 * cl;
    v.sig = atan2(v.sin_sig, v.cos_sig);
    v.sin_al = v.sin_sig > 0.0 ? cu1 * cu2 * sl / v.sin_sig : 0.0;
    v.cos2_al = 1.0 - v.sin_al * v.sin_al;
    v.cos_2sm = v.cos2_al > 0.0 ? v.cos_sig - 2.0 * su1 * su2 / v.cos2_al : 0.0;
    return v;
}

// metres from (lon0, reduced latitude 1) to (lon, reduced latitude 2), degrees in
__device__ __forceinline__ double vin_length_m(double lon0, double su1, double cu1, double lon, double su2, double cu2)
{
#pragma clang fp contract(off)
    constexpr double f = UNC_F, a = UNC_A, b = UNC_B;
    // longitude difference in [-180, 180): Python's % (the sign of the divisor)
    double m = fmod(lon - lon0 + 180.0, 360.0);
    if (m < 0.0) m += 360.0;
    const double big_l = (m - 180.0) * UNC_DEG2RAD;
    double lam = big_l;
    bool done = false;
    for (int it = 0; it < UNC_MAX_ITER; ++it) {
        const VinAt v = vin_at(lam, su1, cu1, su2, cu2);
        const double c = f / 16.0 * v.cos2_al * (4.0 + f * (4.0 - 3.0 * v.cos2_al));
        const double nw = big_l + (1.0 - c) * f * v.sin_al *
                                      (v.sig + c * v.sin_sig * (v.cos_2sm + c * v.cos_sig * (-1.0 + 2.0 * v.cos_2sm * v.cos_2sm)));
        done = fabs(nw - lam) < UNC_TOL;
        lam = nw;
        if (done) break;
    }
    if (!done) return 3.141592653589793 * (a + b) / 2.0;
    const VinAt v = vin_at(lam, su1, cu1, su2, cu2);
    const double usq = v.cos2_al * (a * a - b * b) / (b * b);
    const double big_a = 1.0 + usq / 16384.0 * (4096.0 + usq * (-768.0 + usq * (320.0 - 175.0 * usq)));
    const double big_b = usq / 1024.0 * (256.0 + usq * (-128.0 + usq * (74.0 - 47.0 * usq)));
    const double d_sig =
        big_b * v.sin_sig *
        (v.cos_2sm + big_b / 4.0 * (v.cos_sig * (-1.0 + 2.0 * v.cos_2sm * v.cos_2sm) -
                                    big_b / 6.0 * v.cos_2sm * (-3.0 + 4.0 * v.sin_sig * v.sin_sig) *
                                        (-3.0 + 4.0 * v.cos_2sm * v.cos_2sm)));
    return b * big_a * (v.sig - d_sig);
}

// vin_length_m, the same operations, that also reports whether the iteration converged (*converged = false: the
// value is the fallback pi (a + b) / 2)
__device__ __forceinline__ double vin_length_checked_m(double lon0, double su1, double cu1, double lon, double su2,
                                                       double cu2, bool* converged)
{
#pragma clang fp contract(off)
    constexpr double f = UNC_F, a = UNC_A, b = UNC_B;
    double m = fmod(lon - lon0 + 180.0, 360.0);
    if (m < 0.0) m += 360.0;
    const double big_l = (m - 180.0) * UNC_DEG2RAD;
    double lam = big_l;
    bool done = false;
    for (int it = 0; it < UNC_MAX_ITER; ++it) {
        const VinAt v = vin_at(lam, su1, cu1, su2, cu2);
        const double c = f / 16.0 * v.cos2_al * (4.0 + f * (4.0 - 3.0 * v.cos2_al));
        const double nw = big_l + (1.0 - c) * f * v.sin_al *
                                      (v.sig + c * v.sin_sig * (v.cos_2sm + c * v.cos_sig * (-1.0 + 2.0 * v.cos_2sm * v.cos_2sm)));
        done = fabs(nw - lam) < UNC_TOL;
        lam = nw;
        if (done) break;
    }
    *converged = done;
    if (!done) return 3.141592653589793 * (a + b) / 2.0;
    const VinAt v = vin_at(lam, su1, cu1, su2, cu2);
    const double usq = v.cos2_al * (a * a - b * b) / (b * b);
    const double big_a = 1.0 + usq / 16384.0 * (4096.0 + usq * (-768.0 + usq * (320.0 - 175.0 * usq)));
    const double big_b = usq / 1024.0 * (256.0 + usq * (-128.0 + usq * (74.0 - 47.0 * usq)));
    const double d_sig =
        big_b * v.sin_sig *
        (v.cos_2sm + big_b / 4.0 * (v.cos_sig * (-1.0 + 2.0 * v.cos_2sm * v.cos_2sm) -
                                    big_b / 6.0 * v.cos_2sm * (-3.0 + 4.0 * v.sin_sig * v.sin_sig) *
                                        (-3.0 + 4.0 * v.cos_2sm * v.cos_2sm)));
    return b * big_a * (v.sig - d_sig);
}

}  // namespace bpmf
