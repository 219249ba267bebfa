// The cascade of second-order sections that svdwf.hip (the band-pass of utils.bandpass_filter) and spectrum.hip (the
// octave bands of the multi-band spectra) share, in SciPy's operation order; and Neumaier's compensated sum.  Both files
// are built with -ffp-contract=off: from equal input the cascade equals scipy.signal.sosfilt bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

namespace bpmf {

constexpr int SV_MAX_SECTIONS = 8;

struct SvFilter {
    const double* sos;              // (n_sections, 6) on the device
    int n_sections, detrend, taper, zerophase;
    double alpha;                   // of the Tukey taper, in (0, 1]
};

struct SvCascade {
    double b0[SV_MAX_SECTIONS], b1[SV_MAX_SECTIONS], b2[SV_MAX_SECTIONS], a1[SV_MAX_SECTIONS], a2[SV_MAX_SECTIONS];
    double z0[SV_MAX_SECTIONS], z1[SV_MAX_SECTIONS];
    int n;
    __device__ inline void load(const SvFilter& f)
    {
        n = f.n_sections;
#pragma unroll
        for (int s = 0; s < SV_MAX_SECTIONS; ++s) {
            const bool on = s < n;
            b0[s] = on ? f.sos[6 * s] : 1.0, b1[s] = on ? f.sos[6 * s + 1] : 0.0, b2[s] = on ? f.sos[6 * s + 2] : 0.0;
            a1[s] = on ? f.sos[6 * s + 4] : 0.0, a2[s] = on ? f.sos[6 * s + 5] : 0.0;
        }
    }
    __device__ inline void reset()
    {
#pragma unroll
        for (int s = 0; s < SV_MAX_SECTIONS; ++s) z0[s] = 0.0, z1[s] = 0.0;
    }
    __device__ inline double step(double x)
    {
#pragma unroll
        for (int s = 0; s < SV_MAX_SECTIONS; ++s) {
            if (s < n) {
                const double y = b0[s] * x + z0[s];
                z0[s] = (b1[s] * x - a1[s] * y) + z1[s];
                z1[s] = b2[s] * x - a2[s] * y;
                x = y;
            }
        }
        return x;
    }
};

// Neumaier's compensated sum
struct SvSum {
    double sum = 0.0, comp = 0.0;
    __device__ inline void add(double v)
    {
        const double t = sum + v;
        comp += fabs(sum) >= fabs(v) ? (sum - t) + v : (v - t) + sum;
        sum = t;
    }
    __device__ inline double value() const { return sum + comp; }
};

}  // namespace bpmf
