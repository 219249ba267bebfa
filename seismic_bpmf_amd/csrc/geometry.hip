// Pair geometry: source-receiver distances (utils.compute_distances, BPMF/utils.py:1419-1498) and the three
// template-pair matrices of a TemplateGroup -- intertemplate_dist, dir_errors, ellipsoid_dist (BPMF/dataset.py:
// 4568-4688) -- with the masks the catalogue stages derive from the last one (:4815, :5262-5274).  The host
// definitions are postprocess.compute_distances_host, template_geometry_host, multiples_pair_mask and
// intertemplate_pair_mask; the geodesic is Vincenty's inverse of geodesic.h in place of the reference's cartopy call.
//
//   geo_distances_kernel      one thread per (source k, receiver r); a workgroup is one receiver and 256 sources, so
//                             the receiver's values have a workgroup-uniform address.  The receiver is the geodesic's
//                             first point, as in the reference's G.inverse(receiver, sources).
//   template_geometry_kernel  one thread per pair (t, u); a workgroup is one row t and 256 columns u.  Row values are
//                             uniform, column values are structure-of-arrays: lanes read them coalesced.  The thread
//                             computes dist[t, u], the direction of u from t once, and with it dir_errors[t, u] and
//                             dir_errors[u, t] -- the direction of t from u is the exact negation, so its norm and
//                             every product of the quadratic form are the same bits -- then ellipsoid_dist[t, u].
//   pair_mask_kernel          (T, T) float32 in, uint8 out: `<` a criterion (and optionally cc >= a similarity), or the
//                             transposed `not >` of compute_intertemplate_cc.
//
// The roundings are the reference's: epicentral = float32(metres / 1000); hypocentral = the root of
// epicentral^2 + dz^2 in float32 when every depth is float32, else epicentral^2 in float32 widened and the rest in
// float64, stored as float32.  Everything behind the geodesic is add / multiply / divide / sqrt, IEEE and unfused.
// No workspace and no floating-point atomics: an element depends on its own pair alone.  The one integer atomic
// counts the pairs Vincenty's iteration gave up on (they get pi (a + b) / 2).
#include "common.h"
#include "geodesic.h"
#include "../../include/bpmf_hip.h"

namespace bpmf {
namespace {

constexpr int GEO_THREADS = 256;
constexpr size_t GEO_MAX_ROWS = 65535;       // rows (grid.y) per launch; the launchers walk longer inputs in chunks

// the reference's two rounding steps behind the geodesic's metres (postprocess.hypocentral_from_metres); depths in km
__device__ __forceinline__ float geo_epicentral(double metres)
{
#pragma clang fp contract(off)
    return (float)(metres / 1000.0);
}

__device__ __forceinline__ float geo_hypocentral(float epi, double dep_src, double dep_rcv, bool depth_f64)
{
#pragma clang fp contract(off)
    const float e2 = epi * epi;
    if (depth_f64) {
        const double dz = dep_src - dep_rcv;
        return (float)sqrt((double)e2 + dz * dz);
    }
    const float dz = (float)dep_src - (float)dep_rcv;      // (both are float32 values: the narrowing is exact)
    return sqrtf(e2 + dz * dz);                            // (correctly rounded; __fsqrt_rn is the native approximation)
}

// src, rcv: (4, n) float64 tables -- longitude (degrees), sin and cos of the reduced latitude, depth (km)
__global__ __launch_bounds__(GEO_THREADS) void geo_distances_kernel(
    const double* __restrict__ src, size_t K, const double* __restrict__ rcv, size_t R, size_t r0, int depth_f64,
    float* __restrict__ hypo, float* __restrict__ epi_out, double* __restrict__ metres_out,
    int* __restrict__ nonconverged)
{
#pragma clang fp contract(off)
    const size_t r = r0 + blockIdx.y;
    const size_t k = (size_t)blockIdx.x * GEO_THREADS + threadIdx.x;
    if (k >= K || r >= R) return;
    bool conv;
    const double m = vin_length_checked_m(rcv[r], rcv[R + r], rcv[2 * R + r], src[k], src[K + k], src[2 * K + k], &conv);
    if (!conv) atomicAdd(nonconverged, 1);
    const float e = geo_epicentral(m);
    const size_t o = k * R + r;
    hypo[o] = geo_hypocentral(e, src[3 * K + k], rcv[3 * R + r], depth_f64 != 0);
    if (epi_out) epi_out[o] = e;
    if (metres_out) metres_out[o] = m;
}

// |sum_i (sum_j C_ij u_j) u_i| with j, then i, in index order; c: the matrix, element (i, j) at c[(3 i + j) stride]
__device__ __forceinline__ double geo_cov_dir(const double* __restrict__ c, size_t stride, double u0, double u1,
                                              double u2)
{
#pragma clang fp contract(off)
    const double r0 = (c[0] * u0 + c[stride] * u1) + c[2 * stride] * u2;
    const double r1 = (c[3 * stride] * u0 + c[4 * stride] * u1) + c[5 * stride] * u2;
    const double r2 = (c[6 * stride] * u0 + c[7 * stride] * u1) + c[8 * stride] * u2;
    return fabs((r0 * u0 + r1 * u1) + r2 * u2);
}

__device__ __forceinline__ float geo_dir_error(double cov_dir)
{
#pragma clang fp contract(off)
    return (float)sqrt(3.52 * cov_dir);
}

// geo: (4, T) as above (depths are float32 values); xyz: (3, T) Mercator x, y and the vertical coordinate;
// cov: (9, T), element (i, j) of template t at cov[(3 i + j) T + t], or null; has_cov: (T) or null (null: all have)
__global__ __launch_bounds__(GEO_THREADS) void template_geometry_kernel(
    const double* __restrict__ geo, const double* __restrict__ xyz, const double* __restrict__ cov,
    const uint8_t* __restrict__ has_cov, size_t T, size_t t0, float* __restrict__ dist, float* __restrict__ dir,
    float* __restrict__ ell, int* __restrict__ nonconverged)
{
#pragma clang fp contract(off)
    const size_t t = t0 + blockIdx.y;
    const size_t u = (size_t)blockIdx.x * GEO_THREADS + threadIdx.x;
    if (u >= T || t >= T) return;
    // dist[t, u]: source t, receiver u; the receiver is the geodesic's first point
    bool conv;
    const double m = vin_length_checked_m(geo[u], geo[T + u], geo[2 * T + u], geo[t], geo[T + t], geo[2 * T + t], &conv);
    if (!conv && nonconverged) atomicAdd(nonconverged, 1);
    const float d = geo_hypocentral(geo_epicentral(m), geo[3 * T + t], geo[3 * T + u], false);
    // the unit direction of u seen from t; 0 / 0 (u at t) is replaced by 0
    const double dx = xyz[u] - xyz[t], dy = xyz[T + u] - xyz[T + t], dz = xyz[2 * T + u] - xyz[2 * T + t];
    const double n = sqrt((dx * dx + dy * dy) + dz * dz);
    double u0 = dx / n, u1 = dy / n, u2 = dz / n;
    if (u0 != u0) u0 = 0.0;
    if (u1 != u1) u1 = 0.0;
    if (u2 != u2) u2 = 0.0;
    const bool cov_t = cov && (!has_cov || has_cov[t] != 0), cov_u = cov && (!has_cov || has_cov[u] != 0);
    const float e_tu = cov_t ? geo_dir_error(geo_cov_dir(cov + t, T, u0, u1, u2)) : 15.0f;
    const float e_ut = cov_u ? geo_dir_error(geo_cov_dir(cov + u, T, -u0, -u1, -u2)) : 15.0f;
    const size_t o = t * T + u;
    dist[o] = d;
    dir[o] = e_tu;
    ell[o] = (d - e_tu) - e_ut;
}

// mode BPMF_PAIR_MASK_MULTIPLES: mask[i, j] = ell[i, j] < criterion (& cc[i, j] >= similarity if cc);
// mode BPMF_PAIR_MASK_INTERTEMPLATE: mask[i, j] = !(ell[j, i] > criterion).  Compared in float64: a criterion that
// is a float32 value compares as in float32.
__global__ __launch_bounds__(GEO_THREADS) void pair_mask_kernel(const float* __restrict__ ell,
                                                                const float* __restrict__ cc, size_t T, size_t i0,
                                                                int mode, double criterion, double similarity,
                                                                uint8_t* __restrict__ mask)
{
    const size_t i = i0 + blockIdx.y;
    const size_t j = (size_t)blockIdx.x * GEO_THREADS + threadIdx.x;
    if (j >= T || i >= T) return;
    const size_t o = i * T + j;
    bool ok;
    if (mode == BPMF_PAIR_MASK_MULTIPLES) {
        ok = (double)ell[o] < criterion;
        if (cc) ok = ok & ((double)cc[o] >= similarity);
    } else {
        ok = !((double)ell[j * T + i] > criterion);
    }
    mask[o] = ok ? 1 : 0;
}

}  // namespace
}  // namespace bpmf

using namespace bpmf;

extern "C" int bpmf_geo_distances_dev(const double* d_sources, size_t K, const double* d_receivers, size_t R,
                                      int depth_float64, bpmf_stream_t stream_, float* d_hypocentral,
                                      float* d_epicentral, double* d_metres, int32_t* d_nonconverged)
{
    const char* me = "bpmf_geo_distances_dev";
    hipStream_t stream = (hipStream_t)stream_;
    if (!d_sources || !d_receivers || !d_hypocentral || !d_nonconverged) {
        set_error("%s: null pointer", me);
        return -1;
    }
    if (K == 0 || R == 0 || K > 0x7fffffffull || R > 0x7fffffffull) {
        set_error("%s: bad argument (K=%zu R=%zu)", me, K, R);
        return -1;
    }
    BPMF_HIP_CHECK(hipMemsetAsync(d_nonconverged, 0, sizeof(int32_t), stream));
    const unsigned nbx = (unsigned)((K + GEO_THREADS - 1) / GEO_THREADS);
    for (size_t r0 = 0; r0 < R; r0 += GEO_MAX_ROWS) {
        const size_t rows = R - r0 < GEO_MAX_ROWS ? R - r0 : GEO_MAX_ROWS;
        geo_distances_kernel<<<dim3(nbx, (unsigned)rows), dim3(GEO_THREADS), 0, stream>>>(
            d_sources, K, d_receivers, R, r0, depth_float64, d_hypocentral, d_epicentral, d_metres, d_nonconverged);
        BPMF_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int bpmf_template_geometry_dev(const double* d_geo, const double* d_xyz, const double* d_cov,
                                          const uint8_t* d_has_cov, size_t T, bpmf_stream_t stream_,
                                          float* d_intertemplate_dist, float* d_dir_errors, float* d_ellipsoid_dist,
                                          int32_t* d_nonconverged)
{
    const char* me = "bpmf_template_geometry_dev";
    hipStream_t stream = (hipStream_t)stream_;
    if (!d_geo || !d_xyz || !d_intertemplate_dist || !d_dir_errors || !d_ellipsoid_dist) {
        set_error("%s: null pointer", me);
        return -1;
    }
    if (T == 0 || T > 0x7fffffffull) {
        set_error("%s: bad argument (T=%zu)", me, T);
        return -1;
    }
    if (d_nonconverged) BPMF_HIP_CHECK(hipMemsetAsync(d_nonconverged, 0, sizeof(int32_t), stream));
    const unsigned nbx = (unsigned)((T + GEO_THREADS - 1) / GEO_THREADS);
    for (size_t t0 = 0; t0 < T; t0 += GEO_MAX_ROWS) {
        const size_t rows = T - t0 < GEO_MAX_ROWS ? T - t0 : GEO_MAX_ROWS;
        template_geometry_kernel<<<dim3(nbx, (unsigned)rows), dim3(GEO_THREADS), 0, stream>>>(
            d_geo, d_xyz, d_cov, d_has_cov, T, t0, d_intertemplate_dist, d_dir_errors, d_ellipsoid_dist,
            d_nonconverged);
        BPMF_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int bpmf_pair_mask_dev(const float* d_ellipsoid_dist, const float* d_intertemplate_cc, size_t T, int mode,
                                  double criterion, double similarity, bpmf_stream_t stream_, uint8_t* d_mask)
{
    const char* me = "bpmf_pair_mask_dev";
    hipStream_t stream = (hipStream_t)stream_;
    if (mode != BPMF_PAIR_MASK_MULTIPLES && mode != BPMF_PAIR_MASK_INTERTEMPLATE) {
        set_error("%s: unknown mode %d", me, mode);
        return -1;
    }
    if (!d_ellipsoid_dist || !d_mask) {
        set_error("%s: null pointer", me);
        return -1;
    }
    if (mode == BPMF_PAIR_MASK_INTERTEMPLATE && d_intertemplate_cc) {
        set_error("%s: the similarity test belongs to mode multiples", me);
        return -1;
    }
    if (T == 0 || T > 0x7fffffffull) {
        set_error("%s: bad argument (T=%zu)", me, T);
        return -1;
    }
    const unsigned nbx = (unsigned)((T + GEO_THREADS - 1) / GEO_THREADS);
    for (size_t i0 = 0; i0 < T; i0 += GEO_MAX_ROWS) {
        const size_t rows = T - i0 < GEO_MAX_ROWS ? T - i0 : GEO_MAX_ROWS;
        pair_mask_kernel<<<dim3(nbx, (unsigned)rows), dim3(GEO_THREADS), 0, stream>>>(
            d_ellipsoid_dist, d_intertemplate_cc, T, i0, mode, criterion, similarity, d_mask);
        BPMF_LAUNCH_CHECK();
    }
    return 0;
}
