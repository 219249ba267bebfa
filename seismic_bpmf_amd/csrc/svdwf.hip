// SVD-Wiener stack of a template's detections on the device (BPMF/utils.py: SVDWF :667-772, bandpass_filter :24-90;
// BPMF/dataset.py: EventGroup.SVDWF_stack :4275-4374; the definitions are postprocess.svdwf_host,
// bandpass_filter_host and svdwf_stack_host).  The input is float32, every operation in between float64.
//
// bpmf_svdwf_stack_dev serves a ragged batch of G groups x S x C channels.  A channel is the (n, m) matrix
// A = x[offsets[g] .. offsets[g + 1], s, c, :]; it owns one slot of the workspace, and as many channels as there are
// slots go through the kernels together (a slab):
//   1. sv_gram_kernel     the Gram matrix on the smaller side, K = min(n, m): A A^T (n <= m) or A^T A, 16 x 16 tiles
//                         through LDS, the products added in ascending order of the long index; the eigenvector
//                         matrix starts as the identity.  K odd: one zero row and column are added.
//   2. sv_jacobi_kernel   one workgroup per channel: two-sided cyclic Jacobi in a round-robin order.  A step holds
//                         K / 2 disjoint pairs (p, q); their rotations (tau = (g_qq - g_pp) / 2 g_pq,
//                         t = sign(tau) / (|tau| + sqrt(1 + tau^2))) are applied to the columns, then to the rows of
//                         the matrix and to the rows of the transposed eigenvector matrix (coalesced), in the global
//                         workspace.  A pair with |g_pq| <= 2^-52 sqrt(g_pp g_qq) is skipped; the solve ends with the
//                         first sweep that rotates nothing, or at the sweep cap (status 1, the channel's output is
//                         zeros).  A channel that holds a NaN or an Inf -- a diagonal element of its Gram matrix
//                         is not finite -- is not solved at all: status 1 as well.  Then: the eight largest eigenvalues, their sum with the rest (= sum sigma^2), and
//                         k = min(max_singular_values, 1 + first j with cumsum_j / sum >= expl_var); sum == 0: k = 0.
//   3. sv_project_kernel  P_j = a_j b_j^T for j < k: a_j = u_j, b_j = A^T u_j on the event side; b_j = v_j,
//                         a_j = A v_j on the sample side (= sigma_j u_j v_j^T either way; the sign cancels).
//   4. sv_window_kernel   first Wiener pass, factorised: the window sums of a_j and a_j^2 over the event axis, and
//                         noise_j = mean local variance = sum_i (sq_i / w - (sa_i / w)^2) sum_t b_t^2 / (n m).
//   5. sv_nan_kernel      a projection whose filtered form holds a NaN is skipped whole (only looked for where
//                         noise_j is not a positive number: elsewhere no NaN can arise from finite input).
//   6. sv_sum_kernel      D = sum_j F_j, F = where(var < noise, mean, (p - mean)(1 - noise / var) + mean).
//   7. sv_column_kernel / sv_second_kernel   second pass on D: one thread per sample column walks the events with
//                         running window sums; first the column's sum of local variances, then (noise = their mean
//                         over the whole matrix, reduced by every workgroup in the same order) the result, NaN and
//                         +-Inf -> 0.
//   8. sv_filter_kernel   the zero-phase band-pass of every row in place, one thread per row (bpmf_bandpass_rows_dev
//                         runs the same code on any (rows, m) table): mean, least-squares line, Tukey taper, then the
//                         cascade in SciPy's operation order -- y = b0 x + z0; z0 = (b1 x - a1 y) + z1;
//                         z1 = b2 x - a2 y, sections innermost -- forward and on the reversed row, from zero state.
//                         Built with -ffp-contract=off: without detrend and taper the result is SciPy's bit for bit.
//   9. sv_stack_kernel    filtered = (float) result; stack = float64 mean over the events of the float32 values,
//                         divided by its signed maximum (0 -> 1), rounded to float32; n_singular and status.
// A channel's arithmetic depends on its own (n, m) only: the same channel gives the same bits in any batch and slab.
// Plain vector stores, no atomics on global memory; every element of every output is written.
#include "common.h"
#include "sos_cascade.h"
#include <cmath>
#include "../../include/bpmf_hip.h"

namespace bpmf {

constexpr int SV_MAX_SMALL = 512;                      // min(n, m): the Gram matrix one workgroup diagonalises
constexpr int SV_MAX_LARGE = 16384;                    // max(n, m)
constexpr int SV_MAX_RANK = 8;
constexpr int SV_MAX_WINDOW = 65536;                   // wiener_colsize
constexpr int SV_THREADS = 256;
constexpr int SV_JACOBI_THREADS = 1024;
constexpr int SV_FILTER_THREADS = 64;
constexpr int SV_MAX_SLAB = 65535;                     // gridDim.y
constexpr size_t SV_MAX_ROW_LENGTH = 1u << 24;         // bpmf_bandpass_rows_dev

// the scalars of a slot
enum { SM_LAMBDA = 0, SM_TOTAL = 8, SM_K = 9, SM_NOISE = 10, SM_SKIP = 18, SM_STATUS = 26, SM_SWEEPS = 27,
       SM_INDEX = 28, SM_COUNT = 40 };

struct SvCall {
    const float* x;                 // (N, S, C, m)
    const long long* offsets;       // (G + 1), in the workspace
    double* slots;
    size_t slot;                    // doubles per slot
    size_t o_v, o_a, o_b, o_sa, o_sq, o_d, o_e, o_col, o_small;
    long long job0;                 // the slab's first channel, g * SC + sc
    int SC, m, w;                   // w = 0: the group's size
};

struct SvSizes {
    size_t slot, o_v, o_a, o_b, o_sa, o_sq, o_d, o_e, o_col, o_small;
};

static SvSizes sv_sizes(size_t n_max, size_t m)
{
    const size_t K = n_max < m ? n_max : m, Kp = K + (K & 1);
    SvSizes z{};
    size_t at = Kp * Kp;
    z.o_v = at, at += Kp * Kp;
    z.o_a = at, at += SV_MAX_RANK * n_max;
    z.o_b = at, at += SV_MAX_RANK * m;
    z.o_sa = at, at += SV_MAX_RANK * n_max;
    z.o_sq = at, at += SV_MAX_RANK * n_max;
    z.o_d = at, at += n_max * m;
    z.o_e = at, at += n_max * m;
    z.o_col = at, at += m;
    z.o_small = at, at += SM_COUNT;
    z.slot = align_up(at, 32);
    return z;
}

// The workspace: the offsets table, then `n_slots` slots of `slot` doubles (a multiple of 32: 256 bytes) each.
struct SvWorkspace { long long* offsets; double* slots; size_t head, bytes; };

static SvWorkspace sv_carve(void* base, size_t n_groups, size_t n_slots, size_t slot)
{
    SvWorkspace ws;
    Carver c(base);
    ws.offsets = c.take<long long>(n_groups + 1);
    ws.head = c.offset();
    ws.slots = c.take<double>(n_slots * slot);
    ws.bytes = c.bytes();
    return ws;
}

struct SvChannel {
    const float* A;                 // element (i, t) at A[i * ld + t]
    size_t ld;
    long long row0, job;
    int n, m, K, Kp, side, w;       // side 0: Gram matrix over the events, 1: over the samples
    double *G, *V, *a, *b, *sa, *sq, *D, *E, *col, *small;
};

__device__ inline SvChannel sv_channel(const SvCall& c, unsigned in_slab)
{
    SvChannel ch;
    ch.job = c.job0 + in_slab;
    const long long g = ch.job / c.SC, sc = ch.job - g * c.SC;
    ch.row0 = c.offsets[g];
    ch.n = (int)(c.offsets[g + 1] - ch.row0);
    ch.m = c.m;
    ch.side = ch.n <= ch.m ? 0 : 1;
    ch.K = ch.side == 0 ? ch.n : ch.m;
    ch.Kp = ch.K + (ch.K & 1);
    ch.w = c.w > 0 ? c.w : ch.n;
    ch.ld = (size_t)c.SC * (size_t)c.m;
    ch.A = c.x + ((size_t)ch.row0 * (size_t)c.SC + (size_t)sc) * (size_t)c.m;
    double* s = c.slots + (size_t)in_slab * c.slot;
    ch.G = s, ch.V = s + c.o_v, ch.a = s + c.o_a, ch.b = s + c.o_b, ch.sa = s + c.o_sa, ch.sq = s + c.o_sq;
    ch.D = s + c.o_d, ch.E = s + c.o_e, ch.col = s + c.o_col, ch.small = s + c.o_small;
    return ch;
}

__global__ __launch_bounds__(256) void sv_gram_kernel(const SvCall call)
{
    const SvChannel ch = sv_channel(call, blockIdx.y);
    if (ch.n == 0) return;
    const int tiles = (ch.Kp + 15) / 16;
    if ((int)blockIdx.x >= tiles * tiles) return;
    const int r0 = ((int)blockIdx.x / tiles) * 16, c0 = ((int)blockIdx.x % tiles) * 16;
    __shared__ double sA[16][17], sB[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int K = ch.K, L = ch.side == 0 ? ch.m : ch.n;
    double acc = 0.0;
    for (int k0 = 0; k0 < L; k0 += 16) {
        if (ch.side == 0) {                                            // rows of A: consecutive lanes, consecutive t
            const int k = k0 + tx, ra = r0 + ty, rb = c0 + ty;
            sA[ty][tx] = ra < K && k < L ? (double)ch.A[(size_t)ra * ch.ld + k] : 0.0;
            sB[ty][tx] = rb < K && k < L ? (double)ch.A[(size_t)rb * ch.ld + k] : 0.0;
        } else {                                                       // columns of A: consecutive lanes, consecutive t
            const int k = k0 + ty, ra = r0 + tx, rb = c0 + tx;
            sA[tx][ty] = ra < K && k < L ? (double)ch.A[(size_t)k * ch.ld + ra] : 0.0;
            sB[tx][ty] = rb < K && k < L ? (double)ch.A[(size_t)k * ch.ld + rb] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) acc += sA[ty][kk] * sB[tx][kk];
        __syncthreads();
    }
    const int p = r0 + ty, q = c0 + tx;
    if (p < ch.Kp && q < ch.Kp) {
        ch.G[(size_t)p * ch.Kp + q] = acc;
        ch.V[(size_t)p * ch.Kp + q] = p == q ? 1.0 : 0.0;
    }
}

__global__ __launch_bounds__(SV_JACOBI_THREADS) void sv_jacobi_kernel(const SvCall call, int max_sweeps,
                                                                      double expl_var, int max_rank)
{
    const SvChannel ch = sv_channel(call, blockIdx.x);
    if (ch.n == 0) return;
    __shared__ double rot_c[SV_MAX_SMALL / 2], rot_s[SV_MAX_SMALL / 2];
    __shared__ short rot_p[SV_MAX_SMALL / 2], rot_q[SV_MAX_SMALL / 2];
    __shared__ double red[SV_JACOBI_THREADS];
    __shared__ int red_i[SV_JACOBI_THREADS];
    __shared__ double lam[SV_MAX_SMALL];
    __shared__ int rotated;
    const int tid = threadIdx.x, K = ch.K, Kp = ch.Kp, half = Kp / 2, M1 = Kp - 1;
    double* __restrict__ G = ch.G;
    double* __restrict__ V = ch.V;
    const double eps = 2.220446049250313e-16;                          // 2^-52
    int status = 1, sweeps = 0;
    // every sample is squared into one diagonal element: a NaN or an Inf anywhere in the channel shows there
    if (tid == 0) rotated = 0;
    __syncthreads();
    for (int d = tid; d < K; d += SV_JACOBI_THREADS) {
        const double g = G[(size_t)d * Kp + d];
        if (!(g - g == 0.0)) rotated = 1;
    }
    __syncthreads();
    if (rotated) max_sweeps = 0;                                       // not solved: status 1
    __syncthreads();
    for (int sweep = 0; sweep < max_sweeps; ++sweep) {
        if (tid == 0) rotated = 0;
        __syncthreads();
        for (int step = 0; step < M1; ++step) {
            if (tid < half) {
                // round robin: the last index stays, the others turn
                int a = (step + tid) % M1, b = tid == 0 ? M1 : (step + M1 - tid) % M1;
                const int p = a < b ? a : b, q = a < b ? b : a;
                const double gpp = G[(size_t)p * Kp + p], gqq = G[(size_t)q * Kp + q], gpq = G[(size_t)p * Kp + q];
                double c = 1.0, s = 0.0;
                if (!(fabs(gpq) <= eps * (sqrt(fabs(gpp)) * sqrt(fabs(gqq))))) {
                    const double tau = (gqq - gpp) / (2.0 * gpq);
                    const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                    c = 1.0 / sqrt(1.0 + t * t);
                    s = t * c;
                    if (s != 0.0) rotated = 1;
                }
                rot_p[tid] = (short)p, rot_q[tid] = (short)q, rot_c[tid] = c, rot_s[tid] = s;
            }
            __syncthreads();
            for (int idx = tid; idx < half * Kp; idx += SV_JACOBI_THREADS) {       // columns p and q of every row
                const int pair = idx % half, r = idx / half;
                const double s = rot_s[pair];
                if (s == 0.0) continue;
                const double c = rot_c[pair];
                const size_t ip = (size_t)r * Kp + rot_p[pair], iq = (size_t)r * Kp + rot_q[pair];
                const double x = G[ip], y = G[iq];
                G[ip] = c * x - s * y;
                G[iq] = s * x + c * y;
            }
            __syncthreads();
            for (int idx = tid; idx < half * Kp; idx += SV_JACOBI_THREADS) {       // rows p and q, matrix and vectors
                const int col = idx % Kp, pair = idx / Kp;
                const double s = rot_s[pair];
                if (s == 0.0) continue;
                const double c = rot_c[pair];
                const int p = rot_p[pair], q = rot_q[pair];
                const size_t ip = (size_t)p * Kp + col, iq = (size_t)q * Kp + col;
                const double x = G[ip], y = G[iq];
                G[ip] = col == q ? 0.0 : c * x - s * y;                // the rotated element is zero by construction
                G[iq] = col == p ? 0.0 : s * x + c * y;
                const double vx = V[ip], vy = V[iq];
                V[ip] = c * vx - s * vy;
                V[iq] = s * vx + c * vy;
            }
            __syncthreads();
        }
        sweeps = sweep + 1;
        const int any = rotated;
        __syncthreads();
        if (!any) {
            status = 0;
            break;
        }
    }

    // eigenvalues: the sum of all, the largest eight in descending order (equal values: the lower index first)
    if (tid < SV_MAX_SMALL) lam[tid] = tid < K ? G[(size_t)tid * Kp + tid] : -INFINITY;
    red[tid] = tid < K ? fmax(G[(size_t)tid * Kp + tid], 0.0) : 0.0;
    __syncthreads();
    for (int o = SV_JACOBI_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] = red[tid] + red[tid + o];
        __syncthreads();
    }
    const double total = red[0];
    __syncthreads();
    const int n_top = K < SV_MAX_RANK ? K : SV_MAX_RANK;
    for (int j = 0; j < n_top; ++j) {
        red[tid] = tid < SV_MAX_SMALL ? lam[tid] : -INFINITY;
        red_i[tid] = tid;
        __syncthreads();
        for (int o = SV_JACOBI_THREADS / 2; o > 0; o >>= 1) {
            if (tid < o) {
                const double other = red[tid + o];
                const int other_i = red_i[tid + o];
                if (other > red[tid] || (other == red[tid] && other_i < red_i[tid])) {
                    red[tid] = other;
                    red_i[tid] = other_i;
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            ch.small[SM_LAMBDA + j] = red[0];
            ch.small[SM_INDEX + j] = (double)red_i[0];
            lam[red_i[0]] = -INFINITY;
        }
        __syncthreads();
    }
    if (tid == 0) {
        int k = 0;
        if (status == 0 && total > 0.0) {
            k = max_rank < n_top ? max_rank : n_top;
            double cum = 0.0;
            for (int j = 0; j < n_top && j < max_rank; ++j) {
                cum += fmax(ch.small[SM_LAMBDA + j], 0.0);
                if (cum / total >= expl_var) {
                    k = j + 1;
                    break;
                }
            }
        }
        ch.small[SM_TOTAL] = total;
        ch.small[SM_K] = (double)k;
        ch.small[SM_STATUS] = (double)status;
        ch.small[SM_SWEEPS] = (double)sweeps;
        for (int j = 0; j < SV_MAX_RANK; ++j) ch.small[SM_SKIP + j] = 0.0, ch.small[SM_NOISE + j] = 0.0;
    }
}

__global__ __launch_bounds__(SV_THREADS) void sv_project_kernel(const SvCall call)
{
    const SvChannel ch = sv_channel(call, blockIdx.y);
    if (ch.n == 0) return;
    const int k = (int)ch.small[SM_K], n = ch.n, m = ch.m, Kp = ch.Kp;
    const int gtid = blockIdx.x * SV_THREADS + threadIdx.x, gsize = gridDim.x * SV_THREADS;
    for (int j = 0; j < k; ++j) {
        const double* __restrict__ v = ch.V + (size_t)(int)ch.small[SM_INDEX + j] * Kp;
        double* __restrict__ a = ch.a + (size_t)j * n;
        double* __restrict__ b = ch.b + (size_t)j * m;
        if (ch.side == 0) {
            for (int i = gtid; i < n; i += gsize) a[i] = v[i];
            for (int t = gtid; t < m; t += gsize) {
                double acc = 0.0;
                for (int i = 0; i < n; ++i) acc += v[i] * (double)ch.A[(size_t)i * ch.ld + t];
                b[t] = acc;
            }
        } else {
            for (int t = gtid; t < m; t += gsize) b[t] = v[t];
            const int lane = threadIdx.x & 63, wave = gtid >> 6, n_waves = gsize >> 6;
            for (int i = wave; i < n; i += n_waves) {                  // one wavefront per event
                double acc = 0.0;
                for (int t = lane; t < m; t += 64) acc += (double)ch.A[(size_t)i * ch.ld + t] * v[t];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
                if (lane == 0) a[i] = acc;
            }
        }
    }
}

// the sum of v over the block's threads, the same tree in every block; every thread calls it
__device__ inline double sv_block_sum(double v, double* red, int tid)
{
    red[tid] = v;
    __syncthreads();
    for (int o = SV_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] = red[tid] + red[tid + o];
        __syncthreads();
    }
    const double total = red[0];
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(SV_THREADS) void sv_window_kernel(const SvCall call)
{
    const SvChannel ch = sv_channel(call, blockIdx.x);
    if (ch.n == 0 || ch.w == 1) return;
    __shared__ double red[SV_THREADS];
    const int k = (int)ch.small[SM_K], n = ch.n, m = ch.m, tid = threadIdx.x;
    const long long lo = ch.w / 2, hi = (ch.w - 1) / 2;
    const double w = (double)ch.w;
    for (int j = 0; j < k; ++j) {
        const double* __restrict__ a = ch.a + (size_t)j * n;
        const double* __restrict__ b = ch.b + (size_t)j * m;
        double part = 0.0;
        for (int i = tid; i < n; i += SV_THREADS) {
            const int first = i - lo < 0 ? 0 : (int)(i - lo), last = i + hi > n - 1 ? n - 1 : (int)(i + hi);
            double s1 = 0.0, s2 = 0.0;
            for (int r = first; r <= last; ++r) {
                s1 += a[r];
                s2 += a[r] * a[r];
            }
            ch.sa[(size_t)j * n + i] = s1;
            ch.sq[(size_t)j * n + i] = s2;
            part += s2 / w - (s1 / w) * (s1 / w);
        }
        const double sum_c = sv_block_sum(part, red, tid);
        part = 0.0;
        for (int t = tid; t < m; t += SV_THREADS) part += b[t] * b[t];
        const double sum_b = sv_block_sum(part, red, tid);
        if (tid == 0) ch.small[SM_NOISE + j] = sum_c * sum_b / ((double)n * (double)m);
    }
}

// scipy.signal.wiener's last three lines for one element
__device__ inline double sv_wiener(double p, double mean, double var, double noise)
{
    const double res = (p - mean) * (1.0 - noise / var) + mean;
    return var < noise ? mean : res;
}

__device__ inline double sv_first_pass(double a, double b, double sa, double sq, double w, double noise)
{
    const double mean = sa * b / w;
    return sv_wiener(a * b, mean, sq * (b * b) / w - mean * mean, noise);
}

__global__ __launch_bounds__(SV_THREADS) void sv_nan_kernel(const SvCall call)
{
    const SvChannel ch = sv_channel(call, blockIdx.y);
    if (ch.n == 0 || ch.w == 1) return;
    const int k = (int)ch.small[SM_K], n = ch.n, m = ch.m;
    const size_t count = (size_t)n * m, gsize = (size_t)gridDim.x * SV_THREADS;
    const double w = (double)ch.w;
    for (int j = 0; j < k; ++j) {
        const double noise = ch.small[SM_NOISE + j];
        if (noise > 0.0 && noise < INFINITY) continue;                 // finite input: no NaN can arise
        bool bad = false;
        for (size_t idx = (size_t)blockIdx.x * SV_THREADS + threadIdx.x; idx < count; idx += gsize) {
            const size_t i = idx / m, t = idx - i * m;
            const double f = sv_first_pass(ch.a[(size_t)j * n + i], ch.b[(size_t)j * m + t], ch.sa[(size_t)j * n + i],
                                           ch.sq[(size_t)j * n + i], w, noise);
            bad = bad || f != f;
        }
        if (bad) ch.small[SM_SKIP + j] = 1.0;
    }
}

__global__ __launch_bounds__(SV_THREADS) void sv_sum_kernel(const SvCall call)
{
    const SvChannel ch = sv_channel(call, blockIdx.y);
    if (ch.n == 0) return;
    const int k = (int)ch.small[SM_K], n = ch.n, m = ch.m;
    if (k == 0) return;
    const size_t count = (size_t)n * m, gsize = (size_t)gridDim.x * SV_THREADS;
    const double w = (double)ch.w;
    for (size_t idx = (size_t)blockIdx.x * SV_THREADS + threadIdx.x; idx < count; idx += gsize) {
        const size_t i = idx / m, t = idx - i * m;
        double acc = 0.0;
        for (int j = 0; j < k; ++j) {
            if (ch.small[SM_SKIP + j] != 0.0) continue;
            const double a = ch.a[(size_t)j * n + i], b = ch.b[(size_t)j * m + t];
            acc += ch.w == 1 ? a * b
                             : sv_first_pass(a, b, ch.sa[(size_t)j * n + i], ch.sq[(size_t)j * n + i], w,
                                             ch.small[SM_NOISE + j]);
        }
        if (ch.w == 1) ch.E[idx] = acc - acc == 0.0 ? acc : 0.0;       // no second pass: NaN and +-Inf -> 0
        else ch.D[idx] = acc;
    }
}

// One sample column of the second pass: the events are walked with running sums over rows i - lo .. i + hi.
// f(i, mean, var) is called for every event in order.
template <typename F>
__device__ inline void sv_walk_column(const double* __restrict__ D, int n, int m, int t, int w, const F& f)
{
    const long long lo = w / 2, hi = (w - 1) / 2;
    const double dw = (double)w;
    double s1 = 0.0, s2 = 0.0;
    const int head = hi < n - 1 ? (int)hi : n - 1;
    for (int r = 0; r <= head; ++r) {
        const double v = D[(size_t)r * m + t];
        s1 += v;
        s2 += v * v;
    }
    for (int i = 0; i < n; ++i) {
        const double mean = s1 / dw;
        f(i, mean, s2 / dw - mean * mean);
        const long long enter = i + 1 + hi, leave = i - lo;
        if (enter < n) {
            const double v = D[(size_t)enter * m + t];
            s1 += v;
            s2 += v * v;
        }
        if (leave >= 0) {
            const double v = D[(size_t)leave * m + t];
            s1 -= v;
            s2 -= v * v;
        }
    }
}

__global__ __launch_bounds__(SV_THREADS) void sv_column_kernel(const SvCall call)
{
    const SvChannel ch = sv_channel(call, blockIdx.y);
    if (ch.n == 0 || ch.w == 1 || (int)ch.small[SM_K] == 0) return;
    const int t = blockIdx.x * SV_THREADS + threadIdx.x;
    if (t >= ch.m) return;
    double acc = 0.0;
    sv_walk_column(ch.D, ch.n, ch.m, t, ch.w, [&](int, double, double var) { acc += var; });
    ch.col[t] = acc;
}

__global__ __launch_bounds__(SV_THREADS) void sv_second_kernel(const SvCall call)
{
    const SvChannel ch = sv_channel(call, blockIdx.y);
    if (ch.n == 0 || ch.w == 1 || (int)ch.small[SM_K] == 0) return;
    if ((int)blockIdx.x * SV_THREADS >= ch.m) return;
    __shared__ double red[SV_THREADS];
    const int tid = threadIdx.x, n = ch.n, m = ch.m;
    double part = 0.0;
    for (int c = tid; c < m; c += SV_THREADS) part += ch.col[c];
    const double noise = sv_block_sum(part, red, tid) / ((double)n * (double)m);
    const int t = blockIdx.x * SV_THREADS + tid;
    if (t >= m) return;
    const double* __restrict__ D = ch.D;
    double* __restrict__ E = ch.E;
    sv_walk_column(D, n, m, t, ch.w, [&](int i, double mean, double var) {
        const double f = sv_wiener(D[(size_t)i * m + t], mean, var, noise);
        E[(size_t)i * m + t] = f - f == 0.0 ? f : 0.0;
    });
}

// scipy.signal.windows.tukey(m, alpha)[i]
__device__ inline double sv_tukey(int i, int m, double alpha)
{
    if (m <= 1) return 1.0;
    const double pi = 3.141592653589793;
    const int width = (int)floor(alpha * (double)(m - 1) / 2.0);
    if (i >= m - width - 1) return 0.5 * (1.0 + cos(pi * (-2.0 / alpha + 1.0 + 2.0 * (double)i / alpha / (double)(m - 1))));
    if (i <= width) return 0.5 * (1.0 + cos(pi * (-1.0 + 2.0 * (double)i / alpha / (double)(m - 1))));
    return 1.0;
}

// One row of utils.bandpass_filter.  `y` (float64, m) takes the forward pass of a zero-phase call; it may be `x` or
// `out` themselves where these are float64 (element t is read before it is written).
template <typename Tin, typename Tout>
__device__ inline void sv_filter_row(const Tin* x, double* y, Tout* out, int m, const SvFilter& f)
{
    SvCascade cas;
    cas.load(f);
    double mean = 0.0, slope = 0.0, rest = 0.0;
    const double centre = (double)(m - 1) / 2.0;
    if (f.detrend) {                                                   // (compensated sums: the order does not show)
        SvSum s0;
        for (int t = 0; t < m; ++t) s0.add((double)x[t]);
        mean = s0.value() / (double)m;
        SvSum num, den, left;
        for (int t = 0; t < m; ++t) {
            const double d = (double)t - centre, v = (double)x[t] - mean;
            num.add(v * d);
            den.add(d * d);
            left.add(v);
        }
        rest = left.value() / (double)m;
        slope = den.value() > 0.0 ? num.value() / den.value() : 0.0;
    }
    cas.reset();
    for (int t = 0; t < m; ++t) {
        double v = (double)x[t];
        if (f.detrend) v = (v - mean) - (slope * ((double)t - centre) + rest);
        if (f.taper) v = v * sv_tukey(t, m, f.alpha);
        v = cas.step(v);
        if (f.zerophase) y[t] = v;
        else out[t] = (Tout)v;
    }
    if (!f.zerophase) return;
    cas.reset();
    for (int t = m - 1; t >= 0; --t) out[t] = (Tout)cas.step(y[t]);
}

__global__ __launch_bounds__(SV_FILTER_THREADS) void sv_filter_kernel(const SvCall call, const SvFilter f)
{
    const SvChannel ch = sv_channel(call, blockIdx.y);
    if (ch.n == 0 || (int)ch.small[SM_K] == 0) return;                 // a zero matrix is not filtered
    const int i = blockIdx.x * SV_FILTER_THREADS + threadIdx.x;
    if (i >= ch.n) return;
    double* row = ch.E + (size_t)i * ch.m;
    sv_filter_row<double, double>(row, row, row, ch.m, f);
}

template <typename Tin, typename Tout>
__global__ __launch_bounds__(SV_FILTER_THREADS) void sv_filter_rows_kernel(const Tin* __restrict__ x, size_t rows,
                                                                           int m, const SvFilter f, double* scratch,
                                                                           Tout* out)
{
    const size_t r = (size_t)blockIdx.x * SV_FILTER_THREADS + threadIdx.x;
    if (r >= rows) return;
    Tout* o = out + r * (size_t)m;
    double* y = scratch ? scratch + r * (size_t)m : (double*)o;        // (no scratch: Tout is double)
    sv_filter_row<Tin, Tout>(x + r * (size_t)m, y, o, m, f);
}

__global__ __launch_bounds__(SV_THREADS) void sv_stack_kernel(const SvCall call, float* __restrict__ filtered,
                                                              float* __restrict__ stack,
                                                              int32_t* __restrict__ n_singular,
                                                              int32_t* __restrict__ status)
{
    const SvChannel ch = sv_channel(call, blockIdx.x);
    __shared__ double red[SV_THREADS];
    const int tid = threadIdx.x, n = ch.n, m = ch.m;
    float* __restrict__ st = stack + (size_t)ch.job * m;
    const int k = n ? (int)ch.small[SM_K] : 0;
    if (tid == 0) {
        n_singular[ch.job] = k;
        status[ch.job] = n ? (int)ch.small[SM_STATUS] : 0;
    }
    if (k == 0) {
        for (int t = tid; t < m; t += SV_THREADS) {
            st[t] = 0.0f;
            if (filtered)
                for (int i = 0; i < n; ++i) filtered[(size_t)(ch.A - call.x) + (size_t)i * ch.ld + t] = 0.0f;
        }
        return;
    }
    float* __restrict__ fo = filtered ? filtered + (size_t)(ch.A - call.x) : nullptr;
    double best = -INFINITY;
    for (int t = tid; t < m; t += SV_THREADS) {
        double sum = 0.0;
        for (int i = 0; i < n; ++i) {
            const float v = (float)ch.E[(size_t)i * m + t];
            if (fo) fo[(size_t)i * ch.ld + t] = v;
            sum += (double)v;
        }
        const double mean = sum / (double)n;
        ch.col[t] = mean;
        best = mean > best ? mean : best;
    }
    red[tid] = best;
    __syncthreads();
    for (int o = SV_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] = red[tid + o] > red[tid] ? red[tid + o] : red[tid];
        __syncthreads();
    }
    const double norm = red[0] == 0.0 ? 1.0 : red[0];
    for (int t = tid; t < m; t += SV_THREADS) st[t] = (float)(ch.col[t] / norm);
}

static bool sv_filter_arguments(const char* what, const double* d_sos, size_t n_sections, double taper_alpha,
                                int detrend, int zerophase, SvFilter* f)
{
    if (!d_sos || n_sections == 0 || n_sections > (size_t)SV_MAX_SECTIONS || taper_alpha != taper_alpha) {
        set_error("%s: need a table of 1 .. %d sections and a taper_alpha that is a number (n_sections=%zu)", what,
                  SV_MAX_SECTIONS, n_sections);
        return false;
    }
    f->sos = d_sos;
    f->n_sections = (int)n_sections;
    f->detrend = detrend != 0;
    f->taper = taper_alpha > 0.0;                                      // tukey(m, alpha <= 0) is all ones
    f->alpha = taper_alpha > 1.0 ? 1.0 : taper_alpha;
    f->zerophase = zerophase != 0;
    return true;
}

}  // namespace bpmf

using namespace bpmf;

extern "C" size_t bpmf_svdwf_workspace_bytes(size_t n_groups, size_t max_group_size, size_t n_samples,
                                             size_t n_channels)
{
    const size_t small = max_group_size < n_samples ? max_group_size : n_samples;
    const size_t large = max_group_size < n_samples ? n_samples : max_group_size;
    if (n_samples == 0 || small > (size_t)SV_MAX_SMALL || large > (size_t)SV_MAX_LARGE || n_groups >= (1ull << 31))
        return 0;
    const size_t slot = sv_sizes(max_group_size, n_samples).slot;
    return sv_carve(nullptr, n_groups, max_group_size ? n_channels : 0, slot).bytes;
}

extern "C" int bpmf_svdwf_stack_dev(const float* d_x, const int64_t* offsets, size_t n_groups, size_t S, size_t C,
                                    size_t n_samples, double expl_var, int max_singular_values, size_t wiener_colsize,
                                    const double* d_sos_or_null, size_t n_sections, double taper_alpha,
                                    void* d_workspace, size_t workspace_bytes, bpmf_stream_t stream_,
                                    float* d_filtered_or_null, float* d_stack, int32_t* d_n_singular,
                                    int32_t* d_status)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n_groups == 0) return 0;
    if (!offsets || !d_stack || !d_n_singular || !d_status || !d_workspace) {
        set_error("bpmf_svdwf_stack_dev: null pointer");
        return -1;
    }
    const size_t SC = S * C, m = n_samples;
    if (S == 0 || C == 0 || m == 0 || SC > 0x7fffffffull || n_groups > 0x7fffffffull / SC) {
        set_error("bpmf_svdwf_stack_dev: bad argument (groups=%zu S=%zu C=%zu n_samples=%zu): need samples, channels "
                  "and fewer than 2^31 channels in all", n_groups, S, C, m);
        return -1;
    }
    if (!(expl_var > 0.0 && expl_var <= 1.0) || max_singular_values < 1 || max_singular_values > SV_MAX_RANK ||
        wiener_colsize > (size_t)SV_MAX_WINDOW) {
        set_error("bpmf_svdwf_stack_dev: need expl_var in (0, 1], max_singular_values 1 .. %d and wiener_colsize <= %d "
                  "(expl_var=%g max_singular_values=%d wiener_colsize=%zu)", SV_MAX_RANK, SV_MAX_WINDOW, expl_var,
                  max_singular_values, wiener_colsize);
        return -1;
    }
    SvFilter filter{};
    if (d_sos_or_null &&
        !sv_filter_arguments("bpmf_svdwf_stack_dev", d_sos_or_null, n_sections, taper_alpha, 1, 1, &filter))
        return -1;
    if (offsets[0] != 0) {
        set_error("bpmf_svdwf_stack_dev: offsets[0] = %lld; the offsets start at 0", (long long)offsets[0]);
        return -1;
    }
    size_t n_max = 0;
    for (size_t g = 0; g < n_groups; ++g) {
        if (offsets[g + 1] < offsets[g]) {
            set_error("bpmf_svdwf_stack_dev: offsets[%zu] = %lld < offsets[%zu] = %lld; they must ascend", g + 1,
                      (long long)offsets[g + 1], g, (long long)offsets[g]);
            return -1;
        }
        const size_t n = (size_t)(offsets[g + 1] - offsets[g]);
        if ((n < m ? n : m) > (size_t)SV_MAX_SMALL || (n < m ? m : n) > (size_t)SV_MAX_LARGE) {
            set_error("bpmf_svdwf_stack_dev: group %zu holds %zu events of %zu samples; min(n, m) <= %d and "
                      "max(n, m) <= %d are served", g, n, m, SV_MAX_SMALL, SV_MAX_LARGE);
            return -1;
        }
        n_max = n > n_max ? n : n_max;
    }
    const size_t N = (size_t)offsets[n_groups];
    if (N > 0x7fffffffull / SC) {
        set_error("bpmf_svdwf_stack_dev: %zu events x %zu channels; fewer than 2^31 rows fit", N, SC);
        return -1;
    }
    if (N && !d_x) {
        set_error("bpmf_svdwf_stack_dev: null pointer");
        return -1;
    }
    const size_t n_jobs = n_groups * SC;
    const SvSizes z = sv_sizes(n_max ? n_max : 1, m);
    const size_t slot_bytes = z.slot * sizeof(double);
    const SvWorkspace ws = sv_carve(d_workspace, n_groups, n_max ? 1 : 0, z.slot);   // (empty groups only: no slot)
    if (workspace_bytes < ws.bytes) {
        set_error("bpmf_svdwf_stack_dev: the workspace holds %zu bytes; one channel of %zu events x %zu samples takes "
                  "%zu (bpmf_svdwf_workspace_bytes)", workspace_bytes, n_max, m, ws.bytes);
        return -1;
    }
    // option debug.poison_output (tests): an element the kernels skip comes back as NaN / -1 (behind the last
    // refusal: a refused call writes nothing)
    if (option(OPT_DEBUG_POISON_OUTPUT) != 0) {
        BPMF_HIP_CHECK(hipMemsetAsync(d_stack, 0xFF, n_jobs * m * sizeof(float), stream));
        BPMF_HIP_CHECK(hipMemsetAsync(d_n_singular, 0xFF, n_jobs * sizeof(int32_t), stream));
        BPMF_HIP_CHECK(hipMemsetAsync(d_status, 0xFF, n_jobs * sizeof(int32_t), stream));
        if (d_filtered_or_null && N)
            BPMF_HIP_CHECK(hipMemsetAsync(d_filtered_or_null, 0xFF, N * SC * m * sizeof(float), stream));
    }
    size_t slab = n_max ? (workspace_bytes - ws.head) / slot_bytes : (size_t)SV_MAX_SLAB;
    slab = slab > (size_t)SV_MAX_SLAB ? (size_t)SV_MAX_SLAB : slab;
    // the offsets go to the head of the workspace; the copy has left the caller's array when the stream has drained
    BPMF_HIP_CHECK(hipMemcpyAsync(ws.offsets, offsets, (n_groups + 1) * sizeof(int64_t), hipMemcpyHostToDevice,
                                  stream));
    BPMF_HIP_CHECK(hipStreamSynchronize(stream));

    SvCall call{};
    call.x = d_x;
    call.offsets = ws.offsets;
    call.slots = ws.slots;
    call.slot = z.slot;
    call.o_v = z.o_v, call.o_a = z.o_a, call.o_b = z.o_b, call.o_sa = z.o_sa, call.o_sq = z.o_sq, call.o_d = z.o_d;
    call.o_e = z.o_e, call.o_col = z.o_col, call.o_small = z.o_small;
    call.SC = (int)SC, call.m = (int)m, call.w = (int)wiener_colsize;
    const int max_sweeps = (int)option(OPT_SVDWF_MAX_SWEEPS);
    const size_t K_max = n_max < m ? n_max : m, Kp_max = K_max + (K_max & 1), tiles = (Kp_max + 15) / 16;
    const size_t elements = n_max * m, long_side = n_max < m ? m : n_max;
    const unsigned element_blocks = (unsigned)((elements + 4 * SV_THREADS - 1) / (4 * SV_THREADS) > 1024
                                                   ? 1024 : (elements + 4 * SV_THREADS - 1) / (4 * SV_THREADS));
    const unsigned side_blocks = (unsigned)((long_side + SV_THREADS - 1) / SV_THREADS > 64
                                                ? 64 : (long_side + SV_THREADS - 1) / SV_THREADS);
    const unsigned column_blocks = (unsigned)((m + SV_THREADS - 1) / SV_THREADS);
    const unsigned row_blocks = (unsigned)((n_max + SV_FILTER_THREADS - 1) / SV_FILTER_THREADS);
    for (size_t job0 = 0; job0 < n_jobs; job0 += slab) {
        const unsigned jobs = (unsigned)(n_jobs - job0 < slab ? n_jobs - job0 : slab);
        call.job0 = (long long)job0;
        if (n_max) {
            sv_gram_kernel<<<dim3((unsigned)(tiles * tiles), jobs), dim3(256), 0, stream>>>(call);
            sv_jacobi_kernel<<<dim3(jobs), dim3(SV_JACOBI_THREADS), 0, stream>>>(call, max_sweeps, expl_var,
                                                                                 max_singular_values);
            sv_project_kernel<<<dim3(side_blocks, jobs), dim3(SV_THREADS), 0, stream>>>(call);
            sv_window_kernel<<<dim3(jobs), dim3(SV_THREADS), 0, stream>>>(call);
            sv_nan_kernel<<<dim3(element_blocks, jobs), dim3(SV_THREADS), 0, stream>>>(call);
            sv_sum_kernel<<<dim3(element_blocks, jobs), dim3(SV_THREADS), 0, stream>>>(call);
            sv_column_kernel<<<dim3(column_blocks, jobs), dim3(SV_THREADS), 0, stream>>>(call);
            sv_second_kernel<<<dim3(column_blocks, jobs), dim3(SV_THREADS), 0, stream>>>(call);
            if (d_sos_or_null)
                sv_filter_kernel<<<dim3(row_blocks, jobs), dim3(SV_FILTER_THREADS), 0, stream>>>(call, filter);
        }
        sv_stack_kernel<<<dim3(jobs), dim3(SV_THREADS), 0, stream>>>(call, d_filtered_or_null, d_stack, d_n_singular,
                                                                     d_status);
        BPMF_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" size_t bpmf_bandpass_rows_workspace_bytes(size_t rows, size_t n_samples, int zerophase, int out_f64)
{
    if (n_samples > SV_MAX_ROW_LENGTH || rows > 0x7fffffffull) return 0;              // (sizes the call refuses)
    return zerophase && !out_f64 ? rows * n_samples * sizeof(double) : 0;
}

extern "C" int bpmf_bandpass_rows_dev(const void* d_x, int in_f64, size_t rows, size_t n_samples, const double* d_sos,
                                      size_t n_sections, int detrend, double taper_alpha, int zerophase, int out_f64,
                                      void* d_workspace, size_t workspace_bytes, bpmf_stream_t stream_, void* d_out)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (rows == 0) return 0;
    if (!d_x || !d_out) {
        set_error("bpmf_bandpass_rows_dev: null pointer");
        return -1;
    }
    if (n_samples == 0 || n_samples > SV_MAX_ROW_LENGTH || rows > 0x7fffffffull) {
        set_error("bpmf_bandpass_rows_dev: need 1 .. 2^24 samples per row and fewer than 2^31 rows (rows=%zu "
                  "n_samples=%zu)", rows, n_samples);
        return -1;
    }
    SvFilter f{};
    if (!sv_filter_arguments("bpmf_bandpass_rows_dev", d_sos, n_sections, taper_alpha, detrend, zerophase, &f))
        return -1;
    const size_t need = bpmf_bandpass_rows_workspace_bytes(rows, n_samples, zerophase, out_f64);
    if (need && (!d_workspace || workspace_bytes < need)) {
        set_error("bpmf_bandpass_rows_dev: a zero-phase call with float32 output needs a workspace of %zu bytes (%zu "
                  "given)", need, d_workspace ? workspace_bytes : (size_t)0);
        return -1;
    }
    if (option(OPT_DEBUG_POISON_OUTPUT) != 0)
        BPMF_HIP_CHECK(hipMemsetAsync(d_out, 0xFF, rows * n_samples * (out_f64 ? sizeof(double) : sizeof(float)),
                                      stream));
    const dim3 grid((unsigned)((rows + SV_FILTER_THREADS - 1) / SV_FILTER_THREADS)), block(SV_FILTER_THREADS);
    double* scratch = need ? (double*)d_workspace : nullptr;
    const int m = (int)n_samples;
    if (in_f64 && out_f64)
        sv_filter_rows_kernel<double, double><<<grid, block, 0, stream>>>((const double*)d_x, rows, m, f, scratch,
                                                                          (double*)d_out);
    else if (in_f64)
        sv_filter_rows_kernel<double, float><<<grid, block, 0, stream>>>((const double*)d_x, rows, m, f, scratch,
                                                                         (float*)d_out);
    else if (out_f64)
        sv_filter_rows_kernel<float, double><<<grid, block, 0, stream>>>((const float*)d_x, rows, m, f, scratch,
                                                                         (double*)d_out);
    else
        sv_filter_rows_kernel<float, float><<<grid, block, 0, stream>>>((const float*)d_x, rows, m, f, scratch,
                                                                        (float*)d_out);
    BPMF_LAUNCH_CHECK();
    return 0;
}
