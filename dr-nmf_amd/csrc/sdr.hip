// SDR on the device from the samples to the dB (include/drnmf_sdr.h): the BSS Eval projection of score.hip for a
// RAGGED batch, with the flen x flen Toeplitz normal equations solved on the GPU.  Four stages, enqueued back
// to back on the caller's stream:
//     r[a] = sum_n ref[n] ref[n-a],  d[a] = sum_n est[n] ref[n-a]             sdr_corr_* + sdr_corr_reduce
//     Toeplitz(r) c = d                                                       toeplitz_solve_kernel (Levinson)
//     s[n] = sum_a c[a] ref[n-a];  sum s^2, sum (est - s)^2                   sdr_project_*
//     SDR = 10 log10(sum s^2 / sum (est - s)^2)                               sdr_final_kernel
// fp64 throughout (score.hip's header: the normal equations of a speech signal are badly conditioned).  Every row
// runs over its own length, read from a device array; time splits, block partials and every summation order are
// functions of that length alone, so a row's numbers are bitwise the same in any batch, stride, position and run.
//
// The correlation and the projection are the same small Toeplitz product: out = sum over (sample, lag) of
// x[sample] * ref[sample - lag].  The tiled kernels give a lane an 8 x 8 register tile of it (8 lags x 8 samples
// in the correlation, 8 outputs x 8 lags in the projection), which touches only 15 distinct delayed samples.
// Those come from a window of ref staged in LDS as fp64 and stored TRANSPOSED, win[(p & 7) * K + (p >> 3)]:
// neighbouring lanes' tiles are 8 samples apart, so for a given register they read consecutive doubles of one
// row (no bank conflict), and the window slides by 8 between chunks, so only 8 of the 15 are loaded per 128
// (correlation) or 64 (projection) FMAs.
#include "common.h"
#include "../../include/drnmf_sdr.h"

namespace {

constexpr int MAX_FLEN = 2048;
constexpr int SOLVE_MAX_N = 2048;
constexpr int CORR_SPAN = 8192;        // samples of a row one correlation workgroup sums: splits = ceil(len / SPAN)
constexpr int CORR_TILE = 1024;        // samples staged in LDS at a time (4 waves x 256)
constexpr int CORR_LAGS = 512;         // lags of one workgroup (64 lanes x 8), the same for its 4 waves
constexpr int CORR_K = CORR_TILE / 8 + CORR_LAGS / 8;     // columns of the transposed window
constexpr int PROJ_OUT = 2048;         // output samples of one projection workgroup (256 lanes x 8)

__device__ __forceinline__ int64_t row_len(const int64_t* __restrict__ lengths, int sig, int64_t stride) {
    if (!lengths) return stride;
    const int64_t len = lengths[sig];
    return len < 0 ? 0 : (len > stride ? stride : len);
}

__host__ __device__ inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Sum over the 64 lanes by a fixed butterfly; every lane gets the same bits (each step adds the same pair,
// only commuted).
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- Levinson-Durbin, one wave per system ------------------------------------------------------------------
// Order k -> k + 1 (Golub & Van Loan, Alg. 4.7.2, not normalised): with y the order-k predictor
// (T_k y = -r[1..k]), x the order-k solution and E the prediction error,
//     mu    = (d[k]   - sum_{i<k} r[k-i] x[i]) / E        x <- [x + mu rev(y), mu]
//     alpha = -(r[k+1] + sum_{i<k} r[k-i] y[i]) / E       y <- [y + alpha rev(y), alpha],  E <- E (1 - alpha^2)
// A lane owns the pairs (i, k-1-i), i = lane, lane + 64, ..., so both in-place updates are race free, and it
// accumulates the NEXT step's two dot products from the values it has just written: one pass over LDS and one
// wave reduction per step.  r | d | y | x live in dynamic LDS (4 n doubles: 16 KB at n = 512, 64 KB at 2048).
__global__ void __launch_bounds__(64)
toeplitz_solve_kernel(const double* __restrict__ r, const double* __restrict__ d, int n,
                      double* __restrict__ c_out, int* __restrict__ info_out) {
    extern __shared__ double sm[];
    double* R = sm;
    double* D = sm + n;
    double* Y = sm + 2 * (size_t)n;
    double* X = sm + 3 * (size_t)n;
    const int lane = threadIdx.x;
    const size_t o = (size_t)blockIdx.x * n;
    for (int i = lane; i < n; i += 64) {
        R[i] = r[o + i];
        D[i] = d[o + i];
        Y[i] = 0.0;
        X[i] = 0.0;
    }
    __syncthreads();
    const double r0 = R[0];
    int info = 0;
    if (!(r0 > 0.0) || !(r0 <= 1.7976931348623157e308)) {       // silent (or non-finite) reference: c = 0
        info = 1;
    } else {
        double E = r0;
        const double x0 = D[0] / r0;
        double alpha = 0.0, s1 = 0.0, s2 = 0.0;
        if (n > 1) {
            alpha = -R[1] / r0;
            s1 = R[1] * x0;
            s2 = R[1] * alpha;
        }
        if (lane == 0) {
            X[0] = x0;
            if (n > 1) Y[0] = alpha;
        }
        __syncthreads();
        for (int k = 1; k < n; ++k) {
            E = E * (1.0 - alpha * alpha);
            if (!(E > 0.0)) {                  // the order-k solution, zero-extended, is what is left in X
                info = 2 + k;
                break;
            }
            const bool more = k < n - 1;
            const double mu = (D[k] - s1) / E;
            const double an = more ? -(R[k + 1] + s2) / E : 0.0;
            double p1 = 0.0, p2 = 0.0;
            const int half = (k + 1) >> 1;
            for (int i = lane; i < half; i += 64) {
                const int j = k - 1 - i;
                const double ya = Y[i], yb = Y[j], xa = X[i], xb = X[j];
                const double xi = fma(mu, yb, xa), yi = fma(an, yb, ya);
                X[i] = xi;
                Y[i] = yi;
                if (more) {
                    const double ri = R[k + 1 - i];
                    p1 = fma(ri, xi, p1);
                    p2 = fma(ri, yi, p2);
                }
                if (j != i) {
                    const double xj = fma(mu, ya, xb), yj = fma(an, ya, yb);
                    X[j] = xj;
                    Y[j] = yj;
                    if (more) {
                        const double rj = R[k + 1 - j];
                        p1 = fma(rj, xj, p1);
                        p2 = fma(rj, yj, p2);
                    }
                }
            }
            if (lane == 0) {
                X[k] = mu;
                Y[k] = an;
                if (more) {
                    p1 = fma(R[1], mu, p1);
                    p2 = fma(R[1], an, p2);
                }
            }
            if (more) {
                s1 = wave_sum(p1);
                s2 = wave_sum(p2);
            }
            alpha = an;
            __syncthreads();
        }
    }
    __syncthreads();
    for (int i = lane; i < n; i += 64) c_out[o + i] = info == 1 ? 0.0 : X[i];
    if (lane == 0) info_out[blockIdx.x] = info;
}

// ---- correlation ---------------------------------------------------------------------------------------------
// part[sig][split][2][flen], split = span of CORR_SPAN samples; grid (lag blocks, max splits, n_sig).

// Lane l of every wave owns the lags A0 + 8 l + j (j < 8); wave w sums the samples [256 w, 256 w + 256)
// of each staged tile in chunks of 8.  Sample n0 + 8 c + i against lag A0 + 8 l + j is window element
// p = 8 (c + 63 - l) + (i - j + 7), window origin n0 - A0 - 511.  The four waves' sums are added in wave order.
__global__ void __launch_bounds__(256)
sdr_corr_tiled_kernel(const float* __restrict__ est, const float* __restrict__ ref, int64_t stride,
                      const int64_t* __restrict__ lengths, int flen, int max_splits,
                      double* __restrict__ part) {
    __shared__ double win[8 * CORR_K];
    __shared__ double sT[CORR_TILE];
    __shared__ double eT[CORR_TILE];
    const int sig = blockIdx.z, sp = blockIdx.y;
    const int A0 = blockIdx.x * CORR_LAGS;
    const int64_t len = row_len(lengths, sig, stride);
    const int64_t span0 = (int64_t)sp * CORR_SPAN;
    if (span0 >= len) return;                                   // (the whole workgroup, before any barrier)
    const int64_t span1 = span0 + CORR_SPAN < len ? span0 + CORR_SPAN : len;
    const float* e = est + (size_t)sig * stride;
    const float* s = ref + (size_t)sig * stride;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double ar[8], ad[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) ar[j] = ad[j] = 0.0;
    for (int64_t n0 = span0; n0 < span1; n0 += CORR_TILE) {
        __syncthreads();
        const int64_t w0 = n0 - A0 - (CORR_LAGS - 1);
        for (int p = tid; p < CORR_TILE + CORR_LAGS - 1; p += 256) {
            const int64_t m = w0 + p;
            win[(p & 7) * CORR_K + (p >> 3)] = (m >= 0 && m < len) ? (double)s[m] : 0.0;
        }
        for (int i = tid; i < CORR_TILE; i += 256) {
            const int64_t m = n0 + i;
            const bool ok = m < len;
            sT[i] = ok ? (double)s[m] : 0.0;
            eT[i] = ok ? (double)e[m] : 0.0;
        }
        __syncthreads();
        const int c0 = wv * 32;
        if (n0 + 8 * c0 < len) {                                // (wave-uniform; no barrier inside)
            double w[15];
            const int col = c0 + 63 - lane;
#pragma unroll
            for (int m = 0; m < 7; ++m) w[m] = win[m * CORR_K + col];
            for (int c = 0; c < 32; ++c) {
                if (n0 + 8 * (c0 + c) >= len) break;            // behind the row's end: zeros
                const int cc = col + c;
                w[7] = win[7 * CORR_K + cc];
#pragma unroll
                for (int m = 0; m < 7; ++m) w[8 + m] = win[m * CORR_K + cc + 1];
                double sv[8], ev[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    sv[i] = sT[8 * (c0 + c) + i];
                    ev[i] = eT[8 * (c0 + c) + i];
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        ar[j] = fma(sv[i], w[i - j + 7], ar[j]);
                        ad[j] = fma(ev[i], w[i - j + 7], ad[j]);
                    }
                }
#pragma unroll
                for (int m = 0; m < 7; ++m) w[m] = w[m + 8];
            }
        }
    }
    // ((wave 0 + wave 1) + wave 2) + wave 3, through the window's LDS
    double* buf = win;
    for (int src = 1; src < 4; ++src) {
        __syncthreads();
        if (wv == src) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                buf[j * 64 + lane] = ar[j];
                buf[512 + j * 64 + lane] = ad[j];
            }
        }
        __syncthreads();
        if (wv == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                ar[j] += buf[j * 64 + lane];
                ad[j] += buf[512 + j * 64 + lane];
            }
        }
    }
    if (wv == 0) {
        double* p = part + (((size_t)sig * max_splits + sp) * 2) * flen;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int a = A0 + 8 * lane + j;
            if (a < flen) {
                p[a] = ar[j];
                p[flen + a] = ad[j];
            }
        }
    }
}

// the row's own splits, in order
__global__ void __launch_bounds__(256)
sdr_corr_reduce_kernel(const double* __restrict__ part, int64_t stride, const int64_t* __restrict__ lengths,
                       int flen, int max_splits, double* __restrict__ r_out, double* __restrict__ d_out) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    const int sig = blockIdx.y;
    if (a >= flen) return;
    const int nsp = (int)ceil_div64(row_len(lengths, sig, stride), CORR_SPAN);
    double r = 0.0, d = 0.0;
    for (int sp = 0; sp < nsp; ++sp) {
        const double* p = part + (((size_t)sig * max_splits + sp) * 2) * flen;
        r += p[a];
        d += p[flen + a];
    }
    r_out[(size_t)sig * flen + a] = r;
    d_out[(size_t)sig * flen + a] = d;
}

// ---- projection ----------------------------------------------------------------------------------------------
// part[sig][block][2] over the padded length L = len + flen - 1 (0 for an empty row); grid (max blocks, n_sig).

__device__ __forceinline__ void block_sum2(double en, double er, double* red, double* __restrict__ out) {
    red[threadIdx.x] = en;
    red[256 + threadIdx.x] = er;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            red[threadIdx.x] += red[threadIdx.x + o];
            red[256 + threadIdx.x] += red[256 + threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = red[0];
        out[1] = red[256];
    }
}

// Thread t owns the outputs N0 + 8 t + i (i < 8) and walks the lags in chunks of 8 (C = ceil(flen / 8)
// chunks, coefficients behind flen are zero).  Output N0 + 8 t + i against lag 8 c + j is window element
// p = 8 (t - c + C - 1) + (i - j + 7), window origin N0 - 8 C + 1; the window slides DOWN by 8 per chunk.
// LDS: win[8][256 + C] | cf[8 C] | red[512] doubles.
__global__ void __launch_bounds__(256)
sdr_project_tiled_kernel(const float* __restrict__ est, const float* __restrict__ ref,
                         const double* __restrict__ coef, int64_t stride,
                         const int64_t* __restrict__ lengths, int flen, int64_t max_blocks,
                         double* __restrict__ part) {
    extern __shared__ double sm[];
    const int C = (flen + 7) >> 3;
    const int K = 256 + C;
    double* win = sm;
    double* cf = sm + 8 * (size_t)K;
    double* red = cf + 8 * (size_t)C;
    const int sig = blockIdx.y;
    const int64_t len = row_len(lengths, sig, stride);
    const int64_t L = len > 0 ? len + flen - 1 : 0;
    const int64_t N0 = (int64_t)blockIdx.x * PROJ_OUT;
    if (N0 >= L) return;                                        // (the whole workgroup)
    const float* e = est + (size_t)sig * stride;
    const float* s = ref + (size_t)sig * stride;
    const int tid = threadIdx.x;
    for (int i = tid; i < 8 * C; i += 256) cf[i] = i < flen ? coef[(size_t)sig * flen + i] : 0.0;
    const int64_t w0 = N0 - 8 * (int64_t)C + 1;
    for (int p = tid; p < 8 * K; p += 256) {
        const int64_t m = w0 + p;
        win[(p & 7) * K + (p >> 3)] = (m >= 0 && m < len) ? (double)s[m] : 0.0;
    }
    __syncthreads();
    double st[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = 0.0;
    double en = 0.0, er = 0.0;
    if (N0 + 8 * tid < L) {
        double w[15];
        const int col = tid + C - 1;
#pragma unroll
        for (int m = 0; m < 7; ++m) w[8 + m] = win[m * K + col + 1];
        for (int c = 0; c < C; ++c) {
            const int cc = col - c;
#pragma unroll
            for (int m = 0; m < 8; ++m) w[m] = win[m * K + cc];
            double cv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) cv[j] = cf[8 * c + j];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
#pragma unroll
                for (int i = 0; i < 8; ++i) st[i] = fma(cv[j], w[i - j + 7], st[i]);
            }
#pragma unroll
            for (int m = 0; m < 7; ++m) w[8 + m] = w[m];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int64_t n = N0 + 8 * tid + i;
            if (n < L) {
                const double ev = n < len ? (double)e[n] : 0.0;
                en = fma(st[i], st[i], en);
                er = fma(ev - st[i], ev - st[i], er);
            }
        }
    }
    block_sum2(en, er, red, part + ((size_t)sig * max_blocks + blockIdx.x) * 2);
}

__global__ void __launch_bounds__(256)
sdr_final_kernel(const double* __restrict__ part, int64_t stride, const int64_t* __restrict__ lengths,
                 int flen, int per_block, int64_t max_blocks, double* __restrict__ energies,
                 float* __restrict__ out_db) {
    __shared__ double s0[256], s1[256];
    const int sig = blockIdx.x;
    const int64_t len = row_len(lengths, sig, stride);
    const int64_t nblocks = len > 0 ? ceil_div64(len + flen - 1, per_block) : 0;
    double a = 0.0, b = 0.0;
    for (int64_t i = threadIdx.x; i < nblocks; i += 256) {
        a += part[((size_t)sig * max_blocks + i) * 2 + 0];
        b += part[((size_t)sig * max_blocks + i) * 2 + 1];
    }
    s0[threadIdx.x] = a;
    s1[threadIdx.x] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            s0[threadIdx.x] += s0[threadIdx.x + o];
            s1[threadIdx.x] += s1[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (energies) {
            energies[2 * sig + 0] = s0[0];
            energies[2 * sig + 1] = s1[0];
        }
        out_db[sig] = (float)(10.0 * log10(s0[0] / s1[0]));
    }
}

struct Layout {
    int64_t max_splits, max_blocks;
    size_t off_part, off_r, off_d, off_coef, off_en, off_info, total;
};
Layout layout(int n_sig, int64_t stride, int flen) {
    Layout L;
    L.max_splits = ceil_div64(stride, CORR_SPAN);
    L.max_blocks = ceil_div64(stride + flen - 1, PROJ_OUT);
    const size_t corr = (size_t)n_sig * L.max_splits * 2 * flen * 8;
    const size_t proj = (size_t)n_sig * L.max_blocks * 2 * 8;
    size_t o = 0;
    L.off_part = o;  o += round_up_sz(corr > proj ? corr : proj, 256);      // (the projection reuses it)
    L.off_r = o;     o += round_up_sz((size_t)n_sig * flen * 8, 256);
    L.off_d = o;     o += round_up_sz((size_t)n_sig * flen * 8, 256);
    L.off_coef = o;  o += round_up_sz((size_t)n_sig * flen * 8, 256);
    L.off_en = o;    o += round_up_sz((size_t)n_sig * 2 * 8, 256);
    L.off_info = o;  o += round_up_sz((size_t)n_sig * 4, 256);
    L.total = o;
    return L;
}

void launch_solve(int n_sys, int n, const double* r, const double* d, double* c, int* info, hipStream_t stream) {
    hipLaunchKernelGGL(toeplitz_solve_kernel, dim3((unsigned)n_sys), dim3(64), (size_t)n * 4 * 8, stream, r, d, n,
                       c, info);
}

}  // namespace

extern "C" int32_t drnmf_toeplitz_solve(drnmf_handle_t h, int32_t n_sys, int32_t n, const double* r,
                                        const double* d, double* c_out, int32_t* info_out, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (n_sys <= 0 || n <= 0 || n > SOLVE_MAX_N)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "toeplitz_solve: n_sys >= 1 and 1 <= n <= 2048 (got %d, %d)", n_sys, n);
    if (!r || !d || !c_out || !info_out)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "toeplitz_solve: NULL r, d, c_out or info_out");
    launch_solve(n_sys, n, r, d, c_out, info_out, (hipStream_t)stream_);
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}

extern "C" size_t drnmf_sdr_ragged_workspace_bytes(int32_t n_sig, int64_t stride, int32_t flen) {
    if (n_sig <= 0 || stride <= 0 || flen <= 0 || flen > MAX_FLEN) return 0;
    return layout(n_sig, stride, flen).total;
}

extern "C" int32_t drnmf_sdr_ragged(drnmf_handle_t h, int32_t n_sig, int64_t stride, const int64_t* lengths,
                                    int32_t flen, const float* est, const float* ref, float* sdr_out,
                                    double* coef_out, double* energies_out, double* r_out, double* d_out,
                                    int32_t* info_out, void* workspace, size_t workspace_bytes, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (n_sig <= 0 || n_sig > 65535 || stride <= 0 || flen <= 0 || flen > MAX_FLEN)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG,
                   "sdr_ragged: 1 <= n_sig <= 65535, stride >= 1, 1 <= flen <= 2048 (got %d, %lld, %d)", n_sig,
                   (long long)stride, flen);
    if (!est || !ref || !sdr_out || !workspace)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "sdr_ragged: NULL est, ref, sdr_out or workspace");
    const Layout L = layout(n_sig, stride, flen);
    if (L.max_splits > 65535)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "sdr_ragged: stride %lld is beyond 65535 spans of %d samples",
                   (long long)stride, CORR_SPAN);
    if (workspace_bytes < L.total) DRNMF_FAIL(h, DRNMF_ERR_WORKSPACE, "sdr_ragged: workspace too small");
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    double* part = (double*)(ws + L.off_part);
    double* r = r_out ? r_out : (double*)(ws + L.off_r);
    double* d = d_out ? d_out : (double*)(ws + L.off_d);
    double* coef = coef_out ? coef_out : (double*)(ws + L.off_coef);
    int* info = info_out ? info_out : (int*)(ws + L.off_info);
    const int ms = (int)L.max_splits;
    hipLaunchKernelGGL(sdr_corr_tiled_kernel,
                       dim3((unsigned)((flen + CORR_LAGS - 1) / CORR_LAGS), (unsigned)ms, (unsigned)n_sig), dim3(256), 0,
                       stream, est, ref, stride, lengths, flen, ms, part);
    hipLaunchKernelGGL(sdr_corr_reduce_kernel, dim3((unsigned)((flen + 255) / 256), (unsigned)n_sig), dim3(256), 0,
                       stream, part, stride, lengths, flen, ms, r, d);
    launch_solve(n_sig, flen, r, d, coef, info, stream);
    const int C = (flen + 7) / 8;
    const size_t shmem = ((size_t)8 * (256 + C) + 8 * C + 512) * 8;
    hipLaunchKernelGGL(sdr_project_tiled_kernel, dim3((unsigned)L.max_blocks, (unsigned)n_sig), dim3(256), shmem,
                       stream, est, ref, coef, stride, lengths, flen, L.max_blocks, part);
    hipLaunchKernelGGL(sdr_final_kernel, dim3((unsigned)n_sig), dim3(256), 0, stream, part, stride, lengths, flen,
                       PROJ_OUT, L.max_blocks, energies_out, sdr_out);
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}
