// Waveform criteria on gfx950 (include/drnmf_waveloss.h): per-row MSE or SI-SDR between a reconstruction and
// its reference, with the gradient with respect to the reconstruction.
//
// Three launches.  (1) wave_loss_partial_kernel: one workgroup per DRNMF_WAVE_LOSS_BLOCK samples of a row sums
// <est, ref>, |ref|^2, |est|^2, |est - ref|^2 in fp64 -- 16 consecutive terms per lane, the lanes of a wave by a
// fixed butterfly, the four waves in order (as mix.hip sums its energies).  (2) wave_loss_rows_kernel: one lane per
// row adds the row's partials in ascending order, evaluates the loss and the two coefficients of
// g = ca est + cb ref, and workgroup 0 sums the counted rows in a fixed order.  (3) wave_loss_grad_kernel writes
// g, each element evaluated in fp64 and rounded once: at a high SI-SDR the two terms cancel (for a row of one
// sample exactly, down to the eps terms), which fp32 products would turn into noise far above the gradient.
// A row's loss and gradient depend on that row alone: bitwise the same in any batch.
//
// SI-SDR with t = p^2/q (target energy), r = e - t (residual), c = 10 / ln 10, eps = 1e-8:
//   loss = -c (ln(t + eps) - ln(r + eps)),   d loss / d est = 2 c est / (r + eps) - (2 p / q) c (1 / (t + eps) + 1 / (r + eps)) ref.
// MSE: d loss / d est = (2 / n) (est - ref).
#include "common.h"
#include "../../include/drnmf_waveloss.h"

namespace {

constexpr int WL_BLOCK = DRNMF_WAVE_LOSS_BLOCK, WL_PER_LANE = WL_BLOCK / 256;
static_assert(WL_PER_LANE * 256 == WL_BLOCK, "a workgroup covers a block with whole lanes");

__host__ __device__ inline int64_t wl_blocks(int64_t n) { return (n + WL_BLOCK - 1) / WL_BLOCK; }

__device__ __forceinline__ int64_t wl_len(const int64_t* __restrict__ lengths, int row, int64_t ld) {
    const int64_t n = lengths[row];
    return n < 0 ? 0 : (n > ld ? ld : n);
}

// partial [n_sig][nblk][4] (nblk = wl_blocks(ld)): blocks at or behind a row's length are not written, nor read
__global__ void __launch_bounds__(256)
wave_loss_partial_kernel(const float* __restrict__ est, const float* __restrict__ ref,
                         const int64_t* __restrict__ lengths, int64_t ld, int64_t nblk,
                         double* __restrict__ partial) {
    __shared__ double red[4][4];
    const int tid = threadIdx.x, wv = tid >> 6, l = tid & 63;
    const int row = (int)(blockIdx.x / nblk);
    const int64_t blk = (int64_t)(blockIdx.x % nblk);
    const int64_t n = wl_len(lengths, row, ld);
    if (blk * WL_BLOCK >= n) return;          // (the whole workgroup)
    const float* e = est + (size_t)row * ld;
    const float* s = ref + (size_t)row * ld;
    const int64_t i0 = blk * WL_BLOCK + (int64_t)tid * WL_PER_LANE;
    double p = 0.0, q = 0.0, ee = 0.0, dd = 0.0;
#pragma unroll
    for (int u = 0; u < WL_PER_LANE; ++u) {
        const int64_t i = i0 + u;
        if (i < n) {
            const double a = (double)e[i], b = (double)s[i];
            p += a * b;
            q += b * b;
            ee += a * a;
            dd += (a - b) * (a - b);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        p += __shfl_xor(p, o, 64);
        q += __shfl_xor(q, o, 64);
        ee += __shfl_xor(ee, o, 64);
        dd += __shfl_xor(dd, o, 64);
    }
    if (l == 0) { red[wv][0] = p; red[wv][1] = q; red[wv][2] = ee; red[wv][3] = dd; }
    __syncthreads();
    if (tid < 4)
        partial[((size_t)row * nblk + blk) * 4 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// one lane per row; coef [n_sig][2] = (ca, cb); ONE workgroup, which also leaves sums[2]
__global__ void __launch_bounds__(256)
wave_loss_rows_kernel(const double* __restrict__ partial, const int64_t* __restrict__ lengths, int64_t ld,
                      int64_t nblk, int n_sig, int kind, float* __restrict__ loss, float* __restrict__ counted,
                      double* __restrict__ coef, float* __restrict__ sums) {
    __shared__ double s0[256], s1[256];
    double tot = 0.0, cnt = 0.0;
    for (int row = threadIdx.x; row < n_sig; row += 256) {
        const int64_t n = wl_len(lengths, row, ld);
        const int64_t nb = wl_blocks(n);
        double p = 0.0, q = 0.0, e = 0.0, dd = 0.0;
        for (int64_t b = 0; b < nb; ++b) {
            const double* pp = partial + ((size_t)row * nblk + b) * 4;
            p += pp[0];
            q += pp[1];
            e += pp[2];
            dd += pp[3];
        }
        double l = 0.0, ca = 0.0, cb = 0.0;
        bool on = false;
        if (kind == DRNMF_WAVE_LOSS_MSE) {
            if (n >= 1) {
                on = true;
                l = dd / (double)n;
                ca = 2.0 / (double)n;
                cb = -ca;
            }
        } else if (n >= 1 && q > 0.0) {
            on = true;
            const double eps = 1e-8, c = 10.0 / log(10.0);
            const double t = p * p / q, r = e - t;
            l = -c * (log(t + eps) - log(r + eps));
            ca = 2.0 * c / (r + eps);
            cb = -(2.0 * p / q) * c * (1.0 / (t + eps) + 1.0 / (r + eps));
        }
        loss[row] = (float)l;
        counted[row] = on ? 1.f : 0.f;
        coef[2 * (size_t)row] = ca;
        coef[2 * (size_t)row + 1] = cb;
        if (on) {
            tot += l;
            cnt += 1.0;
        }
    }
    s0[threadIdx.x] = tot;
    s1[threadIdx.x] = cnt;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            s0[threadIdx.x] += s0[threadIdx.x + o];
            s1[threadIdx.x] += s1[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { sums[0] = (float)s0[0]; sums[1] = (float)s1[0]; }
}

// g = ca est + cb ref for i < n, 0 behind it (every element of the row is written)
__global__ void __launch_bounds__(256)
wave_loss_grad_kernel(const float* __restrict__ est, const float* __restrict__ ref,
                      const int64_t* __restrict__ lengths, int64_t ld, int64_t nblk,
                      const double* __restrict__ coef, float* __restrict__ g) {
    const int row = (int)(blockIdx.x / nblk);
    const int64_t blk = (int64_t)(blockIdx.x % nblk);
    const int64_t n = wl_len(lengths, row, ld);
    const double ca = coef[2 * (size_t)row], cb = coef[2 * (size_t)row + 1];
    const size_t o = (size_t)row * ld;
#pragma unroll
    for (int u = 0; u < WL_PER_LANE; ++u) {
        const int64_t i = blk * WL_BLOCK + (int64_t)u * 256 + threadIdx.x;
        if (i < ld) g[o + i] = i < n ? (float)(ca * (double)est[o + i] + cb * (double)ref[o + i]) : 0.f;
    }
}

struct WlWs {
    size_t off_partial, off_coef, total;
    int64_t nblk;
};
WlWs wl_layout(int n_sig, int64_t ld) {
    WlWs L;
    L.nblk = wl_blocks(ld);
    L.off_partial = 0;
    L.off_coef = round_up_sz((size_t)n_sig * (size_t)L.nblk * 4 * sizeof(double), 256);
    L.total = L.off_coef + round_up_sz((size_t)n_sig * 2 * sizeof(double), 256);
    return L;
}

}  // namespace

extern "C" size_t drnmf_wave_loss_workspace_bytes(int32_t n_sig, int64_t ld) {
    if (n_sig <= 0 || ld <= 0) return 0;
    return wl_layout(n_sig, ld).total;
}

extern "C" int32_t drnmf_wave_loss(drnmf_handle_t h, int32_t n_sig, int64_t ld, const int64_t* lengths,
                                   const float* est, const float* ref, int32_t kind, float* loss, float* counted,
                                   float* g, float* sums, void* workspace, size_t workspace_bytes, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (n_sig <= 0 || ld <= 0 || (int64_t)n_sig * wl_blocks(ld > 0 ? ld : 1) > 0x7fffffff)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "wave_loss: bad shape n_sig=%d ld=%lld (n_sig * ceil(ld / %d) < 2^31)",
                   n_sig, (long long)ld, WL_BLOCK);
    if (kind != DRNMF_WAVE_LOSS_MSE && kind != DRNMF_WAVE_LOSS_SI_SDR)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "wave_loss: kind=%d is neither DRNMF_WAVE_LOSS_MSE nor _SI_SDR", kind);
    if (!lengths || !est || !ref || !loss || !counted || !g || !sums)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "wave_loss: NULL pointer argument");
    const WlWs L = wl_layout(n_sig, ld);
    if (!workspace || workspace_bytes < L.total)
        DRNMF_FAIL(h, DRNMF_ERR_WORKSPACE, "wave_loss: workspace too small (%zu < %zu bytes)",
                   workspace ? workspace_bytes : (size_t)0, L.total);
    if ((uintptr_t)workspace & 7) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "wave_loss: workspace must be 8-byte aligned");
    if (h->device < 0) DRNMF_FAIL(h, DRNMF_ERR_HIP, "wave_loss: the handle is bound to no device");
    hipStream_t stream = (hipStream_t)stream_;
    double* partial = (double*)((char*)workspace + L.off_partial);
    double* coef = (double*)((char*)workspace + L.off_coef);
    const dim3 grid((unsigned)((int64_t)n_sig * L.nblk));
    hipLaunchKernelGGL(wave_loss_partial_kernel, grid, dim3(256), 0, stream, est, ref, lengths, ld, L.nblk, partial);
    hipLaunchKernelGGL(wave_loss_rows_kernel, dim3(1), dim3(256), 0, stream, (const double*)partial, lengths, ld,
                       L.nblk, n_sig, kind, loss, counted, coef, sums);
    hipLaunchKernelGGL(wave_loss_grad_kernel, grid, dim3(256), 0, stream, est, ref, lengths, ld, L.nblk,
                       (const double*)coef, g);
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}
