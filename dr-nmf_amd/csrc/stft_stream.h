// Streaming STFT / masked iSTFT (include/drnmf_stream.h).  Included by stft.hip behind the frame bodies, which
// these kernels call unchanged: a frame's samples are gathered from the carry and the chunk into LDS in the
// chunk's own type and handed to stft_real_frame / stft_frame as a signal of N samples whose frame N / hop starts
// at sample 0, so the body runs the instructions it runs for drnmf_stft_ragged on the same values.
//
// Forward: one wave (N = 512 / 1024) or one workgroup per new frame, reading the state only; a second launch
// (one workgroup per stream) then moves the carry and the counters on.  Inverse: one workgroup per stream, the
// new frames in ascending order, four at a time (N = 512 / 1024) or one (other sizes); the partial sums of the
// samples the coming frames still reach sit in LDS and go back to the state at the end.
#pragma once

namespace {

struct StreamHdr {                // 64 bytes in front of every stream's state
    int64_t n_in;                 // samples consumed
    int64_t frames;               // frames emitted
    int64_t push_f0;              // first frame of the latest push
    int32_t push_new;             // its frame count (clamped to that push's T)
    int32_t closed;
    int64_t pad_[4];
};
static_assert(sizeof(StreamHdr) == 64, "drnmf_stream.h documents a 64-byte header");

static size_t stream_state_stride(int N, int hop) {
    return round_up_sz(sizeof(StreamHdr) + sizeof(float) * ((size_t)3 * N - hop), 64);
}

struct StreamState {
    StreamHdr* hdr;
    int32_t* in_carry;            // [N] words: sample frames * hop - N + i of the stream (float bits, or an int16 value)
    float* ola;                   // [N - hop] partial sums of samples frames * hop - N + i
    float* frame;                 // [N] scratch of the inverse at the sizes without the fused frame body
};

__device__ __forceinline__ StreamState stream_state(void* state, size_t per, int b, int N, int hop) {
    char* p = (char*)state + per * (size_t)b;
    StreamState s;
    s.hdr = (StreamHdr*)p;
    s.in_carry = (int32_t*)(p + sizeof(StreamHdr));
    s.ola = (float*)(s.in_carry + N);
    s.frame = s.ola + (N - hop);
    return s;
}

struct StreamPush {               // what a push does to one stream (uniform over the workgroup)
    int64_t n0, n1;               // samples before / after
    int64_t f0, f1;               // frames before / after
    int nnew;                     // min(f1 - f0, T)
    int closed;                   // after the push
};

__device__ __forceinline__ StreamPush stream_push(const StreamHdr* h, int64_t len, int fin, int64_t stride, int T,
                                                  int N, int hop) {
    StreamPush p;
    p.n0 = h->n_in;
    p.f0 = h->frames;
    const int closed0 = h->closed != 0;
    len = len < 0 ? 0 : (len > stride ? stride : len);
    if (closed0) len = 0;
    p.n1 = p.n0 + len;
    p.closed = closed0 || fin != 0;
    // written out in its own form (hop divides N), not stft_frame_count: the kernels' instructions stay as they were
    p.f1 = p.closed ? (p.n1 + hop - 1) / hop + N / hop + 1      // as drnmf_stft_frames
                    : p.n1 / hop + 1;
    if (p.f1 < p.f0) p.f1 = p.f0;
    const int64_t d = p.f1 - p.f0;
    p.nnew = (int)(d < T ? d : T);
    return p;
}

// sample g of the stream as a 32-bit word (float bits, or the int16 value): zero in front of the stream and
// behind its end, the chunk from n0 on, the carry before
__device__ __forceinline__ int32_t stream_word(const void* __restrict__ chunk, int is_int16, size_t row0,
                                               const int32_t* __restrict__ carry, const StreamPush& p, int64_t g,
                                               int N, int hop) {
    if (g < 0 || g >= p.n1) return 0;
    if (g >= p.n0)
        return is_int16 ? (int32_t)((const short*)chunk)[row0 + (size_t)(g - p.n0)]
                        : ((const int32_t*)chunk)[row0 + (size_t)(g - p.n0)];
    const int64_t ci = g - (p.f0 * hop - N);
    return ci >= 0 && ci < N ? carry[ci] : 0;
}

__global__ void __launch_bounds__(256) stream_reset_kernel(uint32_t* __restrict__ state, size_t n_words) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_words) state[i] = 0u;
}

template <int R, int P>
__global__ void __launch_bounds__(256)
stream_fwd_real_kernel(const void* __restrict__ chunk, int is_int16, int64_t stride,
                       const int64_t* __restrict__ chunk_len, const int32_t* __restrict__ fin, int T, int logN,
                       int hop, float mask_value, float* __restrict__ x, float* __restrict__ re,
                       float* __restrict__ im, void* __restrict__ state, size_t per) {
    constexpr int N = RealFft<R, P>::N, F = N / 2 + 1;
    __shared__ float2 tw[N / 2];
    __shared__ float2 bufs[4][RealFft<R, P>::MP];
    __shared__ __attribute__((aligned(16))) int32_t stage[4][N];
    const int tid = threadIdx.x, wv = tid >> 6, j = tid & 63;
    const int t = blockIdx.x * 4 + wv, b = blockIdx.y;
    for (int i = tid; i < N / 2; i += 256) tw[i] = g_twiddle[logN - TAB_LOG_MIN][i];
    __syncthreads();
    if (t >= T) return;                       // (whole waves: no barrier below)
    const StreamState st = stream_state(state, per, b, N, hop);
    const StreamPush p = stream_push(st.hdr, chunk_len[b], fin[b], stride, T, N, hop);
    const size_t o = ((size_t)b * T + t) * F;
    if (t >= p.nnew) {                        // padding frame: Masking's value in every bin
        for (int i = j; i < F; i += 64) x[o + i] = mask_value;
        return;
    }
    const int64_t g0 = (p.f0 + t) * hop - N;  // first sample of the frame
    for (int i = j; i < N; i += 64) {
        const int32_t w = stream_word(chunk, is_int16, (size_t)b * stride, st.in_carry, p, g0 + i, N, hop);
        if (is_int16) ((short*)stage[wv])[i] = (short)w;
        else stage[wv][i] = w;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    stft_real_frame<R, P>((const void*)stage[wv], is_int16, 0, N, logN, hop, N / hop, o, x, re, im, tw, bufs[wv],
                          j);
}

__global__ void __launch_bounds__(256)
stream_fwd_kernel(const void* __restrict__ chunk, int is_int16, int64_t stride,
                  const int64_t* __restrict__ chunk_len, const int32_t* __restrict__ fin, int T, int N, int logN,
                  int hop, float mask_value, float* __restrict__ x, float* __restrict__ re,
                  float* __restrict__ im, void* __restrict__ state, size_t per) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float2* buf = (float2*)smem;
    float2* tw = buf + N;
    int32_t* stage = (int32_t*)(tw + N / 2);  // N words
    const int tid = threadIdx.x, t = blockIdx.x, b = blockIdx.y, F = N / 2 + 1;
    const StreamState st = stream_state(state, per, b, N, hop);
    const StreamPush p = stream_push(st.hdr, chunk_len[b], fin[b], stride, T, N, hop);
    const size_t o = ((size_t)b * T + t) * F;
    if (t >= p.nnew) {                        // (the whole workgroup: no barrier is skipped by a part of it)
        for (int i = tid; i < F; i += 256) x[o + i] = mask_value;
        return;
    }
    const int64_t g0 = (p.f0 + t) * hop - N;
    for (int i = tid; i < N; i += 256) {
        const int32_t w = stream_word(chunk, is_int16, (size_t)b * stride, st.in_carry, p, g0 + i, N, hop);
        if (is_int16) ((short*)stage)[i] = (short)w;
        else stage[i] = w;
    }
    __syncthreads();
    stft_frame((const void*)stage, is_int16, 0, N, N, logN, hop, N / hop, o, x, re, im, buf, tw, tid);
}

// behind the frames of a push: the samples the coming frames read become the carry, the counters move on
__global__ void __launch_bounds__(256)
stream_fwd_commit_kernel(const void* __restrict__ chunk, int is_int16, int64_t stride,
                         const int64_t* __restrict__ chunk_len, const int32_t* __restrict__ fin, int T, int N,
                         int hop, void* __restrict__ state, size_t per) {
    const int tid = threadIdx.x, b = blockIdx.x;
    const StreamState st = stream_state(state, per, b, N, hop);
    const StreamPush p = stream_push(st.hdr, chunk_len[b], fin[b], stride, T, N, hop);
    const int64_t cs = p.f1 * hop - N;        // the next frame's first sample
    int64_t cnt = p.closed ? 0 : p.n1 - cs;   // (n1 mod hop) + N - hop < N on an open stream
    cnt = cnt < 0 ? 0 : (cnt > N ? N : cnt);
    int32_t w[16];                            // N <= 4096 = 16 * 256
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int i = tid + 256 * q;
        w[q] = i < cnt ? stream_word(chunk, is_int16, (size_t)b * stride, st.in_carry, p, cs + i, N, hop) : 0;
    }
    __syncthreads();                          // every read of the old carry and the header is done
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int i = tid + 256 * q;
        if (i < N) st.in_carry[i] = w[q];
    }
    if (tid == 0) {
        st.hdr->n_in = p.n1;
        st.hdr->frames = p.f1;
        st.hdr->push_f0 = p.f0;
        st.hdr->push_new = p.nnew;
        st.hdr->closed = p.closed;
    }
}

// the frame range and the sample range of the push the state records
struct StreamOut {
    int64_t f0;                   // first new frame
    int nnew;
    int64_t out0, out1;           // samples [out0, out1) of the stream become final
    int closed;
};

__device__ __forceinline__ StreamOut stream_out(const StreamHdr* h, int T, int N, int hop, int crop) {
    StreamOut r;
    r.f0 = h->push_f0;
    r.nnew = h->push_new;
    if (r.nnew < 0) r.nnew = 0;
    if (r.nnew > T) r.nnew = T;
    if (r.f0 < 0) r.nnew = 0;
    r.closed = h->closed != 0;
    r.out0 = r.f0 * hop - N;
    if (r.out0 < 0) r.out0 = 0;
    const int64_t f1 = r.f0 + r.nnew;
    r.out1 = (r.closed ? (f1 - 1) * hop : f1 * hop) - N;        // closed: istft_mc's trim of the last N
    if (r.closed && crop && h->n_in < r.out1) r.out1 = h->n_in;
    if (r.out1 < r.out0 || r.nnew == 0) r.out1 = r.out0;
    return r;
}

// util.wavwrite's scaling without its peak normalisation (drnmf_stream.h)
__device__ __forceinline__ void stream_store(void* __restrict__ y, int out_int16, size_t i, float v) {
    if (out_int16) {
        float s = v * 32767.0f;
        s = fminf(fmaxf(s, -32767.0f), 32767.0f);
        ((int16_t*)y)[i] = (int16_t)(int)s;
    } else {
        ((float*)y)[i] = v;
    }
}

// A window of partial sums in LDS: ola[i] belongs to sample base + i.  One step adds `cnt` frames (frame w at
// window offset w hop, N samples each, ascending w), emits the first cnt hop samples, which no later frame
// reaches, and slides the window by them.  VPT * 256 >= N + (cnt - 1) hop.
template <int VPT, class FrameAt>
__device__ __forceinline__ void stream_ola_step(float* ola, int N, int hop, int cnt, int64_t base,
                                                const StreamOut& r, void* __restrict__ y, int out_int16,
                                                size_t yrow, int64_t stride_y, int tid, FrameAt frame_at) {
    const int span = N + (cnt - 1) * hop, adv = cnt * hop;
    float acc[VPT];
#pragma unroll
    for (int q = 0; q < VPT; ++q) {
        const int i = tid + 256 * q;
        acc[q] = 0.f;
        if (i < span) {
            acc[q] = ola[i];
            for (int w = 0; w < cnt; ++w) {
                const int n = i - w * hop;
                if (n >= 0 && n < N) acc[q] += frame_at(w, n);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < VPT; ++q) {
        const int i = tid + 256 * q;
        if (i < span) {
            if (i < adv) {
                const int64_t s = base + i;
                if (s >= r.out0 && s < r.out1 && s - r.out0 < stride_y)
                    stream_store(y, out_int16, yrow + (size_t)(s - r.out0), acc[q]);
            } else {
                ola[i - adv] = acc[q];
            }
        }
        if (i >= span - adv && i < span) ola[i] = 0.f;     // behind the slid window
    }
    __syncthreads();
}

// what both inverse kernels do around their frames: the carry into LDS, and at the end the zeros behind the row's
// samples and the carry back (zeros for a closed stream)
__device__ __forceinline__ void stream_ola_load(float* ola, int width, const StreamState& st, int N, int hop,
                                                int tid) {
    for (int i = tid; i < width; i += 256) ola[i] = i < N - hop ? st.ola[i] : 0.f;
    __syncthreads();
}

__device__ __forceinline__ void stream_ola_finish(const float* ola, const StreamState& st, const StreamOut& r,
                                                  int N, int hop, void* __restrict__ y, int out_int16,
                                                  size_t yrow, int64_t stride_y, int tid) {
    if (r.nnew > 0)
        for (int i = tid; i < N - hop; i += 256) st.ola[i] = r.closed ? 0.f : ola[i];
    int64_t n = r.out1 - r.out0;
    if (n > stride_y) n = stride_y;
    for (int64_t i = n + tid; i < stride_y; i += 256) stream_store(y, out_int16, yrow + (size_t)i, 0.f);
}

template <int R, int P>
__global__ void __launch_bounds__(256)
stream_inv_real_kernel(const float* __restrict__ re, const float* __restrict__ im,
                       const float* __restrict__ mask, int64_t ld_mask, int T, int logN, int hop, int crop,
                       int out_int16, void* __restrict__ y, int64_t stride_y, void* __restrict__ state,
                       size_t per) {
    constexpr int M = RealFft<R, P>::M, N = 2 * M, F = M + 1, MP = RealFft<R, P>::MP;
    __shared__ float2 tw[N / 2];
    __shared__ float2 bufs[4][MP];
    __shared__ float ola[4 * N];              // N + 3 hop in use
    auto pad = [](int i) { return RealFft<R, P>::pad(i); };
    const int tid = threadIdx.x, wv = tid >> 6, j = tid & 63;
    const int b = blockIdx.x;
    const StreamState st = stream_state(state, per, b, N, hop);
    const StreamOut r = stream_out(st.hdr, T, N, hop, crop);
    const size_t yrow = (size_t)b * stride_y;
    for (int i = tid; i < N / 2; i += 256) tw[i] = g_twiddle[logN - TAB_LOG_MIN][i];
    stream_ola_load(ola, N + 3 * hop, st, N, hop, tid);
    const float* __restrict__ win = g_window[logN - TAB_LOG_MIN];
    const float scale = (2.0f / ((float)N / (float)hop)) / (float)N;
    for (int tb = 0; tb < r.nnew; tb += 4) {  // (uniform over the workgroup)
        const int cnt = r.nnew - tb < 4 ? r.nnew - tb : 4;
        if (wv < cnt) {
            const size_t fr = (size_t)b * T + (size_t)(tb + wv);
            istft_real_frame<R, P>(re, im, mask, fr * F, fr * (size_t)ld_mask, tw, bufs[wv], win, scale, j);
        }
        __syncthreads();
        stream_ola_step<16>(ola, N, hop, cnt, (r.f0 + tb) * hop - N, r, y, out_int16, yrow, stride_y, tid,
                            [&](int w, int n) {
                                const float2 z = bufs[w][pad(n >> 1)];
                                return (n & 1) ? z.y : z.x;
                            });
    }
    stream_ola_finish(ola, st, r, N, hop, y, out_int16, yrow, stride_y, tid);
}

// other sizes: istft_frame into the stream's frame scratch, one frame per step
__global__ void __launch_bounds__(256)
stream_inv_kernel(const float* __restrict__ re, const float* __restrict__ im, const float* __restrict__ mask,
                  int64_t ld_mask, int T, int N, int logN, int hop, int crop, int out_int16,
                  void* __restrict__ y, int64_t stride_y, void* __restrict__ state, size_t per) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float2* buf = (float2*)smem;
    float2* tw = buf + N;
    float* ola = (float*)(tw + N / 2);        // N floats
    const int tid = threadIdx.x, b = blockIdx.x, F = N / 2 + 1;
    const StreamState st = stream_state(state, per, b, N, hop);
    const StreamOut r = stream_out(st.hdr, T, N, hop, crop);
    const size_t yrow = (size_t)b * stride_y;
    stream_ola_load(ola, N, st, N, hop, tid);
    float* __restrict__ frame = st.frame;
    for (int t = 0; t < r.nnew; ++t) {        // (uniform over the workgroup)
        const size_t fr = (size_t)b * T + (size_t)t;
        istft_frame(re, im, mask, fr * F, fr * (size_t)ld_mask, N, logN, hop, frame, buf, tw, tid);
        __syncthreads();                      // the frame is stored before it is added
        stream_ola_step<16>(ola, N, hop, 1, (r.f0 + t) * hop - N, r, y, out_int16, yrow, stride_y, tid,
                            [&](int, int n) { return frame[n]; });
    }
    stream_ola_finish(ola, st, r, N, hop, y, out_int16, yrow, stride_y, tid);
}

static int32_t check_stream(drnmf_handle_t h, const char* who, int32_t B, int32_t N, int32_t hop,
                            const void* state, size_t state_bytes) {
    if (B <= 0 || B > 65535)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: B=%d must lie in [1,65535]", who, B);
    if (const int32_t rc = check_fft_size(h, who, N, DRNMF_ERR_INVALID_ARG)) return rc;
    if (hop <= 0 || hop > N || N % hop)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: hop=%d must divide N=%d", who, hop, N);
    if (!state) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: NULL state", who);
    const size_t need = (size_t)B * stream_state_stride(N, hop);
    if (state_bytes < need)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "%s: state of %zu bytes is below drnmf_stream_state_bytes = %zu", who,
                   state_bytes, need);
    return DRNMF_OK;
}

}  // namespace

extern "C" int32_t drnmf_stream_counts(int64_t n_samples, int32_t closed, int32_t N, int32_t hop, int32_t crop,
                                       int64_t* frames, int64_t* samples) {
    if (n_samples < 0 || N <= 0 || hop <= 0 || N % hop || (closed != 0 && closed != 1) ||
        (crop != 0 && crop != 1) || !frames || !samples)
        return DRNMF_ERR_INVALID_ARG;
    if (!closed) {
        *frames = n_samples / hop + 1;
        const int64_t n = *frames * hop - N;
        *samples = n > 0 ? n : 0;
        return DRNMF_OK;
    }
    *frames = stft_frame_count(n_samples, N, hop);
    int64_t n = (int64_t)hop * (*frames - 1) - N;
    if (crop && n_samples < n) n = n_samples;
    *samples = n;
    return DRNMF_OK;
}

extern "C" size_t drnmf_stream_state_bytes(int32_t B, int32_t N, int32_t hop) {
    if (B <= 0 || B > 65535 || !fft_size_ok(N) || hop <= 0 || hop > N || N % hop) return 0;
    return (size_t)B * stream_state_stride(N, hop);
}

extern "C" int32_t drnmf_stream_reset(drnmf_handle_t h, int32_t B, int32_t N, int32_t hop, void* state,
                                      size_t state_bytes, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    const int32_t rc = check_stream(h, "stream_reset", B, N, hop, state, state_bytes);
    if (rc) return rc;
    const size_t n_words = (size_t)B * stream_state_stride(N, hop) / 4;
    hipLaunchKernelGGL(stream_reset_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream_, (uint32_t*)state, n_words);
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}

extern "C" int32_t drnmf_stream_forward(drnmf_handle_t h, int32_t B, int64_t stride, int32_t T, int32_t N,
                                        int32_t hop, int32_t is_int16, float mask_value, const void* chunk,
                                        const int64_t* chunk_len, const int32_t* final, float* x, float* re,
                                        float* im, void* state, size_t state_bytes, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (stride <= 0 || T <= 0 || (is_int16 != 0 && is_int16 != 1))
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "stream_forward: bad shape stride=%lld T=%d is_int16=%d",
                   (long long)stride, T, is_int16);
    if (!chunk || !chunk_len || !final || !x || !re || !im)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "stream_forward: NULL pointer argument");
    const int32_t rc = check_stream(h, "stream_forward", B, N, hop, state, state_bytes);
    if (rc) return rc;
    FftCall c;
    if (const int32_t trc = fft_call(h, N, stream_, &c)) return trc;
    const size_t per = stream_state_stride(N, hop);
    with_fft_size(N, [&](auto s) {
        using S = decltype(s);
        if constexpr (S::fast)
            hipLaunchKernelGGL((stream_fwd_real_kernel<S::R, S::P>), dim3((unsigned)((T + 3) / 4), (unsigned)B),
                               dim3(256), 0, c.stream, chunk, is_int16, stride, chunk_len, final, T, c.logN, hop,
                               mask_value, x, re, im, state, per);
        else                                  // behind the points and the twiddles: N words of stage
            hipLaunchKernelGGL(stream_fwd_kernel, dim3((unsigned)T, (unsigned)B), dim3(256),
                               c.lds + (size_t)N * sizeof(int32_t), c.stream, chunk, is_int16, stride, chunk_len,
                               final, T, N, c.logN, hop, mask_value, x, re, im, state, per);
    });
    hipLaunchKernelGGL(stream_fwd_commit_kernel, dim3((unsigned)B), dim3(256), 0, c.stream, chunk, is_int16, stride,
                       chunk_len, final, T, N, hop, state, per);
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}

extern "C" int32_t drnmf_stream_inverse(drnmf_handle_t h, int32_t B, int32_t T, int32_t N, int32_t hop,
                                        const float* re, const float* im, const float* mask, int64_t ld_mask,
                                        int32_t crop, int32_t out_int16, void* y, int64_t stride_y, void* state,
                                        size_t state_bytes, void* stream_) {
    DRNMF_LOCK(h);
    if (!h) return DRNMF_ERR_INVALID_ARG;
    if (T <= 0 || stride_y <= 0 || (crop != 0 && crop != 1) || (out_int16 != 0 && out_int16 != 1))
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "stream_inverse: bad shape T=%d stride_y=%lld crop=%d out_int16=%d", T,
                   (long long)stride_y, crop, out_int16);
    if (!re || !im || !y) DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "stream_inverse: NULL pointer argument");
    const int32_t rc = check_stream(h, "stream_inverse", B, N, hop, state, state_bytes);
    if (rc) return rc;
    if (mask && ld_mask < N / 2 + 1)
        DRNMF_FAIL(h, DRNMF_ERR_INVALID_ARG, "stream_inverse: ld_mask=%lld is below N/2+1=%d", (long long)ld_mask,
                   N / 2 + 1);
    FftCall c;
    if (const int32_t trc = fft_call(h, N, stream_, &c)) return trc;
    const size_t per = stream_state_stride(N, hop);
    with_fft_size(N, [&](auto s) {
        using S = decltype(s);
        if constexpr (S::fast)
            hipLaunchKernelGGL((stream_inv_real_kernel<S::R, S::P>), dim3((unsigned)B), dim3(256), 0, c.stream, re,
                               im, mask, ld_mask, T, c.logN, hop, crop, out_int16, y, stride_y, state, per);
        else                                  // behind the points and the twiddles: N floats of overlap-add
            hipLaunchKernelGGL(stream_inv_kernel, dim3((unsigned)B), dim3(256), c.lds + (size_t)N * sizeof(float),
                               c.stream, re, im, mask, ld_mask, T, N, c.logN, hop, crop, out_int16, y, stride_y,
                               state, per);
    });
    DRNMF_HIP(h, hipGetLastError());
    return DRNMF_OK;
}
