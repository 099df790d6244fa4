// Chained models (reference module/cascad.py): two kernels.
//
// 1. Stage-pair mean squared errors.  x (N, D) is stage 0 (the same for every draw), R_1 .. R_M (L, N, D) the sampled
//    reconstructions of the M models of a cascade; one row per pair of stages, in the reference's order
//    `for i in 1..M: for j in 0..i-1` (p = i (i - 1) / 2 + j):
//      mse[p, n] = 1 / (L D) sum_{l, d} (R_i[l, n, d] - R_j[l, n, d])^2
//    The reference forms the rows pair by pair: an (L, N, D) temporary and two full reads per pair.  Here ONE pass: a workgroup
//    owns a sample and a chunk of 256 consecutive d (a lane: 4 of them), its four waves deal the draws round-robin
//    (l = w, w + 4, ...).  The chunk of x is fetched from memory once and handed to the four waves through LDS; every stage
//    element is loaded once and feeds ALL M (M + 1) / 2 accumulators of its lane (M a template parameter: the accumulators
//    stay in registers).  Differences and squares are taken in fp64 - the fp32 operands are exact in it.  The 64 lanes of a wave are
//    folded by a butterfly, the four waves as (w0 + w1) + (w2 + w3) through LDS, and one fp64 partial per (chunk, row, sample)
//    goes to the workspace; the second kernel adds the chunks in ascending order and divides once.  No atomics: the order of
//    every sum hangs on (L, D) alone.  A lane reads its 4 values with one 16-byte load where D % 4 == 0 and every base pointer is
//    16-byte aligned, else (a view x_reco[1:] of an odd-sized tensor) with 4 guarded 4-byte loads - the same values into the same
//    sums, so both paths give the same bits.
// 2. Sequential Bayesian update (iterate_with_prior).  p (M, C, N) -> posterior (M, C, N), one thread per sample:
//      prior_0 = 1 / C;  joint = p[i] prior;  posterior[i] = joint / sum_c joint;  prior = posterior[i]
//    The prior of stage i is read back from the output slot of stage i - 1, written by the same thread.  Products and class sums
//    in fp64 (ascending c), one rounding on the way out.  A stage whose class sum is 0 gives 0 / 0 = NaN for that sample from
//    that stage on.
#include "common.h"
#include "jvae_internal.h"
#include <math.h>

// every product and sum below is rounded on its own unless written as fma
#pragma clang fp contract(off)

namespace {

constexpr int CS_BLOCK = 256;
constexpr int CS_WAVES = CS_BLOCK / 64;
constexpr int CS_QUAD = 4;                         // consecutive d of a lane
constexpr int CS_CHUNK = 64 * CS_QUAD;             // d of a workgroup
constexpr int CS_MAX_M = 8;
constexpr int CS_MAX_C = 128;                      // ops.MISCLASS_MAX_CLASSES
constexpr long CS_MAX_N = 1L << 30;
constexpr long CS_MAX_THREADS = (1L << 32) - 1;        // of one launch: N x ceil(D / 256) workgroups of 256 threads

struct Stages { const float* r[CS_MAX_M]; };      // by value in the kernel arguments, as AggArgs

// the 4 values of a lane at row + d0: one 16-byte load, or 4 guarded loads (0 past the end of the row: it adds nothing)
template <bool VEC>
__device__ __forceinline__ void load_quad(const float* __restrict__ row, long d0, long D, float (&v)[CS_QUAD]) {
    if constexpr (VEC) {
        if (d0 < D) {
            const float4 q = *reinterpret_cast<const float4*>(row + d0);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            v[0] = v[1] = v[2] = v[3] = 0.f;
        }
    } else {
#pragma unroll
        for (int k = 0; k < CS_QUAD; ++k) v[k] = d0 + k < D ? row[d0 + k] : 0.f;
    }
}

template <int M, bool VEC>
__global__ __launch_bounds__(CS_BLOCK) void cascade_mse_kernel(const float* __restrict__ x, Stages st, double* __restrict__ part,
                                                               int L, long N, long D) {
    constexpr int P = M * (M + 1) / 2;
    __shared__ float xs[CS_CHUNK];
    __shared__ double red[CS_WAVES][P];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long n = blockIdx.x;
    const long d0 = (long)blockIdx.y * CS_CHUNK + lane * CS_QUAD;
    if (w == 0) {                                                  // the only read of this chunk of x
        float q[CS_QUAD];
        load_quad<VEC>(x + (size_t)n * D, d0, D, q);
#pragma unroll
        for (int k = 0; k < CS_QUAD; ++k) xs[lane * CS_QUAD + k] = q[k];
    }
    __syncthreads();
    double x0[CS_QUAD];
#pragma unroll
    for (int k = 0; k < CS_QUAD; ++k) x0[k] = (double)xs[lane * CS_QUAD + k];
    double acc[P];
#pragma unroll
    for (int p = 0; p < P; ++p) acc[p] = 0.;
    for (int l = w; l < L; l += CS_WAVES) {
        const size_t at = ((size_t)l * N + n) * D;
        float q[M][CS_QUAD];
#pragma unroll
        for (int i = 0; i < M; ++i) load_quad<VEC>(st.r[i] + at, d0, D, q[i]);
#pragma unroll
        for (int k = 0; k < CS_QUAD; ++k) {
            double v[M + 1];
            v[0] = x0[k];
#pragma unroll
            for (int i = 0; i < M; ++i) v[i + 1] = (double)q[i][k];
            int p = 0;
#pragma unroll
            for (int i = 1; i <= M; ++i)
#pragma unroll
                for (int j = 0; j < i; ++j, ++p) {
                    const double df = v[i] - v[j];
                    acc[p] = fma(df, df, acc[p]);
                }
        }
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
        double s = acc[p];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) red[w][p] = s;
    }
    __syncthreads();
    if (threadIdx.x < P)
        part[((size_t)blockIdx.y * P + threadIdx.x) * N + n] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

__global__ __launch_bounds__(CS_BLOCK) void cascade_mse_fold_kernel(const double* __restrict__ part, float* __restrict__ mse,
                                                                    int chunks, int P, long N, double count) {
    const long n = (long)blockIdx.x * CS_BLOCK + threadIdx.x;
    if (n >= N) return;
    const int p = blockIdx.y;
    double s = 0.;
    for (int c = 0; c < chunks; ++c) s += part[((size_t)c * P + p) * N + n];
    mse[(size_t)p * N + n] = (float)(s / count);
}

template <int M>
void cascade_mse_launch(bool vec, dim3 grid, hipStream_t s, const float* x, const Stages& st, double* part, int L, long N, long D) {
    if (vec) cascade_mse_kernel<M, true><<<grid, CS_BLOCK, 0, s>>>(x, st, part, L, N, D);
    else cascade_mse_kernel<M, false><<<grid, CS_BLOCK, 0, s>>>(x, st, part, L, N, D);
}

// ------------------------------------------------------------------------------------------- 2. sequential Bayesian update
__global__ __launch_bounds__(CS_BLOCK) void iterate_prior_kernel(const float* __restrict__ p, float* post, int M, int C, long N) {
    const long n = (long)blockIdx.x * CS_BLOCK + threadIdx.x;
    if (n >= N) return;
    const size_t plane = (size_t)C * N;
    const double flat = 1. / (double)C;
    for (int i = 0; i < M; ++i) {
        const float* __restrict__ pi = p + (size_t)i * plane + n;
        const float* prior = i ? post + (size_t)(i - 1) * plane + n : nullptr;     // this thread's own slots of the stage before
        float* out = post + (size_t)i * plane + n;
        double sum = 0.;
        for (int c = 0; c < C; ++c) sum += (double)pi[(size_t)c * N] * (prior ? (double)prior[(size_t)c * N] : flat);
        for (int c = 0; c < C; ++c)
            out[(size_t)c * N] = (float)((double)pi[(size_t)c * N] * (prior ? (double)prior[(size_t)c * N] : flat) / sum);
    }
}

}  // namespace

extern "C" {

size_t jvae_cascade_mse_workspace_bytes(int M, long N, long D) {
    if (M < 1 || M > CS_MAX_M || N < 1 || D < 1) return 0;
    return sizeof(double) * (size_t)cdiv(D, CS_CHUNK) * (size_t)(M * (M + 1) / 2) * (size_t)N;
}

int jvae_cascade_mse_f32(const float* x, const void* const* stages, int M, float* mse, int L, long N, long D, void* ws,
                         size_t ws_bytes, void* stream) {
    if (!x || !stages || !mse || M < 1 || M > CS_MAX_M || L < 1 || N < 0 || N > CS_MAX_N || D < 1 || D > 65535L * CS_CHUNK)
        return JVAE_EINVAL;
    if ((double)N * (double)cdiv(D, CS_CHUNK) * CS_BLOCK > (double)CS_MAX_THREADS) return JVAE_EINVAL;
    if ((double)L * (double)N * (double)D > 1e15) return JVAE_EINVAL;
    Stages st;
    uintptr_t bits = (uintptr_t)x;
    for (int i = 0; i < CS_MAX_M; ++i) {
        st.r[i] = i < M ? static_cast<const float*>(stages[i]) : nullptr;
        if (i < M && !st.r[i]) return JVAE_EINVAL;
        bits |= (uintptr_t)st.r[i];
    }
    if ((bits & 3) || ((uintptr_t)mse & 3)) return JVAE_EINVAL;
    if (N == 0) return 0;
    if (!ws || ((uintptr_t)ws & 7)) return JVAE_EINVAL;
    if (ws_bytes < jvae_cascade_mse_workspace_bytes(M, N, D)) return JVAE_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int chunks = cdiv(D, CS_CHUNK), P = M * (M + 1) / 2;
    const bool vec = D % CS_QUAD == 0 && !(bits & 15);
    const dim3 grid((unsigned)N, (unsigned)chunks);
    double* part = (double*)ws;
    switch (M) {
        case 1: cascade_mse_launch<1>(vec, grid, s, x, st, part, L, N, D); break;
        case 2: cascade_mse_launch<2>(vec, grid, s, x, st, part, L, N, D); break;
        case 3: cascade_mse_launch<3>(vec, grid, s, x, st, part, L, N, D); break;
        case 4: cascade_mse_launch<4>(vec, grid, s, x, st, part, L, N, D); break;
        case 5: cascade_mse_launch<5>(vec, grid, s, x, st, part, L, N, D); break;
        case 6: cascade_mse_launch<6>(vec, grid, s, x, st, part, L, N, D); break;
        case 7: cascade_mse_launch<7>(vec, grid, s, x, st, part, L, N, D); break;
        default: cascade_mse_launch<8>(vec, grid, s, x, st, part, L, N, D); break;
    }
    JVAE_LAUNCH_CHECK();
    cascade_mse_fold_kernel<<<dim3((unsigned)cdiv(N, CS_BLOCK), (unsigned)P), CS_BLOCK, 0, s>>>(part, mse, chunks, P, N,
                                                                                               (double)L * (double)D);
    JVAE_LAUNCH_CHECK();
    return 0;
}

int jvae_iterate_prior_f32(const float* p, float* posterior, int M, int C, long N, void* stream) {
    if (!p || !posterior || p == posterior || M < 1 || M > CS_MAX_M || C < 1 || C > CS_MAX_C || N < 0 || N > CS_MAX_N)
        return JVAE_EINVAL;
    if (N == 0) return 0;
    iterate_prior_kernel<<<cdiv(N, CS_BLOCK), CS_BLOCK, 0, (hipStream_t)stream>>>(p, posterior, M, C, N);
    JVAE_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
