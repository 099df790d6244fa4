// The padded bitonic sort of score rows shared by the ROC (roc.hip), the precision-recall figures (prc.hip) and the SCOD risk
// curves (scod.hip): the order-preserving integer image of fp32 scores, the row padding, the compare-exchange passes for 32- and
// 64-bit keys, and what roc.hip and prc.hip both need of a row's mode: its decoded mode word and the centre of an around-mean row.
//
// Rows are padded to a power of two (>= one tile) with the largest key, which sorts behind every real key.  Strides below the
// 2048-key tile run in LDS, longer ones in HBM.  Everything lives in an unnamed namespace: each translation unit that includes
// this header gets kernels of its own.
#pragma once
#include "common.h"
#include "jvae_internal.h"

namespace {

constexpr int ROC_TILE = 2048;         // keys per workgroup of the LDS passes (16 KiB of uint64)
constexpr int ROC_TILE_THREADS = 1024; // one compare-exchange per thread and pass
constexpr long ROC_MAX_N = 1L << 24;   // counts stay in int32 and M rows of padded keys in a 32-bit grid

__host__ __device__ inline long roc_pad(long n) {
    long p = ROC_TILE;
    while (p < n) p <<= 1;
    return p;
}

// fp32 -> uint32 with the order of the floats (-inf < ... < -0 < +0 < ... < +inf), and back
__device__ __forceinline__ uint32_t roc_key(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float roc_unkey(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
// roc_key with -0 canonicalised to +0: IEEE-equal scores are ONE key, as they are one value to numpy.  For every caller that
// compares KEYS (tie groups in prc.hip) or breaks ties by a payload packed behind the key (positions in scod.hip); a caller
// that compares the decoded floats (roc.hip) keeps roc_key, whose image roc_unkey inverts bit for bit.
__device__ __forceinline__ uint32_t roc_key_canonical(float v) {
    return roc_key((__float_as_uint(v) & 0x7FFFFFFFu) ? v : 0.0f);
}

// Mode word of a row -> 0 one-sided, 1 around-mean, 2 strided quantiles with the factors f_low = bits 8-15 and f_up = bits
// 16-23, each in [1, 255], of the word 2 | f_low << 8 | f_up << 16; -1: the word decodes to nothing.
__device__ __forceinline__ int roc_decode(int w, int& f_low, int& f_up) {
    f_low = (w >> 8) & 255;
    f_up = (w >> 16) & 255;
    if (w == 0 || w == 1) return w;
    return ((w & 255) == 2 && (w >> 24) == 0 && f_low >= 1 && f_up >= 1) ? 2 : -1;
}

// c = mean(ins) in fp64 of the around-mean rows (roc_curves.py:69): strided partial sums, then a fixed tree.  Shared by the ROC
// and the precision-recall figures (prc.hip), whose around-mean scores are distances to the same centre, bit for bit.
__global__ __launch_bounds__(1024) void roc_mean_kernel(const float* __restrict__ ins, const int* __restrict__ modes,
                                                        double* __restrict__ c, long n) {
    const int m = blockIdx.x, t = threadIdx.x;
    if (modes[m] != 1) return;
    __shared__ double red[1024];
    double s = 0.0;
    for (long i = t; i < n; i += 1024) s += (double)ins[(size_t)m * n + i];
    red[t] = s;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) c[m] = red[0] / (double)n;
}

// Compare-exchange passes of the bitonic network that fit one tile.  k == 0: the whole local sort (k = 2 ... ROC_TILE);
// k > ROC_TILE: the tail j = ROC_TILE/2 ... 1 of merge stage k.  Element g sorts ascending where (g & k) == 0.
// modes (may be NULL): only the rows whose mode word is 1 are sorted.
template <typename KT>
__global__ __launch_bounds__(ROC_TILE_THREADS) void roc_bitonic_tile_kernel(KT* __restrict__ keys, long P,
                                                                            const int* __restrict__ modes, long k) {
    if (modes && modes[blockIdx.y] != 1) return;
    __shared__ KT s[ROC_TILE];
    const int t = threadIdx.x;
    const long base = (long)blockIdx.x * ROC_TILE;
    KT* row = keys + (size_t)blockIdx.y * P + base;
    s[t] = row[t];
    s[t + ROC_TILE_THREADS] = row[t + ROC_TILE_THREADS];
    __syncthreads();
    for (long kk = k ? k : 2; kk <= (k ? k : (long)ROC_TILE); kk <<= 1) {
        for (int j = (int)(kk < ROC_TILE ? kk : ROC_TILE) >> 1; j > 0; j >>= 1) {
            const int i = 2 * t - (t & (j - 1));
            const bool up = ((base + i) & kk) == 0;
            const KT a = s[i], b = s[i + j];
            if ((a > b) == up) { s[i] = b; s[i + j] = a; }
            __syncthreads();
        }
    }
    row[t] = s[t];
    row[t + ROC_TILE_THREADS] = s[t + ROC_TILE_THREADS];
}

// One pass (k, j) with j >= ROC_TILE: partners are in different tiles
template <typename KT>
__global__ __launch_bounds__(256) void roc_bitonic_step_kernel(KT* __restrict__ keys, long P, const int* __restrict__ modes,
                                                               long k, long j) {
    if (modes && modes[blockIdx.y] != 1) return;
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (P >> 1)) return;
    const long i = 2 * g - (g & (j - 1));
    KT* row = keys + (size_t)blockIdx.y * P;
    const bool up = (i & k) == 0;
    const KT a = row[i], b = row[i + j];
    if ((a > b) == up) { row[i] = b; row[i + j] = a; }
}

// M rows of P keys each (P = roc_pad(n)), ascending
template <typename KT>
int roc_sort_rows(KT* keys, long P, int M, const int* modes, hipStream_t st) {
    const dim3 tiles((unsigned)(P / ROC_TILE), (unsigned)M), pairs((unsigned)cdiv(P >> 1, 256), (unsigned)M);
    roc_bitonic_tile_kernel<KT><<<tiles, ROC_TILE_THREADS, 0, st>>>(keys, P, modes, 0);
    JVAE_LAUNCH_CHECK();
    for (long k = 2L * ROC_TILE; k <= P; k <<= 1) {
        for (long j = k >> 1; j >= ROC_TILE; j >>= 1) {
            roc_bitonic_step_kernel<KT><<<pairs, 256, 0, st>>>(keys, P, modes, k, j);
            JVAE_LAUNCH_CHECK();
        }
        roc_bitonic_tile_kernel<KT><<<tiles, ROC_TILE_THREADS, 0, st>>>(keys, P, modes, k);
        JVAE_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace
