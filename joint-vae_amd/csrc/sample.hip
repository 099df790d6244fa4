// The two ends of image generation (reference module/sample.py::sample): noise -> prior draws, decoded rows -> image grid.
//
// Prior draws: z (R, K) = means[y] + (factor of the component applied to t * eps), y the row's label (NULL: component 0):
//   UNIT    z = m + t eps                  the reference's draw (module/sample.py:129-132): unit variance whatever the prior's
//   SCALAR  z = m + (t eps) / T[y]         DIAG  z = m + (t eps) / T[y, k]
//   FULL    z = m + u,  tril(T[y]) u = t eps    (the inverse of GaussianPrior.whiten, module/priors.py:228-233)
// The first three are one thread per element, every product / quotient / sum rounded on its own (__fmul_rn, __fdiv_rn,
// __fadd_rn: no contraction), i.e. the fp32 torch expressions bit for bit.  FULL is a forward substitution, ONE WAVE per row
// whatever the launch: lane l keeps u[l], u[l + 64], ... in registers; step k sums T[k, j] u[j] over the lane's own j < k in
// ascending j (fmaf), the 64 partial sums by the xor butterfly (the same value in every lane), u[k] = (t eps[k] - sum) / T[k, k].
// Row k of T is read contiguously by the wave.  The order of every sum is fixed by K alone.
//
// Image grid: cell (row n, column c) of the grid is an input image, one decoded row, or the mean of a run of decoded rows
// (summed in ascending row order, then ONE division); the fp32 grid (D, N H, Ncol W) and / or the 8-bit, channel-last grid
// (N H, Ncol W, D) an image writer wants: floor(min(max(v * 255 + 0.5, 0), 255)), product and sum rounded separately, NaN -> 0
// (torchvision's save_image arithmetic).  A pure streaming kernel: a thread owns VEC = 4 (16-byte loads and stores; W a
// multiple of 4 and 16-byte aligned tensors) or 1 consecutive pixels of one grid line, all D channels of them, so the D bytes of
// a pixel are written by one thread.  Grid-stride, no LDS.
// No atomics in either kernel: one writer per output element, the same bits run to run.
#include "common.h"
#include "jvae_internal.h"
#include <algorithm>

// __fmul_rn / __fadd_rn / __fdiv_rn are the plain operators in this toolchain's headers: contraction is switched off for the whole
// file so that no product meets a sum in an fma behind them (the substitution's fmaf is written out)
#pragma clang fp contract(off)

namespace {

enum { PS_UNIT = 0, PS_SCALAR = 1, PS_DIAG = 2, PS_FULL = 3 };
constexpr int PS_BLOCK = 256;
constexpr int PS_MAX_K = 1024;
constexpr int PS_MAX_BLOCKS = 2048;

__global__ __launch_bounds__(PS_BLOCK) void prior_sample_kernel(const float* __restrict__ eps, const long long* __restrict__ y,
                                                                const float* __restrict__ means, const float* __restrict__ T,
                                                                float* __restrict__ z, int* __restrict__ status, long R, int K,
                                                                int C, float t, int mode) {
    const long total = R * (long)K;
    for (long i = (long)blockIdx.x * PS_BLOCK + threadIdx.x; i < total; i += (long)gridDim.x * PS_BLOCK) {
        const long r = i / K;
        const int k = (int)(i - r * K);
        long long c = 0;
        if (y) {
            c = y[r];
            if (c < 0 || c >= (long long)C) {
                z[i] = NAN;
                *status = 1;                   // every writer stores the same word
                continue;
            }
        }
        float v = __fmul_rn(t, eps[i]);
        if (mode == PS_SCALAR) v = __fdiv_rn(v, T[c]);
        else if (mode == PS_DIAG) v = __fdiv_rn(v, T[(size_t)c * K + k]);
        z[i] = __fadd_rn(means[(size_t)c * K + k], v);
    }
}

// NI = ceil(K / 64) rounded up to a power of two: the registers of u, indexed at compile time throughout
template <int NI>
__global__ __launch_bounds__(PS_BLOCK) void prior_sample_full_kernel(const float* __restrict__ eps, const long long* __restrict__ y,
                                                                     const float* __restrict__ means, const float* __restrict__ T,
                                                                     float* __restrict__ z, int* __restrict__ status, long R,
                                                                     int K, int C, float t) {
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * (PS_BLOCK / 64) + (threadIdx.x >> 6), nwaves = (long)gridDim.x * (PS_BLOCK / 64);
    for (long r = wave; r < R; r += nwaves) {          // wave-uniform: all 64 lanes stay together
        long long c = 0;
        bool bad = false;
        if (y) {
            c = y[r];
            bad = c < 0 || c >= (long long)C;
        }
        const float* __restrict__ e = eps + (size_t)r * K;
        float* __restrict__ zr = z + (size_t)r * K;
        if (bad) {
            for (int j = lane; j < K; j += 64) zr[j] = NAN;
            if (lane == 0) *status = 1;
            continue;
        }
        const float* __restrict__ Tc = T + (size_t)c * K * K;
        float u[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) u[i] = 0.f;
#pragma unroll
        for (int ik = 0; ik < NI; ++ik) {
            const int kend = min(K - ik * 64, 64);     // <= 0: nothing left
            for (int kk = 0; kk < kend; ++kk) {
                const int k = ik * 64 + kk;
                const float* __restrict__ row = Tc + (size_t)k * K;
                float s = 0.f;
#pragma unroll
                for (int i = 0; i <= ik; ++i) {
                    const int j = i * 64 + lane;
                    if (j < k) s = fmaf(row[j], u[i], s);
                }
                s = wave_sum(s);
                const float uk = __fdiv_rn(__fsub_rn(__fmul_rn(t, e[k]), s), row[k]);
                if (lane == kk) u[ik] = uk;
            }
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int j = i * 64 + lane;
            if (j < K) zr[j] = __fadd_rn(means[(size_t)c * K + j], u[i]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- image grid
enum { IG_INPUT = 0, IG_DRAW = 1, IG_AVERAGE = 2 };
constexpr int IG_BLOCK = 256;
constexpr int IG_MAX_COLS = 1024;
constexpr int IG_MAX_BLOCKS = 2048;

template <int VEC> struct IgVec;
template <> struct IgVec<1> { typedef float type; };
template <> struct IgVec<4> { typedef f32x4 type; };

__device__ __forceinline__ float ig_get(float v, int) { return v; }
__device__ __forceinline__ float ig_get(f32x4 v, int j) { return v[j]; }
__device__ __forceinline__ void ig_set(float& v, int, float x) { v = x; }
__device__ __forceinline__ void ig_set(f32x4& v, int j, float x) { v[j] = x; }

__device__ __forceinline__ unsigned ig_quant(float v) {
    float q = __fadd_rn(__fmul_rn(v, 255.f), 0.5f);
    q = q > 0.f ? q : 0.f;                     // NaN -> 0
    q = q < 255.f ? q : 255.f;
    return (unsigned)(int)q;                   // q >= 0: the truncation is floor
}

// DU8 = 0: no 8-bit grid, D at run time; DU8 = 1 .. 4: D == DU8, channel loop unrolled, the VEC * D bytes of a thread packed in words
template <int VEC, int DU8>
__global__ __launch_bounds__(IG_BLOCK) void image_grid_kernel(const float* __restrict__ x_in, const float* __restrict__ x_out,
                                                              const int* __restrict__ specs, float* __restrict__ gf,
                                                              unsigned char* __restrict__ gu, int N, int Drt, int H, int W,
                                                              int Ncol) {
    typedef typename IgVec<VEC>::type vec_t;
    constexpr int DUNROLL = DU8 ? DU8 : 1;
    const int D = DU8 ? DU8 : Drt;
    const int WV = W / VEC;
    const long items = (long)N * H * Ncol * WV;
    const size_t plane = (size_t)H * W, image = plane * D, draw = image * N;      // elements of one channel, image, decoded row
    const size_t line = (size_t)Ncol * W;                                          // pixels of one grid line
    for (long it = (long)blockIdx.x * IG_BLOCK + threadIdx.x; it < items; it += (long)gridDim.x * IG_BLOCK) {
        const int wv = (int)(it % WV);
        long q = it / WV;
        const int c = (int)(q % Ncol);
        q /= Ncol;
        const int h = (int)(q % H), n = (int)(q / H);
        const int kind = specs[3 * c], a = specs[3 * c + 1], b = specs[3 * c + 2];
        const size_t pix = (size_t)h * W + (size_t)wv * VEC;                       // inside a plane
        const size_t gpix = ((size_t)n * H + h) * line + (size_t)c * W + (size_t)wv * VEC;
        unsigned bytes[VEC * DUNROLL];
#pragma unroll DUNROLL
        for (int d = 0; d < D; ++d) {
            vec_t v;
            if (kind == IG_INPUT) {
                v = *reinterpret_cast<const vec_t*>(x_in + (size_t)n * image + d * plane + pix);
            } else {
                const float* __restrict__ src = x_out + (size_t)n * image + d * plane + pix;
                v = *reinterpret_cast<const vec_t*>(src + (size_t)a * draw);
                if (kind == IG_AVERAGE) {
                    const float cnt = (float)(b - a + 1);
#pragma unroll 4
                    for (int l = a + 1; l <= b; ++l) {
                        const vec_t w = *reinterpret_cast<const vec_t*>(src + (size_t)l * draw);
#pragma unroll
                        for (int j = 0; j < VEC; ++j) ig_set(v, j, __fadd_rn(ig_get(v, j), ig_get(w, j)));
                    }
#pragma unroll
                    for (int j = 0; j < VEC; ++j) ig_set(v, j, __fdiv_rn(ig_get(v, j), cnt));
                }
            }
            if (gf) *reinterpret_cast<vec_t*>(gf + (size_t)d * N * H * line + gpix) = v;
            if (DU8) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) bytes[j * DUNROLL + d] = ig_quant(ig_get(v, j));
            }
        }
        if (DU8) {
            unsigned char* __restrict__ dst = gu + gpix * DU8;
            if (VEC == 4) {                    // 4 * D bytes at a multiple of 4 * D: D aligned words
#pragma unroll
                for (int w = 0; w < DU8; ++w)
                    reinterpret_cast<unsigned*>(dst)[w] = bytes[4 * w] | bytes[4 * w + 1] << 8 | bytes[4 * w + 2] << 16 | bytes[4 * w + 3] << 24;
            } else {
#pragma unroll
                for (int d = 0; d < DU8; ++d) dst[d] = (unsigned char)bytes[d];
            }
        }
    }
}

template <int VEC>
int image_grid_launch(const float* x_in, const float* x_out, const int* specs, float* gf, unsigned char* gu, int N, int D, int H,
                      int W, int Ncol, hipStream_t st) {
    const long items = (long)N * H * Ncol * (W / VEC);
    const int blocks = std::min(cdiv(items, IG_BLOCK), IG_MAX_BLOCKS);
#define IG_GO(DU8) image_grid_kernel<VEC, DU8><<<blocks, IG_BLOCK, 0, st>>>(x_in, x_out, specs, gf, gu, N, D, H, W, Ncol)
    if (!gu) IG_GO(0);
    else if (D == 1) IG_GO(1);
    else if (D == 2) IG_GO(2);
    else if (D == 3) IG_GO(3);
    else IG_GO(4);
#undef IG_GO
    JVAE_LAUNCH_CHECK();
    return 0;
}

inline bool aligned_to(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" {

int jvae_prior_sample_f32(const float* eps, const long long* y, const float* means, const float* T, float* z, int* status,
                          long R, int K, int C, float t, int mode, void* stream) {
    if (!eps || !means || !z || !status || R < 0 || K < 1 || K > PS_MAX_K || C < 1 || mode < PS_UNIT || mode > PS_FULL)
        return JVAE_EINVAL;
    if (mode != PS_UNIT && !T) return JVAE_EINVAL;
    if (R > (1L << 40) / K) return JVAE_EINVAL;
    if (R == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (mode != PS_FULL) {
        const int blocks = std::min(cdiv(R * K, PS_BLOCK), PS_MAX_BLOCKS);
        prior_sample_kernel<<<blocks, PS_BLOCK, 0, st>>>(eps, y, means, T, z, status, R, K, C, t, mode);
    } else {
        const int blocks = std::min(cdiv(R, PS_BLOCK / 64), PS_MAX_BLOCKS);
#define PS_GO(NI) prior_sample_full_kernel<NI><<<blocks, PS_BLOCK, 0, st>>>(eps, y, means, T, z, status, R, K, C, t)
        if (K <= 64) PS_GO(1);
        else if (K <= 128) PS_GO(2);
        else if (K <= 256) PS_GO(4);
        else if (K <= 512) PS_GO(8);
        else PS_GO(16);
#undef PS_GO
    }
    JVAE_LAUNCH_CHECK();
    return 0;
}

int jvae_image_grid_f32(const float* x_in, const float* x_out, const int* specs, const int* specs_host, int Ncol, float* grid_f32,
                        unsigned char* grid_u8, int N, int D, int H, int W, int Rr, void* stream) {
    if (!x_out || !specs || !specs_host || (!grid_f32 && !grid_u8) || Ncol < 1 || Ncol > IG_MAX_COLS || N < 1 || D < 1 || H < 1
        || W < 1 || Rr < 1)
        return JVAE_EINVAL;
    for (int c = 0; c < Ncol; ++c) {
        const int kind = specs_host[3 * c], a = specs_host[3 * c + 1], b = specs_host[3 * c + 2];
        if (kind < IG_INPUT || kind > IG_AVERAGE) return JVAE_EINVAL;
        if (kind == IG_INPUT) {
            if (!x_in) return JVAE_EINVAL;
            continue;
        }
        if (a < 0 || a >= Rr || b < 0 || b >= Rr || (kind == IG_AVERAGE && b < a)) return JVAE_EINVAL;
    }
    if (grid_u8 && D > 4) return JVAE_ENOTSUP;
    // every index is 64-bit; the bound keeps the products of the extents themselves inside a long
    if ((double)N * D * H * W * (double)std::max(Rr, Ncol) > 1e15) return JVAE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = W % 4 == 0 && aligned_to(x_out, 16) && (!x_in || aligned_to(x_in, 16)) && (!grid_f32 || aligned_to(grid_f32, 16))
                     && (!grid_u8 || aligned_to(grid_u8, 4));
    return vec ? image_grid_launch<4>(x_in, x_out, specs, grid_f32, grid_u8, N, D, H, W, Ncol, st)
               : image_grid_launch<1>(x_in, x_out, specs, grid_f32, grid_u8, N, D, H, W, Ncol, st);
}

}  // extern "C"
