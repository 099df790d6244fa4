// The BatchNorm arithmetic that the fp32 NCHW kernels (bn.hip) and the bf16 B8 kernels (bn_b8.hip) share, written once: the
// coefficients of y = fmaf(x, scale, shift), the fp64 fold of a channel's partial sums, the moments with their publication, the
// walk over an fp32 channel plane and the host's choice of where the forward statistics come from.  What differs per layout on
// purpose (split / chunk thresholds, MAX_SPLIT, finalize-inside-apply versus a finalize launch, leaky ReLU) stays in the two files.
#pragma once
#include <type_traits>
#include "common.h"

// y = fmaf(x, scale, shift): one definition so that backward re-derives the forward's ReLU mask bit-exactly
__device__ __forceinline__ void bn_coef(float g, float b, float mean, float invstd, float* sc, float* sh) {
    *sc = g * invstd;
    *sh = b - mean * (g * invstd);
}

// ---- fp64 fold of partial[c][0..nsplit) = (s1, s2) pairs, in a fixed order per thread shape -----------------------------------
//   BN_FOLD_THREAD      one thread, s = 0, 1, 2, ...                                  bn_bwd_apply_kernel, bn_fold_kernel
//   BN_FOLD_WAVE        one wave (a 64-thread block): stride 64, xor butterfly 32..1    bn8_finalize / bn8_bwd_finalize / bn8_fold
//   BN_FOLD_BLOCK_SEQ   256 threads: stride 256, butterfly per wave, ((w0+w1)+w2)+w3    bn_apply_kernel
//   BN_FOLD_BLOCK_PAIR  256 threads: the same, but (w0+w1)+(w2+w3)                      bn_finalize_kernel
// The two block shapes differ in how they add the four wave sums, which shows in the last bit once nsplit > 128 (a convolution that
// hands over more than two waves' worth of tile partials).  Nobody chose that; it is kept so that every caller computes the bits
// it always did.  The block shapes need `dred` (LDS, 2 x 4 doubles), contain a barrier and return the sums in every thread; the
// wave shape returns them in every lane.
enum BnFold { BN_FOLD_THREAD, BN_FOLD_WAVE, BN_FOLD_BLOCK_SEQ, BN_FOLD_BLOCK_PAIR };
struct BnSums { double s1, s2; };
template <BnFold SHAPE>
__device__ __forceinline__ BnSums bn_fold(const float* __restrict__ partial, int c, int nsplit, double (*dred)[4] = nullptr) {
    constexpr int step = SHAPE == BN_FOLD_THREAD ? 1 : (SHAPE == BN_FOLD_WAVE ? 64 : 256);
    BnSums t = {0., 0.};
    for (int s = SHAPE == BN_FOLD_THREAD ? 0 : (int)threadIdx.x; s < nsplit; s += step) {
        t.s1 += (double)partial[((long)c * nsplit + s) * 2 + 0];
        t.s2 += (double)partial[((long)c * nsplit + s) * 2 + 1];
    }
    if constexpr (SHAPE != BN_FOLD_THREAD) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { t.s1 += __shfl_xor(t.s1, o, 64); t.s2 += __shfl_xor(t.s2, o, 64); }
    }
    if constexpr (SHAPE == BN_FOLD_BLOCK_SEQ || SHAPE == BN_FOLD_BLOCK_PAIR) {
        if ((threadIdx.x & 63) == 0) { dred[0][threadIdx.x >> 6] = t.s1; dred[1][threadIdx.x >> 6] = t.s2; }
        __syncthreads();
        if constexpr (SHAPE == BN_FOLD_BLOCK_SEQ) {
            t.s1 = dred[0][0] + dred[0][1] + dred[0][2] + dred[0][3];
            t.s2 = dred[1][0] + dred[1][1] + dred[1][2] + dred[1][3];
        } else {
            t.s1 = (dred[0][0] + dred[0][1]) + (dred[0][2] + dred[0][3]);
            t.s2 = (dred[1][0] + dred[1][1]) + (dred[1][2] + dred[1][3]);
        }
    }
    return t;
}

// ---- moments of one channel from its folded sums of (x - pv): n elements behind them, fp64 throughout, rounded once ------------
struct BnMoments { float mean, invstd; double var; };
__device__ __forceinline__ BnMoments bn_moments(double s1, double s2, double n, double pv, float eps) {
    BnMoments m;
    const double dm = s1 / n;
    m.var = s2 / n - dm * dm;
    if (m.var < 0.) m.var = 0.;
    m.mean = (float)(pv + dm);
    m.invstd = (float)(1.0 / sqrt(m.var + (double)eps));
    return m;
}
// ... and their publication: the caller guards this with its "I am the channel's one writer" predicate.  running_var receives the
// unbiased variance, num_batches_tracked is bumped by channel 0.
__device__ __forceinline__ void bn_publish(const BnMoments& m, double n, int c, float momentum, float* save_mean, float* save_invstd,
                                           float* running_mean, float* running_var, long long* num_batches_tracked) {
    save_mean[c] = m.mean;
    save_invstd[c] = m.invstd;
    if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * m.mean;
    if (running_var) {
        const float unbiased = (float)(n > 1. ? m.var * n / (n - 1.) : m.var);
        running_var[c] = (1.f - momentum) * running_var[c] + momentum * unbiased;
    }
    if (c == 0 && num_batches_tracked) *num_batches_tracked += 1;
}

// ---- walk over channel c of an fp32 (N, C, P) tensor, images [nb, ne), by a 256-thread block ---------------------------------
// float offset of the i-th float4 of channel c inside the images [nb, ne): 32-bit arithmetic, a shift when the plane size is a
// power of two.  (The loops used 64-bit i / P4 and i % P4 per 16 bytes: ~100 vector instructions per load, which is what made
// these HBM-bound kernels crawl beside the matrix-core kernels of the other stream - they compete for the same issue slots.)
struct Plane4Idx {
    unsigned p4; int sh; long stride, base;
    __device__ __forceinline__ long operator()(unsigned i) const {
        const unsigned n = sh >= 0 ? i >> sh : i / p4;
        return base + (long)n * stride + (long)(i - n * p4) * 4;
    }
};
__device__ __forceinline__ Plane4Idx plane4_idx(int nb, int C, int c, int P) {
    Plane4Idx u;
    u.p4 = (unsigned)(P >> 2);
    u.sh = (u.p4 & (u.p4 - 1)) == 0 ? __ffs((int)u.p4) - 1 : -1;
    u.stride = (long)C * P;
    u.base = ((long)nb * C + c) * P;
    return u;
}
// Calls f(x, dy) once per element, in 16-byte units when P % 4 == 0 and one float at a time otherwise, and stores what it returns
// to `out`.  Pass nullptr for dy (f then receives 0) or for out (a pure reduction: f's result, if any, is dropped): neither
// tensor is then touched, which is decided at compile time.  Each thread meets its elements in ascending order, so sums that f
// accumulates keep their order.
template <typename G, typename O, typename F>
__device__ __forceinline__ void bn_plane_walk(const float* __restrict__ x, G dy, O out, int nb, int ne, int C, int c, int P, F f) {
    constexpr bool two = !std::is_null_pointer_v<G>, store = !std::is_null_pointer_v<O>;
    if ((P & 3) == 0) {
        const unsigned cnt = (unsigned)(ne - nb) * (unsigned)(P >> 2);
        const Plane4Idx pi = plane4_idx(nb, C, c, P);
#pragma unroll 2
        for (unsigned i = threadIdx.x; i < cnt; i += 256) {
            const long off = pi(i);
            const f32x4 xv = *reinterpret_cast<const f32x4*>(x + off);
            f32x4 gv = 0.f;
            if constexpr (two) gv = *reinterpret_cast<const f32x4*>(dy + off);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if constexpr (store) gv[e] = f(xv[e], gv[e]); else f(xv[e], gv[e]);
            }
            if constexpr (store) *reinterpret_cast<f32x4*>(out + off) = gv;
        }
    } else {
        const long cnt = (long)(ne - nb) * P;
        for (long i = threadIdx.x; i < cnt; i += blockDim.x) {
            const long n = nb + i / P, q = i % P;
            const long off = (n * C + c) * (long)P + q;
            float g = 0.f;
            if constexpr (two) g = dy[off];
            if constexpr (store) out[off] = f(x[off], g); else f(x[off], g);
        }
    }
}

// ---- host: where the forward's statistics come from ---------------------------------------------------------------------------
// Training with ext_stats (the producing convolution's tile partials, or all-reduced sums): those, ext_nsplit of them.  Training
// without: `own_split` parts, written to the workspace by the layout's statistics kernel, which launch_stats(own_split) launches.
// Eval: the running statistics, which must then exist.  Returns 0 with *src filled, or the error code.  N == 0 returns 0 (after
// the workspace check, before anything is launched): the caller has nothing to do then.
struct BnStatsSrc { const float* partial; int nsplit; int ext; };
template <typename LaunchStats>
inline int bn_stats_source(void* ws, size_t ws_bytes, size_t ws_need, int N, int training, const float* ext_stats, int ext_nsplit,
                           const float* save_mean, const float* save_invstd, const float* running_mean, const float* running_var,
                           int own_split, LaunchStats launch_stats, BnStatsSrc* src) {
    if (ws_bytes < ws_need || !ws) return JVAE_EWORKSPACE;
    if (N == 0) return 0;
    src->partial = (const float*)ws;
    src->nsplit = 1;
    src->ext = training && ext_stats && ext_nsplit > 0;
    if (training && (!save_mean || !save_invstd)) return JVAE_EINVAL;
    if (src->ext) {
        src->partial = ext_stats;
        src->nsplit = ext_nsplit;
    } else if (training) {
        src->nsplit = own_split;
        launch_stats(own_split);
        JVAE_LAUNCH_CHECK();
    } else if (!running_mean || !running_var) {
        return JVAE_EINVAL;
    }
    return 0;
}
