// SSIM reconstruction OOD scores (Wang et al. 2004; Bergmann et al. 2018): the structural similarity of every
// image x[n] of a batch to each of its R reconstructions y[r, n], in ONE launch.
//
// Per plane (n, c) and draw r, with g the normalised 11-tap Gaussian of sigma 1.5 applied separably over the valid region:
//   mx = g*x, my = g*y, vx = g*x^2 - mx^2, vy = g*y^2 - my^2, cxy = g*xy - mx my,
//   cs = (2 cxy + C2) / (vx + vy + C2), l = (2 mx my + C1) / (mx^2 + my^2 + C1), map = l cs, C1 = 0.01^2, C2 = 0.03^2.
// The second moments are taken of x - a and y - a, a = the plane mean of x (fp64 sum in a fixed order, rounded once): they do not
// change under the shift and g*x^2 - mx^2 no longer cancels on a bright flat plane; the means get a added back.
//
// A workgroup of 256 threads owns one sample n and a chunk of its draws.  Per channel it sums the plane mean, then walks the plane
// in strips of S output rows (S + 10 staged rows, full width): the centred x strip is staged in LDS ONCE, filtered along the rows
// into two intermediates (g*x, g*x^2) and down the columns into the maps mx and vx, which stay in LDS; then every draw of the
// chunk stages its strip, forms its three row-filtered intermediates (g*y, g*y^2, g*xy) in LDS and each thread finishes the pixels
// it owns.  A chunk repeats the x side; a (r, n) entry lies in one workgroup whatever the chunking.
// The moments x^2, y^2 and xy go through ONE function (ssim_hmom, then ssim_vcol and ssim_central), every product and sum rounded
// as written (the file is built with -ffp-contract=off; the taps are explicit fmaf chains): a draw equal to x gives vy == cxy ==
// vx and my == mx bit for bit, so cs == l == 1.0f exactly.
// Scores: every thread adds its pixels in fp64 in ascending order, the workgroup folds the 256 partial sums by one fixed tree and
// thread 0 adds the strips and channels in ascending order; one division, one rounding to fp32.  No floating-point atomics: an
// entry's bits depend on nothing but its own planes.
#include "common.h"
#include "jvae_hip.h"
#include <math.h>

#define SSIM_BLOCK 256
#define SSIM_TAPS 11
#define SSIM_HALO 10
#define SSIM_MAX_W 128              // a strip is staged at full width
#define SSIM_MAX_H 32768
#define SSIM_MAX_CHUNK 32           // draws of one workgroup
#define SSIM_LDS_SOFT 40960         // bytes of a workgroup's strip buffers: four workgroups per CU ...
#define SSIM_LDS_HARD 64512         // ... unless that leaves a strip of fewer than SSIM_MIN_ROWS output rows
#define SSIM_MIN_ROWS 8
#define SSIM_TARGET_GROUPS 1024     // the draws are chunked so that about this many workgroups exist
#define SSIM_STATUS_X 1
#define SSIM_STATUS_Y 2

struct SsimTaps { float g[SSIM_TAPS]; };

static size_t ssim_lds_bytes(int S, int W) {
    const size_t Wo = W - SSIM_HALO, rows = S + SSIM_HALO;
    return sizeof(float) * (2 * rows * W + 5 * rows * Wo + 2 * (size_t)S * Wo);
}

// the output rows of a strip: the most that fit SSIM_LDS_SOFT, or SSIM_LDS_HARD where that is fewer than SSIM_MIN_ROWS
static int ssim_strip_rows(int H, int W) {
    const int Ho = H - SSIM_HALO;
    int S = 0;
    while (S < Ho && ssim_lds_bytes(S + 1, W) <= SSIM_LDS_SOFT) ++S;
    if (S < Ho && S < SSIM_MIN_ROWS)
        while (S < Ho && ssim_lds_bytes(S + 1, W) <= SSIM_LDS_HARD) ++S;
    return S;
}

__device__ __forceinline__ bool ssim_bad(float v) { return !(fabsf(v) < INFINITY); }

// g * p along a row or (stride ld) down a column: one fmaf chain, taps ascending
__device__ __forceinline__ float ssim_hmean(const float* p, const SsimTaps& t) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < SSIM_TAPS; ++k) acc = fmaf(t.g[k], p[k], acc);
    return acc;
}
// g * (p q) along a row: the product rounded on its own, then the same chain.  THE second-moment path of x^2, y^2 and xy.
__device__ __forceinline__ float ssim_hmom(const float* p, const float* q, const SsimTaps& t) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < SSIM_TAPS; ++k) acc = fmaf(t.g[k], __fmul_rn(p[k], q[k]), acc);
    return acc;
}
__device__ __forceinline__ float ssim_vcol(const float* h, int ld, const SsimTaps& t) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < SSIM_TAPS; ++k) acc = fmaf(t.g[k], h[k * ld], acc);
    return acc;
}
__device__ __forceinline__ float ssim_central(float e, float m1, float m2) { return __fsub_rn(e, __fmul_rn(m1, m2)); }

// the sums of a and b over the workgroup -> thread 0 (one fixed tree: lanes by halving, then the four waves in ascending order)
__device__ __forceinline__ void ssim_fold(double& a, double& b, double* s_red) {
    for (int off = 32; off; off >>= 1) {
        a += __shfl_down(a, off, 64);
        b += __shfl_down(b, off, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_red[2 * wave] = a;
        s_red[2 * wave + 1] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = ((s_red[0] + s_red[2]) + s_red[4]) + s_red[6];
        b = ((s_red[1] + s_red[3]) + s_red[5]) + s_red[7];
    }
    __syncthreads();                                            // s_red is free again
}

__global__ __launch_bounds__(SSIM_BLOCK) void ssim_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                          float* __restrict__ ssim, float* __restrict__ cs, float* map, long N, long R,
                                                          int C, int H, int W, int S, int RC, int chunks, SsimTaps taps, int* status) {
    extern __shared__ __attribute__((aligned(16))) float ssim_lds[];
    __shared__ double s_acc[2 * SSIM_MAX_CHUNK];
    __shared__ double s_red[8];
    __shared__ int s_ybad[SSIM_MAX_CHUNK];
    __shared__ int s_xbad;
    __shared__ float s_a;
    const int tid = threadIdx.x;
    const long n = blockIdx.x / chunks;
    const long r0 = (long)(blockIdx.x % chunks) * RC;
    const int rn = R - r0 < RC ? (int)(R - r0) : RC;
    const int Wo = W - SSIM_HALO, Ho = H - SSIM_HALO, max_rows = S + SSIM_HALO, plane = H * W;
    float* xs = ssim_lds;                                       // (S + 10, W): the centred strip of x
    float* ys = xs + max_rows * W;                              // the same of the draw
    float* hx = ys + max_rows * W;                              // (S + 10, Wo) each: g*x, g*x^2, g*y, g*y^2, g*xy along the rows
    float* hxx = hx + max_rows * Wo;
    float* hy = hxx + max_rows * Wo;
    float* hyy = hy + max_rows * Wo;
    float* hxy = hyy + max_rows * Wo;
    float* mux = hxy + max_rows * Wo;                           // (S, Wo) each: the centred local mean and the local variance of x
    float* vxm = mux + S * Wo;
    const float C1 = 1e-4f, C2 = 9e-4f;

    if (tid < 2 * SSIM_MAX_CHUNK) s_acc[tid] = 0.;
    if (tid < SSIM_MAX_CHUNK) s_ybad[tid] = 0;
    if (tid == 0) s_xbad = 0;
    __syncthreads();

    for (int c = 0; c < C; ++c) {
        const float* xp = x + ((size_t)n * C + c) * plane;
        // the centring constant: the plane mean of x
        double part = 0., none = 0.;
        int bad = 0;
        for (int i = tid; i < plane; i += SSIM_BLOCK) {
            const float v = xp[i];
            bad |= ssim_bad(v);
            part += (double)v;
        }
        if (bad) atomicOr(&s_xbad, 1);
        ssim_fold(part, none, s_red);
        if (tid == 0) s_a = (float)(part / (double)plane);
        __syncthreads();
        const float a = s_a;

        for (int s0 = 0; s0 < Ho; s0 += S) {
            const int sh = Ho - s0 < S ? Ho - s0 : S, rows = sh + SSIM_HALO;
            // the x side of the strip, once for every draw of the chunk
            for (int i = tid; i < rows * W; i += SSIM_BLOCK) xs[i] = __fsub_rn(xp[s0 * W + i], a);
            __syncthreads();
            for (int i = tid; i < rows * Wo; i += SSIM_BLOCK) {
                const int row = i / Wo;
                const float* p = xs + row * W + (i - row * Wo);
                hx[i] = ssim_hmean(p, taps);
                hxx[i] = ssim_hmom(p, p, taps);
            }
            __syncthreads();
            for (int i = tid; i < sh * Wo; i += SSIM_BLOCK) {
                const float m = ssim_vcol(hx + i, Wo, taps);
                mux[i] = m;
                vxm[i] = ssim_central(ssim_vcol(hxx + i, Wo, taps), m, m);
            }
            // (mux and vxm are read back by the thread that wrote them)

            for (int r = 0; r < rn; ++r) {
                const size_t entry = (size_t)(r0 + r) * N + n;
                const float* yp = y + (entry * C + c) * plane + s0 * W;
                bad = 0;
                for (int i = tid; i < rows * W; i += SSIM_BLOCK) {
                    const float v = yp[i];
                    bad |= ssim_bad(v);
                    ys[i] = __fsub_rn(v, a);
                }
                if (bad) atomicOr(&s_ybad[r], 1);
                __syncthreads();
                for (int i = tid; i < rows * Wo; i += SSIM_BLOCK) {
                    const int row = i / Wo, o = row * W + (i - row * Wo);
                    const float *p = xs + o, *q = ys + o;
                    hy[i] = ssim_hmean(q, taps);
                    hyy[i] = ssim_hmom(q, q, taps);
                    hxy[i] = ssim_hmom(p, q, taps);
                }
                __syncthreads();
                double sum_s = 0., sum_c = 0.;
                float* mp = map ? map + entry * ((size_t)Ho * Wo) + (size_t)s0 * Wo : nullptr;
                for (int i = tid; i < sh * Wo; i += SSIM_BLOCK) {
                    const float mx = mux[i], vx = vxm[i];
                    const float my = ssim_vcol(hy + i, Wo, taps);
                    const float vy = ssim_central(ssim_vcol(hyy + i, Wo, taps), my, my);
                    const float cxy = ssim_central(ssim_vcol(hxy + i, Wo, taps), mx, my);
                    const float csv = __fadd_rn(__fadd_rn(cxy, cxy), C2) / __fadd_rn(__fadd_rn(vx, vy), C2);
                    const float fx = __fadd_rn(a, mx), fy = __fadd_rn(a, my);            // the means, uncentred again
                    const float pxy = __fmul_rn(fx, fy), pxx = __fmul_rn(fx, fx), pyy = __fmul_rn(fy, fy);
                    const float lum = __fadd_rn(__fadd_rn(pxy, pxy), C1) / __fadd_rn(__fadd_rn(pxx, pyy), C1);
                    const float v = __fmul_rn(lum, csv);
                    sum_s += (double)v;
                    sum_c += (double)csv;
                    if (mp) {                                   // the channel mean: the same thread owns the pixel in every channel
                        float t = c ? __fadd_rn(mp[i], v) : v;
                        if (c == C - 1) t = t / (float)C;
                        mp[i] = t;
                    }
                }
                ssim_fold(sum_s, sum_c, s_red);                 // its barriers also free ys and the draw's intermediates
                if (tid == 0) {
                    s_acc[2 * r] += sum_s;
                    s_acc[2 * r + 1] += sum_c;
                }
            }
        }
    }
    __syncthreads();
    const int xbad = s_xbad;
    if (tid < rn) {
        const int flags = (xbad ? SSIM_STATUS_X : 0) | (s_ybad[tid] ? SSIM_STATUS_Y : 0);
        const double count = (double)C * (double)Ho * (double)Wo;
        const size_t entry = (size_t)(r0 + tid) * N + n;
        ssim[entry] = flags ? NAN : (float)(s_acc[2 * tid] / count);
        cs[entry] = flags ? NAN : (float)(s_acc[2 * tid + 1] / count);
        if (flags) atomicOr(status, flags);
    }
    if (map)
        for (int r = 0; r < rn; ++r)
            if (xbad || s_ybad[r]) {                            // uniform over the workgroup
                float* mp = map + ((size_t)(r0 + r) * N + n) * ((size_t)Ho * Wo);
                for (int i = tid; i < Ho * Wo; i += SSIM_BLOCK) mp[i] = NAN;
            }
}

extern "C" int jvae_ssim_f32(const float* x, const float* y, long N, long R, int C, int H, int W, float* ssim, float* cs, float* map,
                             int* status, void* stream) {
    if (N < 0 || R < 0) return JVAE_EINVAL;
    if (C < 1 || H < SSIM_TAPS || W < SSIM_TAPS || W > SSIM_MAX_W || H > SSIM_MAX_H || N >= (1L << 31) || R >= (1L << 31))
        return JVAE_ENOTSUP;
    // the draws of a workgroup: about SSIM_TARGET_GROUPS workgroups, at most SSIM_MAX_CHUNK draws each, evenly
    long rc = N * R / SSIM_TARGET_GROUPS;
    rc = rc < 1 ? 1 : (rc > SSIM_MAX_CHUNK ? SSIM_MAX_CHUNK : rc);
    if (rc > R && R > 0) rc = R;
    const long chunks = R ? (R + rc - 1) / rc : 0;
    if (N * chunks >= (1L << 31)) return JVAE_ENOTSUP;
    if (N == 0 || R == 0) return 0;
    if (!x || !y || !ssim || !cs || !status) return JVAE_EINVAL;
    rc = (R + chunks - 1) / chunks;
    static SsimTaps taps;
    static bool taps_set = false;
    if (!taps_set) {
        double g[SSIM_TAPS], sum = 0.;
        for (int k = 0; k < SSIM_TAPS; ++k) {
            const double d = k - SSIM_TAPS / 2;
            g[k] = exp(-d * d / (2. * 1.5 * 1.5));
            sum += g[k];
        }
        for (int k = 0; k < SSIM_TAPS; ++k) taps.g[k] = (float)(g[k] / sum);
        taps_set = true;
    }
    const int S = ssim_strip_rows(H, W);
    ssim_kernel<<<(unsigned)(N * chunks), SSIM_BLOCK, ssim_lds_bytes(S, W), (hipStream_t)stream>>>(x, y, ssim, cs, map, N, R, C, H, W, S,
                                                                                                   (int)rc, (int)chunks, taps, status);
    JVAE_LAUNCH_CHECK();
    return 0;
}

// the strip height of a shape, for the tests and the bench (0: the shape is refused)
extern "C" int jvae_ssim_strip_rows(int H, int W) {
    if (H < SSIM_TAPS || W < SSIM_TAPS || W > SSIM_MAX_W || H > SSIM_MAX_H) return 0;
    return ssim_strip_rows(H, W);
}
