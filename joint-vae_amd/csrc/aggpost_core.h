// The kernels of the aggregate posterior that more than one file launches (csrc/aggpost.hip: a stored bank; csrc/tcvae.hip: the
// batch's own posteriors as the bank).  The arithmetic is described at the head of aggpost.hip and in DESIGN.md section 7u; every
// file that includes this header is built with -ffp-contract=off, so that a pair (query, row) gives the same bits wherever it is met.
#pragma once
#include "common.h"
#include <math.h>

#define AGP_MAX_K 1024
#define AGP_MAX_BANK (1L << 24)
#define AGP_PART 1024          // bank rows of a piece
#define AGP_QT 64              // queries of a workgroup
#define AGP_BLOCK 256
#define AGP_WAVES 4
#define AGP_TILE 64            // joint launch: bank rows of a staged tile (16 per wave)
#define AGP_ROWS (AGP_TILE / AGP_WAVES)
#define AGP_KC 32              // joint launch: coordinates of a staged chunk
#define AGP_DTILE 256          // marginal launch: bank rows of a staged tile (64 per wave)
#define AGP_DROWS (AGP_DTILE / AGP_WAVES)
#define AGP_DG 8               // marginal launch: rows whose terms are formed together
#define AGP_KD 8               // marginal launch: coordinates of a workgroup
#define AGP_STACK 15           // levels of the pairwise sum over the pieces
#define AGP_STATUS_BANK 1
#define AGP_STATUS_QUERY 2
#define AGP_STATUS_EMPTY 4
#define AGP_KK (-0.72134752044448170368f)      // -log2(e) / 2

static_assert(AGP_PART % AGP_DTILE == 0 && AGP_DTILE % AGP_TILE == 0, "tiles divide the piece");
static_assert((AGP_MAX_BANK / AGP_PART) < (1L << AGP_STACK), "the merge's counter holds every piece");

__device__ __forceinline__ float agp_exp2(float x) { return __builtin_amdgcn_exp2f(x); }      // v_exp_f32
__device__ __forceinline__ bool agp_finite(float x) { return fabsf(x) < INFINITY; }

static inline long agp_padded(long N) { return (N + AGP_TILE - 1) / AGP_TILE * AGP_TILE; }
static inline int agp_pieces(long N) { return (int)((N + AGP_PART - 1) / AGP_PART); }

// the stored inverse variance of a row: fp32(exp(-(double)lv))
__device__ __forceinline__ float agp_w(float lv) { return (float)exp(-(double)lv); }

// one thread per row of the padded bank
static __global__ __launch_bounds__(AGP_BLOCK) void agp_prepare_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                                                                       float* __restrict__ muT, float* __restrict__ wT,
                                                                       float* __restrict__ lvT, float* __restrict__ c, long N, long Np,
                                                                       int K) {
    const long n = (long)blockIdx.x * AGP_BLOCK + threadIdx.x;
    if (n >= Np) return;
    double sum = 0.;
    for (int k = 0; k < K; ++k) {
        const bool in = n < N;
        const float m = in ? mu[(size_t)n * K + k] : 0.f, l = in ? lv[(size_t)n * K + k] : 0.f;
        sum += (double)l;
        muT[(size_t)k * Np + n] = m;
        wT[(size_t)k * Np + n] = in ? agp_w(l) : 0.f;
        lvT[(size_t)k * Np + n] = l;
    }
    c[n] = (float)sum;
}

// (a, s) <- (a, s) + (at, st): the fold of aggpost.hip's head.  An empty side has a = +inf and s = 0 and leaves the other as it is.
__device__ __forceinline__ void agp_fold(float& a, float& s, float at, float st) {
    const float an = fminf(a, at), as = an < INFINITY ? an : 0.f;
    const float left = s * agp_exp2(AGP_KK * (a - as)), right = st * agp_exp2(AGP_KK * (at - as));
    s = left + right;
    a = an;
}

// ws pair[(piece, q)] = (a, s) of the piece, cnt[(piece, q)] = rows of the query's group in it.  STORE: every Q of the launch is
// kept as well, qall[q][row] with a row stride of Np floats, +inf for a masked row (another group, padding), and the launch does
// not look at what it stages: its caller has no status word (`status` may be null), a non-finite operand shows in its outputs.  PART: the rows of a
// piece, a multiple of AGP_TILE (the bank's AGP_PART; a training batch is cut finer, so that a small batch fills the device).
template <bool COND, bool STORE, int PART = AGP_PART>
__global__ __launch_bounds__(AGP_BLOCK) void agp_joint_kernel(const float* __restrict__ z, const int* __restrict__ zgroup,
                                                              const float* __restrict__ muT, const float* __restrict__ wT,
                                                              const float* __restrict__ c, const int* __restrict__ group,
                                                              float2* __restrict__ pair, int* __restrict__ cnt, long M, long N,
                                                              long Np, int K, int* status, float* __restrict__ qall) {
    __shared__ __attribute__((aligned(16))) float mt[AGP_KC][AGP_TILE];
    __shared__ __attribute__((aligned(16))) float wt[AGP_KC][AGP_TILE];
    __shared__ float zt[AGP_KC][AGP_QT + 1];           // + 1: the transposing store walks k at a stride of 65 words
    __shared__ float ct[AGP_TILE];
    __shared__ int gt[AGP_TILE];
    __shared__ float xa[AGP_WAVES][AGP_QT], xs[AGP_WAVES][AGP_QT];
    __shared__ int xc[AGP_WAVES][AGP_QT];
    static_assert(PART % AGP_TILE == 0, "tiles divide the piece");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long q0 = (long)blockIdx.x * AGP_QT, q = q0 + lane;
    const long base = (long)blockIdx.y * PART, end = base + PART < N ? base + PART : N;
    const int qg = COND ? (q < M ? max(zgroup[q], -1) : -1) : 0;      // bank groups are >= 0, padding rows -2
    const bool look = !STORE && blockIdx.x == 0;       // the first query tile looks at the operands it stages
    bool bad = false;
    float a = INFINITY, s = 0.f;
    int count = 0;

    for (long t0 = base; t0 < end; t0 += AGP_TILE) {
        float acc[AGP_ROWS];
        for (int kc = 0; kc < K; kc += AGP_KC) {
            const int kn = K - kc < AGP_KC ? K - kc : AGP_KC;
            __syncthreads();                           // the tiles are free
            for (int i = tid; i < kn * AGP_TILE; i += AGP_BLOCK) {
                const int kk = i >> 6, r = i & 63;
                const size_t at = (size_t)(kc + kk) * Np + t0 + r;       // t0 + r < Np: Np is a multiple of the tile
                const float m = muT[at], w = wT[at];
                mt[kk][r] = m;
                wt[kk][r] = w;
                if (look) bad |= !agp_finite(m) || !agp_finite(w);
            }
            for (int i = tid; i < kn * AGP_QT; i += AGP_BLOCK) {
                const int ql = i / kn, kk = i - ql * kn;
                zt[kk][ql] = q0 + ql < M ? z[(size_t)(q0 + ql) * K + kc + kk] : 0.f;
            }
            if (kc == 0 && tid < AGP_TILE) {
                const long n = t0 + tid;
                const float cn = c[n];
                ct[tid] = cn;
                gt[tid] = n < N ? (COND ? group[n] : 0) : -2;
                if (look) bad |= !agp_finite(cn);
            }
            __syncthreads();
            if (kc == 0) {
#pragma unroll
                for (int r = 0; r < AGP_ROWS; ++r) acc[r] = ct[wave * AGP_ROWS + r];
            }
#pragma unroll 2
            for (int kk = 0; kk < kn; ++kk) {
                const float zk = zt[kk][lane];
#pragma unroll
                for (int j = 0; j < AGP_ROWS / 4; ++j) {
                    const f32x4 m4 = *reinterpret_cast<const f32x4*>(&mt[kk][wave * AGP_ROWS + 4 * j]);
                    const f32x4 w4 = *reinterpret_cast<const f32x4*>(&wt[kk][wave * AGP_ROWS + 4 * j]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float d = zk - m4[e];
                        acc[4 * j + e] = fmaf(d * d, w4[e], acc[4 * j + e]);
                    }
                }
            }
        }
        float at = INFINITY;
#pragma unroll
        for (int r = 0; r < AGP_ROWS; ++r) {
            const bool in = gt[wave * AGP_ROWS + r] == qg;
            acc[r] = in ? acc[r] : INFINITY;
            count += in;
            at = fminf(at, acc[r]);
        }
        if (STORE && q < M) {                          // 16 floats of one query: t0 + 16 wave + 15 < Np, 64-byte aligned
            f32x4* o = reinterpret_cast<f32x4*>(qall + (size_t)q * Np + t0 + wave * AGP_ROWS);
#pragma unroll
            for (int j = 0; j < AGP_ROWS / 4; ++j) {
                f32x4 v;
                v[0] = acc[4 * j]; v[1] = acc[4 * j + 1]; v[2] = acc[4 * j + 2]; v[3] = acc[4 * j + 3];
                o[j] = v;
            }
        }
        const float as = at < INFINITY ? at : 0.f;
        float e[AGP_ROWS];
#pragma unroll
        for (int r = 0; r < AGP_ROWS; ++r) e[r] = agp_exp2(AGP_KK * (acc[r] - as));
#pragma unroll
        for (int r = 0; r < AGP_ROWS; r += 4) e[r] = (e[r] + e[r + 1]) + (e[r + 2] + e[r + 3]);
        const float st = (e[0] + e[4]) + (e[8] + e[12]);
        agp_fold(a, s, at, st);
    }
    if (!STORE && bad) atomicOr(status, AGP_STATUS_BANK);
    xa[wave][lane] = a;
    xs[wave][lane] = s;
    xc[wave][lane] = count;
    __syncthreads();
    if (wave == 0 && q < M) {
        float a0 = xa[0][lane], s0 = xs[0][lane], a2 = xa[2][lane], s2 = xs[2][lane];
        agp_fold(a0, s0, xa[1][lane], xs[1][lane]);
        agp_fold(a2, s2, xa[3][lane], xs[3][lane]);
        agp_fold(a0, s0, a2, s2);
        const size_t o = (size_t)blockIdx.y * M + q;
        pair[o] = make_float2(a0, s0);
        cnt[o] = (xc[0][lane] + xc[1][lane]) + (xc[2][lane] + xc[3][lane]);
    }
}

// ws pair[((piece, k), q)] = (a, s) of coordinate k in the piece; blockIdx.z = the chunk of AGP_KD coordinates
template <bool COND>
__global__ __launch_bounds__(AGP_BLOCK) void agp_dims_kernel(const float* __restrict__ z, const int* __restrict__ zgroup,
                                                             const float* __restrict__ muT, const float* __restrict__ wT,
                                                             const float* __restrict__ lvT, const int* __restrict__ group,
                                                             float2* __restrict__ pair, long M, long N, long Np, int K) {
    __shared__ __attribute__((aligned(16))) float mt[AGP_KD][AGP_DTILE];
    __shared__ __attribute__((aligned(16))) float wt[AGP_KD][AGP_DTILE];
    __shared__ __attribute__((aligned(16))) float lt[AGP_KD][AGP_DTILE];
    __shared__ __attribute__((aligned(16))) int gt[AGP_DTILE];
    __shared__ float xa[AGP_WAVES][AGP_KD][AGP_QT], xs[AGP_WAVES][AGP_KD][AGP_QT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long q = (long)blockIdx.x * AGP_QT + lane;
    const long base = (long)blockIdx.y * AGP_PART, end = base + AGP_PART < N ? base + AGP_PART : N;
    const int k0 = blockIdx.z * AGP_KD;
    const int qg = COND ? (q < M ? max(zgroup[q], -1) : -1) : 0;      // bank groups are >= 0, padding rows -2
    float zk[AGP_KD], a[AGP_KD], s[AGP_KD];
#pragma unroll
    for (int kd = 0; kd < AGP_KD; ++kd) {
        zk[kd] = q < M && k0 + kd < K ? z[(size_t)q * K + k0 + kd] : 0.f;
        a[kd] = INFINITY;
        s[kd] = 0.f;
    }

    for (long t0 = base; t0 < end; t0 += AGP_DTILE) {
        __syncthreads();                               // the tiles are free
        for (int i = tid; i < AGP_KD * AGP_DTILE; i += AGP_BLOCK) {
            const int kd = i / AGP_DTILE, r = i % AGP_DTILE;
            const bool in = k0 + kd < K && t0 + r < Np;
            const size_t at = (size_t)(k0 + kd) * Np + t0 + r;
            mt[kd][r] = in ? muT[at] : 0.f;
            wt[kd][r] = in ? wT[at] : 0.f;
            lt[kd][r] = in ? lvT[at] : 0.f;
        }
        {
            const long n = t0 + tid;                   // AGP_DTILE == AGP_BLOCK
            gt[tid] = n < N ? (COND ? group[n] : 0) : -2;
        }
        __syncthreads();
#pragma unroll 1
        for (int g = 0; g < AGP_DROWS; g += AGP_DG) {
            const int r0 = wave * AGP_DROWS + g;
            bool in[AGP_DG];
#pragma unroll
            for (int r = 0; r < AGP_DG; ++r) in[r] = gt[r0 + r] == qg;
#pragma unroll
            for (int kd = 0; kd < AGP_KD; ++kd) {
                float qv[AGP_DG];
                float at = INFINITY;
#pragma unroll
                for (int j = 0; j < AGP_DG / 4; ++j) {
                    const f32x4 m4 = *reinterpret_cast<const f32x4*>(&mt[kd][r0 + 4 * j]);
                    const f32x4 w4 = *reinterpret_cast<const f32x4*>(&wt[kd][r0 + 4 * j]);
                    const f32x4 l4 = *reinterpret_cast<const f32x4*>(&lt[kd][r0 + 4 * j]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float d = zk[kd] - m4[e];
                        const float v = in[4 * j + e] ? fmaf(d * d, w4[e], l4[e]) : INFINITY;
                        qv[4 * j + e] = v;
                        at = fminf(at, v);
                    }
                }
                const float as = at < INFINITY ? at : 0.f;
#pragma unroll
                for (int r = 0; r < AGP_DG; ++r) qv[r] = agp_exp2(AGP_KK * (qv[r] - as));
                const float st = ((qv[0] + qv[1]) + (qv[2] + qv[3])) + ((qv[4] + qv[5]) + (qv[6] + qv[7]));
                agp_fold(a[kd], s[kd], at, st);
            }
        }
    }
#pragma unroll
    for (int kd = 0; kd < AGP_KD; ++kd) {
        xa[wave][kd][lane] = a[kd];
        xs[wave][kd][lane] = s[kd];
    }
    __syncthreads();
    if (q >= M) return;
#pragma unroll
    for (int j = 0; j < AGP_KD / AGP_WAVES; ++j) {     // wave v merges coordinates v and v + 4
        const int kd = wave + AGP_WAVES * j;
        if (k0 + kd >= K) continue;
        float a0 = xa[0][kd][lane], s0 = xs[0][kd][lane], a2 = xa[2][kd][lane], s2 = xs[2][kd][lane];
        agp_fold(a0, s0, xa[1][kd][lane], xs[1][kd][lane]);
        agp_fold(a2, s2, xa[3][kd][lane], xs[3][kd][lane]);
        agp_fold(a0, s0, a2, s2);
        pair[((size_t)blockIdx.y * K + k0 + kd) * M + q] = make_float2(a0, s0);
    }
}
