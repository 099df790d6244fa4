// Density-of-states OOD scores (Morningstar et al. 2021; the typicality test of Nalisnick et al. 2019): a
// Gaussian kernel density estimate of S statistics over a bank of M training samples, evaluated at N queries in ONE scoring launch
// and one merge launch - S marginal log-densities, their sum, the log-density of the product kernel and S typicality rows.
//
// Fit.  The moments of every bank row are fp64 sums in a fixed order that hangs on M alone: a slab of DOSE_SLAB values is dealt to
// the 256 threads of a workgroup in strides (a thread adds its values ascending), the 64 partials of a wave meet in a butterfly,
// the four waves are added in sequence and a fold adds the slabs ascending - first the mean, then the centred squares.  The bank
// is centred and scaled in fp64, z = (B - c) / h(1), and rounded ONCE.  A non-finite element sets bit s of the status word, a
// row without spread bit 8 + s (integer OR; there are no floating-point atomics anywhere in this file).
//
// Scores.  The bank is cut into pieces of DOSE_PART values whatever N and the grid are.  A workgroup owns 64 queries (one per
// lane) and ONE piece, whose z tile lies in LDS (S x DOSE_PART floats, read as broadcast 16-byte words); each of its four waves
// takes a quarter of the tile for the same 64 queries.  The query is centred and scaled in fp64 and rounded once, t = fp32((T - c)
// / h(1)); differences, squares and exponentials are fp32.  Pass A finds, per statistic, the smallest |t - z| of the piece and the
// smallest sum of squares (a minimum is exact and has no order); the four waves exchange them through LDS.  Pass B adds
// 2^(k (d^2 - min d^2)) with k = -log2(e) / 2: the difference of the squares is taken BEFORE the product (k d^2 itself is only
// known to 2^-24 of its size, thousands of units for a far query), so the largest term of every sum is exactly 1, no exponent
// is positive and nothing underflows however far the query is; a = fp32(k min d^2) is the piece's largest exponent.  The sums
// are pairwise: 16 values as a tree of depth 4, four of those in sequence, four of those in sequence, the four waves as a tree -
// at most 12 roundings on the way of a term.  The S + 1 running (exponent, sum) pairs of a query stay in registers.  The joint
// kernel's bandwidth is h(S) = h(1) / r with ONE ratio r for all rows, so its exponent is k r^2 sum_s d_s^2 (s ascending, an fmaf
// chain) on the same differences.
// The merge launch takes the (a, sum) pairs of the pieces of a query: A = max a, the sums scaled by 2^(a - A) and added pairwise
// in the pieces' order, log density = (A + log2 sum) ln 2 - log normaliser in fp64, rounded once.  A padded element (past M) is
// z = +inf: its term is exactly +0 and it is in no minimum.  A finite query whose square overflows fp32 is given -inf and
// flagged like an infinite one.
#include "common.h"
#include "jvae_hip.h"
#include <math.h>

#define DOSE_MAX_STATS 8
#define DOSE_MAX_BANK (1L << 24)
#define DOSE_PART 1024         // bank values of a piece = of a scoring workgroup's LDS tile (per statistic)
#define DOSE_QT 64             // queries of a workgroup
#define DOSE_BLOCK 256
#define DOSE_WAVES 4
#define DOSE_WPART (DOSE_PART / DOSE_WAVES)
#define DOSE_SLAB 4096         // bank values of a slab of the moment sums
#define DOSE_STACK 16          // levels of the pairwise sum over the pieces: 2^16 pieces
#define DOSE_STATUS_QUERY 0x10000
#define DOSE_K (-0.72134752044448170368)      // -log2(e) / 2

// part[(s, slab)] = the sum over the slab of b (centre == nullptr) or of (b - centre[s])^2
__global__ __launch_bounds__(DOSE_BLOCK) void dose_rowsum_kernel(const float* __restrict__ bank, const double* __restrict__ centre,
                                                                 double* __restrict__ part, long M, int* status) {
    __shared__ double red[DOSE_BLOCK / 64];
    const int s = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long b0 = (long)blockIdx.x * DOSE_SLAB, b1 = b0 + DOSE_SLAB < M ? b0 + DOSE_SLAB : M;
    const float* row = bank + (size_t)s * M;
    const double c = centre ? centre[s] : 0.;
    double acc = 0.;
    bool finite = true;
    for (long i = b0 + threadIdx.x; i < b1; i += DOSE_BLOCK) {
        const float b = row[i];
        finite &= fabsf(b) < INFINITY;
        const double d = (double)b - c;
        acc = centre ? fma(d, d, acc) : acc + d;
    }
    if (!finite && !centre) atomicOr(status, 1 << s);
    acc = wave_sum64(acc);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = red[0];
        for (int w = 1; w < DOSE_BLOCK / 64; ++w) t += red[w];
        part[(size_t)s * gridDim.x + blockIdx.x] = t;
    }
}

// mode 0: centre[s] = the slabs' sums added ascending / M.  mode 1: sigma (ddof = 1), h(1), h(S) and the S + 1 log-normalisers
__global__ __launch_bounds__(64) void dose_fold_kernel(const double* __restrict__ part, int slabs, long M, int S, int mode,
                                                       double bandwidth, double scott1, double scottS, double* __restrict__ centre,
                                                       double* __restrict__ sigma, double* __restrict__ h1, double* __restrict__ hS,
                                                       double* __restrict__ lognorm, int* status) {
    __shared__ double lh[DOSE_MAX_STATS];
    const int s = threadIdx.x;
    const double log2pi = 1.8378770664093454836;
    if (s < S) {
        double acc = 0.;
        for (int i = 0; i < slabs; ++i) acc += part[(size_t)s * slabs + i];
        if (mode == 0) {
            centre[s] = acc / (double)M;
        } else {
            const double sg = sqrt(acc / (double)(M - 1));
            if (!(sg > 0.) || !(sg < INFINITY)) atomicOr(status, 1 << (8 + s));
            sigma[s] = sg;
            h1[s] = bandwidth * sg * scott1;
            hS[s] = bandwidth * sg * scottS;
            lognorm[s] = log((double)M * h1[s]) + 0.5 * log2pi;
            lh[s] = log(hS[s]);
        }
    }
    __syncthreads();
    if (mode == 1 && s == 0) {
        double j = log((double)M);
        for (int i = 0; i < S; ++i) j += lh[i];
        lognorm[S] = j + 0.5 * S * log2pi;
    }
}

__global__ __launch_bounds__(DOSE_BLOCK) void dose_z_kernel(const float* __restrict__ bank, const double* __restrict__ centre,
                                                            const double* __restrict__ h1, float* __restrict__ z, long M) {
    const int s = blockIdx.y;
    const long i = (long)blockIdx.x * DOSE_BLOCK + threadIdx.x;
    if (i < M) z[(size_t)s * M + i] = (float)(((double)bank[(size_t)s * M + i] - centre[s]) / h1[s]);
}

__device__ __forceinline__ float dose_exp2(float x) { return __builtin_amdgcn_exp2f(x); }      // v_exp_f32

template <int S>
__global__ __launch_bounds__(DOSE_BLOCK) void dose_score_kernel(const float* __restrict__ stats, const float* __restrict__ z,
                                                                const double* __restrict__ centre, const double* __restrict__ h1,
                                                                float2* __restrict__ ws, long N, long M, float kj) {
    constexpr int R = S + 1;                           // the marginals and the joint row
    __shared__ __attribute__((aligned(16))) float zt[S * DOSE_PART];
    __shared__ float xch[DOSE_WAVES][R][DOSE_QT];      // pass A: the waves' minima; pass B: their sums
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long q = (long)blockIdx.x * DOSE_QT + lane, base = (long)blockIdx.y * DOSE_PART;
    const float k = (float)DOSE_K;

#pragma unroll
    for (int s = 0; s < S; ++s)
        for (int i = threadIdx.x; i < DOSE_PART; i += DOSE_BLOCK)
            zt[s * DOSE_PART + i] = base + i < M ? z[(size_t)s * M + base + i] : INFINITY;
    float t[S];
#pragma unroll
    for (int s = 0; s < S; ++s) t[s] = q < N ? (float)(((double)stats[(size_t)s * N + q] - centre[s]) / h1[s]) : 0.f;
    __syncthreads();

    const float* zw = zt + wave * DOSE_WPART;
    float mn[R];
#pragma unroll
    for (int r = 0; r < R; ++r) mn[r] = INFINITY;
#pragma unroll 2
    for (int j = 0; j < DOSE_WPART; j += 4) {
        f32x4 zv[S];
#pragma unroll
        for (int s = 0; s < S; ++s) zv[s] = *reinterpret_cast<const f32x4*>(zw + s * DOSE_PART + j);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float jd = 0.f;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const float d = t[s] - zv[s][e];
                mn[s] = fminf(mn[s], fabsf(d));
                jd = s ? fmaf(d, d, jd) : d * d;
            }
            mn[S] = fminf(mn[S], jd);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) xch[wave][r][lane] = mn[r];
    __syncthreads();
    float m2[R];                                       // the piece's smallest square (sum of squares), row by row
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float m = fminf(fminf(xch[0][r][lane], xch[1][r][lane]), fminf(xch[2][r][lane], xch[3][r][lane]));
        m2[r] = r < S ? m * m : m;
    }
    __syncthreads();                                   // xch is written again below

    float s3[R];
#pragma unroll 1
    for (int i3 = 0; i3 < 4; ++i3) {
        float s2[R];
#pragma unroll 1
        for (int i2 = 0; i2 < 4; ++i2) {
            const float* zp = zw + (i3 * 4 + i2) * 16;
            float g[4][R];
#pragma unroll
            for (int gi = 0; gi < 4; ++gi) {
                f32x4 zv[S];
#pragma unroll
                for (int s = 0; s < S; ++s) zv[s] = *reinterpret_cast<const f32x4*>(zp + s * DOSE_PART + 4 * gi);
                float e[4][R];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    float jd = 0.f;
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        const float d = t[s] - zv[s][c];
                        const float sq = d * d;
                        jd = s ? fmaf(d, d, jd) : sq;
                        e[c][s] = dose_exp2(k * (sq - m2[s]));
                    }
                    e[c][S] = dose_exp2(kj * (jd - m2[S]));
                }
#pragma unroll
                for (int r = 0; r < R; ++r) g[gi][r] = (e[0][r] + e[1][r]) + (e[2][r] + e[3][r]);
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float t16 = (g[0][r] + g[1][r]) + (g[2][r] + g[3][r]);
                s2[r] = i2 ? s2[r] + t16 : t16;
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) s3[r] = i3 ? s3[r] + s2[r] : s2[r];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) xch[wave][r][lane] = s3[r];
    __syncthreads();
    if (q >= N) return;
#pragma unroll
    for (int r = 0; r < R; ++r)
        if ((r & (DOSE_WAVES - 1)) == wave) {
            const float tot = (xch[0][r][lane] + xch[1][r][lane]) + (xch[2][r][lane] + xch[3][r][lane]);
            ws[((size_t)blockIdx.y * R + r) * N + q] = make_float2((r < S ? k : kj) * m2[r], tot);
        }
}

// out (2S + 2, N): the marginals, their sum, the joint row, the typicality rows - one thread per query
__global__ __launch_bounds__(DOSE_BLOCK) void dose_merge_kernel(const float* __restrict__ stats, const float2* __restrict__ ws,
                                                                const double* __restrict__ centre, const double* __restrict__ sigma,
                                                                const double* __restrict__ lognorm, float* __restrict__ out, long N,
                                                                int S, int pieces, int* status) {
    const long q = (long)blockIdx.x * DOSE_BLOCK + threadIdx.x;
    if (q >= N) return;
    const int R = S + 1;
    const double ln2 = 0.69314718055994530942;
    bool any_nan = false, any_inf = false;
    double dose = 0.;
    for (int r = 0; r < R; ++r) {
        const float2* w = ws + (size_t)r * N + q;
        const size_t step = (size_t)R * N;
        float A = -INFINITY;
        for (int p = 0; p < pieces; ++p) A = fmaxf(A, w[p * step].x);
        float stack[DOSE_STACK];
#pragma unroll
        for (int l = 0; l < DOSE_STACK; ++l) stack[l] = 0.f;
        for (int p = 0; p < pieces; ++p) {
            const float2 v = w[p * step];
            float carry = v.y * exp2f(v.x - A);
            bool open = true;
#pragma unroll
            for (int l = 0; l < DOSE_STACK; ++l) {     // a binary counter: level l holds the sum of 2^l pieces
                const bool full = (p >> l) & 1;
                if (open && full) carry = stack[l] + carry;
                if (open && !full) {
                    stack[l] = carry;
                    open = false;
                }
            }
        }
        float total = 0.f;
        bool first = true;
#pragma unroll
        for (int l = 0; l < DOSE_STACK; ++l)           // the levels left, the fewest pieces first
            if ((pieces >> l) & 1) {
                total = first ? stack[l] : total + stack[l];
                first = false;
            }
        const double val = ((double)A + (double)log2f(total)) * ln2 - lognorm[r];
        if (r < S) {
            const float T = stats[(size_t)r * N + q];
            // a finite statistic so far from the bank that a square overflows fp32 (|t - z| above 2^63) leaves no finite sum: it
            // is treated as an infinite one
            const bool isn = T != T, isi = !isn && (fabsf(T) == INFINITY || !(fabs(val) < INFINITY));
            any_nan |= isn;
            any_inf |= isi;
            out[(size_t)r * N + q] = isn ? NAN : (isi ? -INFINITY : (float)val);
            out[(size_t)(S + 2 + r) * N + q] = (float)(-fabs((double)T - centre[r]) / sigma[r]);
            dose += val;
        } else {
            out[(size_t)S * N + q] = any_nan ? NAN : (any_inf ? -INFINITY : (float)dose);
            any_inf |= !(fabs(val) < INFINITY);          // the sum of the squares alone can overflow: the joint row only
            out[(size_t)(S + 1) * N + q] = any_nan ? NAN : (any_inf ? -INFINITY : (float)val);
        }
    }
    if (any_nan || any_inf) atomicOr(status, DOSE_STATUS_QUERY);
}

static int dose_slabs(long M) { return (int)((M + DOSE_SLAB - 1) / DOSE_SLAB); }
static int dose_pieces(long M) { return (int)((M + DOSE_PART - 1) / DOSE_PART); }

extern "C" int jvae_kde_partition(void) { return DOSE_PART; }

extern "C" size_t jvae_kde_fit_workspace_bytes(long M, int S) {
    if (M < 2 || M > DOSE_MAX_BANK || S < 1 || S > DOSE_MAX_STATS) return 0;
    return (size_t)S * dose_slabs(M) * sizeof(double);
}

// factors: a HOST pointer to (bandwidth, M^(-1/5), M^(-1/(S+4))), read here
extern "C" int jvae_kde_fit_f32(const float* bank, long M, int S, const double* factors, float* z, double* centre, double* sigma,
                                double* h1, double* hS, double* lognorm, int* status, void* ws, size_t ws_bytes, void* stream) {
    if (M < 2 || S < 1 || !factors) return JVAE_EINVAL;
    const double bandwidth = factors[0], scott1 = factors[1], scottS = factors[2];
    if (!(bandwidth > 0.) || !(scott1 > 0.) || !(scottS > 0.)) return JVAE_EINVAL;
    if (S > DOSE_MAX_STATS || M > DOSE_MAX_BANK) return JVAE_ENOTSUP;
    if (!bank || !z || !centre || !sigma || !h1 || !hS || !lognorm || !status || !ws || ((uintptr_t)ws & 7)) return JVAE_EINVAL;
    if (ws_bytes < jvae_kde_fit_workspace_bytes(M, S)) return JVAE_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int slabs = dose_slabs(M);
    double* part = (double*)ws;
    const dim3 grid((unsigned)slabs, (unsigned)S);
    dose_rowsum_kernel<<<grid, DOSE_BLOCK, 0, st>>>(bank, nullptr, part, M, status);
    JVAE_LAUNCH_CHECK();
    dose_fold_kernel<<<1, 64, 0, st>>>(part, slabs, M, S, 0, bandwidth, scott1, scottS, centre, sigma, h1, hS, lognorm, status);
    JVAE_LAUNCH_CHECK();
    dose_rowsum_kernel<<<grid, DOSE_BLOCK, 0, st>>>(bank, centre, part, M, status);
    JVAE_LAUNCH_CHECK();
    dose_fold_kernel<<<1, 64, 0, st>>>(part, slabs, M, S, 1, bandwidth, scott1, scottS, centre, sigma, h1, hS, lognorm, status);
    JVAE_LAUNCH_CHECK();
    dose_z_kernel<<<dim3((unsigned)cdiv(M, DOSE_BLOCK), (unsigned)S), DOSE_BLOCK, 0, st>>>(bank, centre, h1, z, M);
    JVAE_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t jvae_kde_workspace_bytes(long N, long M, int S) {
    if (N < 1 || N >= (1L << 31) || M < 2 || M > DOSE_MAX_BANK || S < 1 || S > DOSE_MAX_STATS) return 0;
    return (size_t)dose_pieces(M) * (S + 1) * N * sizeof(float2);
}

template <int S>
static void dose_launch(const float* stats, const float* z, const double* centre, const double* h1, float2* ws, long N, long M,
                        float kj, hipStream_t st) {
    dose_score_kernel<S><<<dim3((unsigned)cdiv(N, DOSE_QT), (unsigned)dose_pieces(M)), DOSE_BLOCK, 0, st>>>(stats, z, centre, h1, ws,
                                                                                                        N, M, kj);
}

extern "C" int jvae_kde_logdensity_f32(const float* stats, const float* z, const double* centre, const double* sigma,
                                       const double* h1, const double* lognorm, float* out, long N, long M, int S,
                                       const double* ratio2_host, int* status, void* ws, size_t ws_bytes, void* stream) {
    if (N < 0 || M < 2 || S < 1 || !ratio2_host) return JVAE_EINVAL;
    const double ratio2 = *ratio2_host;                // a HOST pointer, read here
    if (!(ratio2 > 0.) || !(ratio2 < INFINITY)) return JVAE_EINVAL;
    if (S > DOSE_MAX_STATS || M > DOSE_MAX_BANK || N >= (1L << 31)) return JVAE_ENOTSUP;
    if (N == 0) return 0;
    if (!stats || !z || !centre || !sigma || !h1 || !lognorm || !out || !status || !ws || ((uintptr_t)ws & 7)) return JVAE_EINVAL;
    if (ws_bytes < jvae_kde_workspace_bytes(N, M, S)) return JVAE_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float2* w = (float2*)ws;
    const float kj = (float)(DOSE_K * ratio2);
    switch (S) {
        case 1: dose_launch<1>(stats, z, centre, h1, w, N, M, kj, st); break;
        case 2: dose_launch<2>(stats, z, centre, h1, w, N, M, kj, st); break;
        case 3: dose_launch<3>(stats, z, centre, h1, w, N, M, kj, st); break;
        case 4: dose_launch<4>(stats, z, centre, h1, w, N, M, kj, st); break;
        case 5: dose_launch<5>(stats, z, centre, h1, w, N, M, kj, st); break;
        case 6: dose_launch<6>(stats, z, centre, h1, w, N, M, kj, st); break;
        case 7: dose_launch<7>(stats, z, centre, h1, w, N, M, kj, st); break;
        default: dose_launch<8>(stats, z, centre, h1, w, N, M, kj, st); break;
    }
    JVAE_LAUNCH_CHECK();
    dose_merge_kernel<<<cdiv(N, DOSE_BLOCK), DOSE_BLOCK, 0, st>>>(stats, w, centre, sigma, lognorm, out, N, S, dose_pieces(M), status);
    JVAE_LAUNCH_CHECK();
    return 0;
}
