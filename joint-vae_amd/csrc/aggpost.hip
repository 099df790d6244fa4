// The aggregate posterior of a bank of N diagonal Gaussians (Hoffman & Johnson 2016, "ELBO surgery"; Chen et al. 2018, beta-TCVAE;
// DESIGN.md section 7u): log q(z) = log 1/|S| sum_{n in S} N(z; mu_n, diag e^{lv_n}) at M queries, and optionally the same for every
// coordinate alone, with S the whole bank or the rows of the query's group.  No (M, N) or (M, N, K) array exists anywhere.
//
// Stored operands (jvae_aggpost_prepare_f32, once per bank).  w = fp32(exp(-(double)lv)), c_n = fp32(sum_k (double)lv_nk), k
// ascending; mu, w and lv are stored k-major, (K, Np) with Np = N rounded up to AGP_TILE (padding rows are zeros and are masked,
// never read as terms), so that a tile of bank rows is a run of floats for every k.
//
// Arithmetic.  A pair (query m, bank row n) has Q = c_n + sum_k (z_mk - mu_nk)^2 w_nk: the fmaf chain acc = fmaf(d * d, w, acc)
// from acc = c_n on, k ascending, d = z - mu and d * d rounded on their own (built with -ffp-contract=off) - the direct form; its
// bits hang on (z_m, row n, K) alone, whichever tile, wave or piece meets the pair.  The pair's term is 2^(kk (Q - a)) with kk =
// -log2(e) / 2 and a the smallest Q of the sum: the DIFFERENCE is taken before the product (kk Q itself is only known to 2^-24 of
// its size, thousands of units for a far query), so the largest term of every sum is exactly 1, no exponent is positive and the
// sum is finite and >= 1 however far the query is.  A coordinate's term is the same with Q = fmaf(d * d, w, lv).
//
// Partition.  The bank is cut into pieces of AGP_PART rows whatever M and the grid are.  A workgroup owns AGP_QT queries (one per
// lane) and ONE piece; wave v of its four takes rows 16 v .. 16 v + 15 of every 64-row tile of the piece (joint launch) or rows
// 64 v .. 64 v + 63 of every 256-row tile (marginal launch).  A wave forms the terms of 16 (8) rows at a time: their smallest Q
// (exact, no order), the terms against it added as a tree, and the result folded into its running (a, s):
//   a' = min(a, a_t),  s' = s 2^(kk (a - a')) + s_t 2^(kk (a_t - a'))      (one of the two factors is exactly 1)
// in the tiles' order; the four waves meet through LDS as a tree, a piece leaves (a, s) and the number of rows of the query's
// group in the workspace, and the merge launch folds the pieces in their order the same way (pairwise: a binary counter) and ends
// in fp64: log q = -a / 2 + ln s - ln |S| - (K / 2) ln 2 pi, rounded once.  No floating-point atomics: a second run, another M or
// a subset of the queries give the same bits.
//
// Masked rows (padding, another group) have Q = +inf: their term is exactly +0 and they are in no minimum.  A query whose group has
// no row gets -inf and AGP_STATUS_EMPTY.  A query with a NaN gets NaN, one with an infinite element -inf, and so does a finite
// query so far away that every Q overflows fp32; they set AGP_STATUS_QUERY.  A non-finite stored operand sets AGP_STATUS_BANK (the
// workgroups of the first query tile look at what they stage).  The status word only ever takes an integer OR.
//
// Limits: 1 <= K <= AGP_MAX_K, 1 <= N <= AGP_MAX_BANK (so at most AGP_MAX_BANK / AGP_PART = 16384 pieces, the binary counter of
// the merge holds 2^AGP_STACK), 1 <= M < 2^31.
#include "common.h"
#include "jvae_hip.h"
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

// one thread per row of the padded bank
__global__ __launch_bounds__(AGP_BLOCK) void agp_prepare_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
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
        wT[(size_t)k * Np + n] = in ? (float)exp(-(double)l) : 0.f;
        lvT[(size_t)k * Np + n] = l;
    }
    c[n] = (float)sum;
}

// (a, s) <- (a, s) + (at, st): the fold of the file's head.  An empty side has a = +inf and s = 0 and leaves the other as it is.
__device__ __forceinline__ void agp_fold(float& a, float& s, float at, float st) {
    const float an = fminf(a, at), as = an < INFINITY ? an : 0.f;
    const float left = s * agp_exp2(AGP_KK * (a - as)), right = st * agp_exp2(AGP_KK * (at - as));
    s = left + right;
    a = an;
}

// ws pair[(piece, q)] = (a, s) of the piece, cnt[(piece, q)] = rows of the query's group in it
template <bool COND>
__global__ __launch_bounds__(AGP_BLOCK) void agp_joint_kernel(const float* __restrict__ z, const int* __restrict__ zgroup,
                                                              const float* __restrict__ muT, const float* __restrict__ wT,
                                                              const float* __restrict__ c, const int* __restrict__ group,
                                                              float2* __restrict__ pair, int* __restrict__ cnt, long M, long N,
                                                              long Np, int K, int* status) {
    __shared__ __attribute__((aligned(16))) float mt[AGP_KC][AGP_TILE];
    __shared__ __attribute__((aligned(16))) float wt[AGP_KC][AGP_TILE];
    __shared__ float zt[AGP_KC][AGP_QT + 1];           // + 1: the transposing store walks k at a stride of 65 words
    __shared__ float ct[AGP_TILE];
    __shared__ int gt[AGP_TILE];
    __shared__ float xa[AGP_WAVES][AGP_QT], xs[AGP_WAVES][AGP_QT];
    __shared__ int xc[AGP_WAVES][AGP_QT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long q0 = (long)blockIdx.x * AGP_QT, q = q0 + lane;
    const long base = (long)blockIdx.y * AGP_PART, end = base + AGP_PART < N ? base + AGP_PART : N;
    const int qg = COND ? (q < M ? max(zgroup[q], -1) : -1) : 0;      // bank groups are >= 0, padding rows -2
    const bool look = blockIdx.x == 0;                 // the first query tile looks at the operands it stages
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
        const float as = at < INFINITY ? at : 0.f;
        float e[AGP_ROWS];
#pragma unroll
        for (int r = 0; r < AGP_ROWS; ++r) e[r] = agp_exp2(AGP_KK * (acc[r] - as));
#pragma unroll
        for (int r = 0; r < AGP_ROWS; r += 4) e[r] = (e[r] + e[r + 1]) + (e[r + 2] + e[r + 3]);
        const float st = (e[0] + e[4]) + (e[8] + e[12]);
        agp_fold(a, s, at, st);
    }
    if (bad) atomicOr(status, AGP_STATUS_BANK);
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

// One thread per output: R = 1 (out (M,), the whole row of z is looked at) or R = K (out (M, K), coordinate r of query q).
// pair[((piece, r), q)], cnt[(piece, q)]
__global__ __launch_bounds__(AGP_BLOCK) void agp_merge_kernel(const float* __restrict__ z, const float2* __restrict__ pair,
                                                              const int* __restrict__ cnt, float* __restrict__ out, long M,
                                                              int K, int R, int pieces, int* status) {
    const long i = (long)blockIdx.x * AGP_BLOCK + threadIdx.x;
    if (i >= (long)R * M) return;
    const long r = i / M, q = i - r * M;
    const float2* w = pair + (size_t)r * M + q;
    const size_t step = (size_t)R * M;
    float A = INFINITY;
    long rows = 0;
    for (int p = 0; p < pieces; ++p) {
        A = fminf(A, w[p * step].x);
        rows += cnt[(size_t)p * M + q];
    }
    float stack[AGP_STACK];
#pragma unroll
    for (int l = 0; l < AGP_STACK; ++l) stack[l] = 0.f;
    const float As = A < INFINITY ? A : 0.f;
    for (int p = 0; p < pieces; ++p) {
        const float2 v = w[p * step];
        float carry = v.y * exp2f(AGP_KK * (v.x - As));
        bool open = true;
#pragma unroll
        for (int l = 0; l < AGP_STACK; ++l) {          // a binary counter: level l holds the sum of 2^l pieces
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
    for (int l = 0; l < AGP_STACK; ++l)                // the levels left, the fewest pieces first
        if ((pieces >> l) & 1) {
            total = first ? stack[l] : total + stack[l];
            first = false;
        }
    bool isn = false, isi = false;
    if (R == 1) {
        for (int k = 0; k < K; ++k) {
            const float v = z[(size_t)q * K + k];
            isn |= v != v;
            isi |= fabsf(v) == INFINITY;
        }
    } else {
        const float v = z[(size_t)q * K + r];
        isn = v != v;
        isi = fabsf(v) == INFINITY;
    }
    const double half_log2pi = 0.91893853320467274178;
    const double val = -0.5 * (double)A + log((double)total) - log((double)rows) - (R == 1 ? K : 1) * half_log2pi;
    const bool empty = rows == 0, lost = !(fabs(val) < INFINITY);      // lost: every Q overflowed, or a non-finite operand
    out[R == 1 ? q : q * K + r] = isn ? NAN : (isi || empty || lost ? -INFINITY : (float)val);
    if (isn || isi || (lost && !empty)) atomicOr(status, AGP_STATUS_QUERY);
    else if (empty) atomicOr(status, AGP_STATUS_EMPTY);
}

static long agp_padded(long N) { return (N + AGP_TILE - 1) / AGP_TILE * AGP_TILE; }
static int agp_pieces(long N) { return (int)((N + AGP_PART - 1) / AGP_PART); }
static bool agp_in_range(long M, long N, int K) {
    return M >= 1 && M < (1L << 31) && N >= 1 && N <= AGP_MAX_BANK && K >= 1 && K <= AGP_MAX_K;
}

extern "C" int jvae_aggpost_partition(void) { return AGP_PART; }

extern "C" long jvae_aggpost_padded_rows(long N) { return N >= 1 && N <= AGP_MAX_BANK ? agp_padded(N) : 0; }

extern "C" int jvae_aggpost_prepare_f32(const float* mu, const float* log_var, float* muT, float* wT, float* lvT, float* c, long N,
                                        int K, void* stream) {
    if (N < 1 || K < 1) return JVAE_EINVAL;
    if (N > AGP_MAX_BANK || K > AGP_MAX_K) return JVAE_ENOTSUP;
    if (!mu || !log_var || !muT || !wT || !lvT || !c) return JVAE_EINVAL;
    const long Np = agp_padded(N);
    agp_prepare_kernel<<<cdiv(Np, AGP_BLOCK), AGP_BLOCK, 0, (hipStream_t)stream>>>(mu, log_var, muT, wT, lvT, c, N, Np, K);
    JVAE_LAUNCH_CHECK();
    return 0;
}

// pieces * M (a, s) pairs and counts; with dims, pieces * K * M pairs more
extern "C" size_t jvae_aggpost_workspace_bytes(long M, long N, int K, int dims) {
    if (!agp_in_range(M, N, K)) return 0;
    const size_t pm = (size_t)agp_pieces(N) * M;
    return pm * (sizeof(float2) + sizeof(int)) + (dims ? pm * K * sizeof(float2) : 0);
}

extern "C" int jvae_aggpost_logdensity_f32(const float* z, const int* zgroup, const float* muT, const float* wT, const float* lvT,
                                           const float* c, const int* group, float* logq, float* logq_dims, long M, long N, int K,
                                           int conditional, int* status, void* ws, size_t ws_bytes, void* stream) {
    if (M < 0 || N < 1 || K < 1) return JVAE_EINVAL;
    if (M == 0) return 0;
    if (!agp_in_range(M, N, K)) return JVAE_ENOTSUP;
    if (!z || !muT || !wT || !lvT || !c || !logq || !status || !ws || ((uintptr_t)ws & 7)) return JVAE_EINVAL;
    if (conditional && (!zgroup || !group)) return JVAE_EINVAL;
    const int dims = logq_dims != nullptr;
    if (ws_bytes < jvae_aggpost_workspace_bytes(M, N, K, dims)) return JVAE_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int pieces = agp_pieces(N);
    const long Np = agp_padded(N);
    const size_t pm = (size_t)pieces * M;
    float2* pair = (float2*)ws;
    float2* dpair = pair + pm;
    int* cnt = (int*)(dpair + (dims ? pm * K : 0));
    const dim3 grid((unsigned)cdiv(M, AGP_QT), (unsigned)pieces);
    if (conditional)
        agp_joint_kernel<true><<<grid, AGP_BLOCK, 0, st>>>(z, zgroup, muT, wT, c, group, pair, cnt, M, N, Np, K, status);
    else
        agp_joint_kernel<false><<<grid, AGP_BLOCK, 0, st>>>(z, zgroup, muT, wT, c, group, pair, cnt, M, N, Np, K, status);
    JVAE_LAUNCH_CHECK();
    agp_merge_kernel<<<cdiv(M, AGP_BLOCK), AGP_BLOCK, 0, st>>>(z, pair, cnt, logq, M, K, 1, pieces, status);
    JVAE_LAUNCH_CHECK();
    if (dims) {
        const dim3 dgrid(grid.x, grid.y, (unsigned)cdiv(K, AGP_KD));
        if (conditional)
            agp_dims_kernel<true><<<dgrid, AGP_BLOCK, 0, st>>>(z, zgroup, muT, wT, lvT, group, dpair, M, N, Np, K);
        else
            agp_dims_kernel<false><<<dgrid, AGP_BLOCK, 0, st>>>(z, zgroup, muT, wT, lvT, group, dpair, M, N, Np, K);
        JVAE_LAUNCH_CHECK();
        agp_merge_kernel<<<cdiv((long)M * K, AGP_BLOCK), AGP_BLOCK, 0, st>>>(z, dpair, cnt, logq_dims, M, K, K, pieces, status);
        JVAE_LAUNCH_CHECK();
    }
    return 0;
}
