// k nearest neighbours of query rows among the rows of a bank: distances on the fp32 matrix cores, fused with a per-row top-k
// selection, so that no (N, M) distance matrix exists anywhere (the deep-nearest-neighbour OOD score).
//
// Arithmetic.  The dot product of a pair is ONE chain of v_mfma_f32_32x32x2_f32 steps over k ascending (zero padded to a
// multiple of 8): bit for bit a k-ordered fmaf chain, whatever tile, wave or partition meets the pair.  The squared norms come
// from knn_sqnorms_kernel (a k-ordered fmaf chain per row) and are inputs here.  The epilogue is
//   plain:       d2 = fmaf(-2, q.b, |q|^2 + |b|^2)
//   normalised:  d2 = fmaf(-2, q.b / (max(sqrt|q|^2, 1e-12) * max(sqrt|b|^2, 1e-12)), 2)
// clamped at 0 by a select that keeps a NaN.
//
// Selection.  A workgroup of four waves owns 128 query rows (32 per wave) and one partition of the bank; a tile of 32 bank rows
// passes through LDS per step.  The accumulator of the 32 x 32 product has its bank row on the lane and its query row in the
// register, so a wave keeps, for each of its 32 query rows, the sorted list of the best 64 candidates with ONE SLOT PER LANE (two
// registers per row) and the row's current k-th value beside it.  A candidate is first compared with that k-th value; the few
// that pass are taken in lane (= bank index) order and put into the list by a wave-wide shift-insert (ballot + popcount for the
// position, DPP wave_shr:1 for the move: no LDS).  Order: (distance, bank
// index) ascending; candidates reach a list in ascending bank index, so `<` against the k-th value keeps the lower index of a tie.
// A distance that is not finite never passes (it orders as +inf) and sets KNN_STATUS_BANK.
//
// The lists of the partitions go to the workspace; knn_merge_kernel, a second launch, folds them in partition order with the
// same insert (one wave per query row) and writes the result.  Bits do not depend on the number of partitions: the distance of
// a pair does not, and the k smallest keys under a total order are one set.  No floating-point atomics; the status word takes an
// integer OR.
#include "common.h"
#include "jvae_hip.h"
#include <math.h>

#define KNN_MAX_K 64           // neighbours: one list slot per lane
#define KNN_MAX_DIM 4096
#define KNN_MAX_SPLITS 1024
#define KNN_QT 128             // query rows of a workgroup: 4 waves x 32
#define KNN_BT 32              // bank rows of a tile
#define KNN_KC 64              // columns of a staged chunk
#define KNN_LD 68              // LDS row stride in floats: rows stay 16-byte aligned, 4 banks apart
#define KNN_STATUS_BANK 1
#define KNN_STATUS_QUERY 2

__global__ __launch_bounds__(256) void knn_sqnorms_kernel(const float* __restrict__ x, float* __restrict__ sq, long M, int K) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= M) return;
    const float* p = x + r * K;
    float s = 0.f;
    for (int k = 0; k < K; ++k) s = fmaf(p[k], p[k], s);
    sq[r] = s;
}

__device__ __forceinline__ float knn_readlane(float v, int src) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src));
}

// lanes above `src`
__device__ __forceinline__ unsigned long long knn_above(int src) { return (~0ull << src) << 1; }

// Put the wave-uniform candidate (d, idx) into the list (ld, li): one slot per lane, ascending by (distance, index), unused slots
// +inf / -1 at the end.  The slots that order before the candidate are a prefix; the others move up one lane, lane 63 drops out.
// (branch-free on purpose: with branches the compiler carries the whole register-resident set of lists through every join)
__device__ __forceinline__ int knn_shift_up(int v) {
    // lane l takes lane l - 1 (DPP wave_shr:1, on the vector ALU: no LDS round trip); lane 0 keeps its own value
    return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false);
}
__device__ __forceinline__ void knn_insert(float& ld, int& li, float d, int idx, int lane) {
    const bool before = (ld < d) | ((ld == d) & (li < idx));
    const int p = __popcll(__builtin_amdgcn_ballot_w64(before));
    const float ud = __builtin_bit_cast(float, knn_shift_up(__builtin_bit_cast(int, ld)));
    const int ui = knn_shift_up(li);
    ld = lane == p ? d : (lane > p ? ud : ld);
    li = lane == p ? idx : (lane > p ? ui : li);
}

// rows x KNN_KC floats of `src` (row stride K) from column k0 into LDS, zero where the row or the column does not exist.  Column
// k of the chunk lands at (k & 1) * 32 + (k >> 1): the 32x32x2 step s reads k = 2 s + (lane >> 5), so a lane's operands of four
// consecutive steps are one 16-byte read.
template <int ROWS>
__device__ __forceinline__ void knn_stage(float* lds, const float* __restrict__ src, long row0, long row_end, int K, int k0) {
    const int kk = threadIdx.x & 63, col = k0 + kk, r0 = threadIdx.x >> 6;     // a thread keeps its column; rows r0, r0 + 4, ...
    float* dst = lds + (kk & 1) * 32 + (kk >> 1);
    for (int rb = r0; rb < ROWS; rb += 32) {          // eight loads in flight, then eight LDS writes
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const long row = row0 + rb + 4 * j;
            v[j] = (row < row_end && col < K) ? src[row * K + col] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) dst[(rb + 4 * j) * KNN_LD] = v[j];
    }
}

template <bool NORM>
__global__ __launch_bounds__(256) void knn_partial_kernel(const float* __restrict__ q, const float* __restrict__ q_sq,
                                                          const float* __restrict__ bank, const float* __restrict__ bank_sq,
                                                          float* __restrict__ pd, int* __restrict__ pi, long N, long M, int K, int k,
                                                          int splits, long per, int* status) {
    __shared__ __attribute__((aligned(16))) float s_q[KNN_QT * KNN_LD];
    __shared__ __attribute__((aligned(16))) float s_b[KNN_BT * KNN_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, c = lane & 31;
    const int part = blockIdx.y;
    const long q0 = (long)blockIdx.x * KNN_QT, wq0 = q0 + wave * 32;
    const long b_lo = part * per < M ? part * per : M, b_hi = b_lo + per < M ? b_lo + per : M;
    const bool active = wq0 < N;                       // wave-uniform: a wave without rows only helps staging
    const float inf = INFINITY;

    float Ld[32], qv[16], thr[16];
    int Li[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        Ld[j] = inf;
        Li[j] = -1;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {                     // accumulator register r of this lane: query row (r & 3) + 8 (r >> 2) + 4 h
        const long row = wq0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const float qs = row < N ? q_sq[row] : NAN;
        qv[r] = NORM ? fmaxf(sqrtf(qs), 1e-12f) : qs;
        thr[r] = fabsf(qs) < inf ? inf : -inf;         // a row that is absent or not finite takes no candidate
    }
    const int nchunks = (K + KNN_KC - 1) / KNN_KC;
    bool flag = false;

    for (long b0 = b_lo; b0 < b_hi; b0 += KNN_BT) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int ch = 0; ch < nchunks; ++ch) {
            const int k0 = ch * KNN_KC, kn = K - k0 < KNN_KC ? K - k0 : KNN_KC;
            __syncthreads();
            if (nchunks > 1 || b0 == b_lo) knn_stage<KNN_QT>(s_q, q, q0, N, K, k0);      // K <= 64: the query tile stays resident
            knn_stage<KNN_BT>(s_b, bank, b0, b_hi, K, k0);
            __syncthreads();
            if (active) {
                const float* pa = s_q + (wave * 32 + c) * KNN_LD + h * 32;
                const float* pb = s_b + c * KNN_LD + h * 32;
                const int nt = (kn + 7) >> 3;          // groups of four steps; the columns past kn are zeros
                for (int t = 0; t < nt; ++t) {
                    const f32x4 a4 = *reinterpret_cast<const f32x4*>(pa + 4 * t);
                    const f32x4 b4 = *reinterpret_cast<const f32x4*>(pb + 4 * t);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[j], b4[j], acc, 0, 0, 0);
                }
            }
        }
        if (!active) continue;
        const long col = b0 + c;
        const bool cv = col < b_hi;
        const float bs = cv ? bank_sq[col] : 0.f;
        const bool cfin = cv && fabsf(bs) < inf;       // a norm that overflowed or is NaN: the row is never selected
        const float bv = NORM ? fmaxf(sqrtf(bs), 1e-12f) : bs;
        flag |= cv && !cfin;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float d = NORM ? fmaf(-2.f, acc[r] / (qv[r] * bv), 2.f) : fmaf(-2.f, acc[r], qv[r] + bv);
            d = d < 0.f ? 0.f : d;                     // keeps a NaN
            flag |= cfin & (thr[r] >= 0.f) & !(d < inf);
            if (!__builtin_amdgcn_ballot_w64(cfin & (d < thr[r]))) continue;      // rare once the lists have filled
            // (taking one candidate of each half per turn, to overlap the two dependent chains, was measured slower: late in a
            // partition one half has a candidate and the other does not)
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {           // the two query rows of the register, each with its own list
                const unsigned long long half = hh ? 0xffffffff00000000ull : 0xffffffffull;
                unsigned long long mask = __builtin_amdgcn_ballot_w64(cfin & (d < thr[r])) & half;
                while (mask) {
                    const int src = __builtin_ctzll(mask);
                    knn_insert(Ld[2 * r + hh], Li[2 * r + hh], knn_readlane(d, src), (int)b0 + (src & 31), lane);
                    const float kth = knn_readlane(Ld[2 * r + hh], k - 1);
                    thr[r] = h == hh ? kth : thr[r];
                    mask = __builtin_amdgcn_ballot_w64(cfin & (d < thr[r])) & half & knn_above(src);
                }
            }
        }
    }
    if (!active) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const long row = wq0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
            if (row < N && lane < k) {
                const long o = (row * splits + part) * k + lane;
                pd[o] = Ld[2 * r + hh];
                pi[o] = Li[2 * r + hh];
            }
        }
    }
    if (__builtin_amdgcn_ballot_w64(flag) && lane == 0) atomicOr(status, KNN_STATUS_BANK);
}

// One wave per query row: the partitions' lists, each ascending and the partitions in ascending bank index, folded in that order.
__global__ __launch_bounds__(256) void knn_merge_kernel(const float* __restrict__ pd, const int* __restrict__ pi,
                                                        const float* __restrict__ q_sq, float* __restrict__ d2, int* __restrict__ idx,
                                                        long N, int k, int splits, int* status) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const float inf = INFINITY;
    if (!(fabsf(q_sq[row]) < inf)) {                   // a query row with a NaN or an infinity (or an overflowing norm)
        if (lane < k) {
            d2[row * k + lane] = NAN;
            idx[row * k + lane] = -1;
        }
        if (lane == 0) atomicOr(status, KNN_STATUS_QUERY);
        return;
    }
    const float* rd = pd + row * splits * k;
    const int* ri = pi + row * splits * k;
    float ld = lane < k ? rd[lane] : inf;
    int li = lane < k ? ri[lane] : -1;
    float thr = knn_readlane(ld, k - 1);
    for (int p = 1; p < splits; ++p) {
        const float cd = lane < k ? rd[p * k + lane] : inf;
        const int ci = lane < k ? ri[p * k + lane] : -1;
        unsigned long long mask = __builtin_amdgcn_ballot_w64(cd < thr);
        while (mask) {
            const int src = __builtin_ctzll(mask);
            knn_insert(ld, li, knn_readlane(cd, src), __builtin_amdgcn_readlane(ci, src), lane);
            thr = knn_readlane(ld, k - 1);
            mask = __builtin_amdgcn_ballot_w64(cd < thr) & knn_above(src);
        }
    }
    if (lane < k) {
        d2[row * k + lane] = ld;
        idx[row * k + lane] = li;
    }
}

// Partitions when the caller leaves the choice (splits = 0): about one workgroup per CU of an MI355X, at least 256 bank rows each.
static int knn_pick_splits(long N, long M) {
    const long qtiles = (N + KNN_QT - 1) / KNN_QT;
    long s = qtiles > 0 ? 256 / qtiles : 1;
    const long cap = M / 256;
    if (s > cap) s = cap;
    if (s > KNN_MAX_SPLITS) s = KNN_MAX_SPLITS;
    return s < 1 ? 1 : (int)s;
}

static int knn_check_sizes(long N, long M, int K, int k, int splits) {
    if (N < 0 || M < 0 || splits < 0 || splits > KNN_MAX_SPLITS) return JVAE_EINVAL;
    if (k < 1 || k > KNN_MAX_K || K < 1 || K > KNN_MAX_DIM || M >= (1L << 31) || N >= (1L << 31)) return JVAE_ENOTSUP;
    return 0;
}

extern "C" int jvae_knn_sqnorms_f32(const float* x, float* sq, long M, int K, void* stream) {
    if (M < 0) return JVAE_EINVAL;
    if (K < 1 || K > KNN_MAX_DIM || M >= (1L << 31)) return JVAE_ENOTSUP;
    if (M == 0) return 0;
    if (!x || !sq) return JVAE_EINVAL;
    knn_sqnorms_kernel<<<cdiv(M, 256), 256, 0, (hipStream_t)stream>>>(x, sq, M, K);
    JVAE_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t jvae_knn_workspace_bytes(long N, long M, int K, int k, int splits) {
    if (knn_check_sizes(N, M, K, k, splits)) return 0;
    if (!splits) splits = knn_pick_splits(N, M);
    return (size_t)N * splits * k * (sizeof(float) + sizeof(int));
}

extern "C" int jvae_knn_f32(const float* q, const float* q_sq, const float* bank, const float* bank_sq, float* d2_out, int* idx_out,
                            long N, long M, int K, int k, int normalized, int splits, int* status, void* ws, size_t ws_bytes,
                            void* stream) {
    const int rc = knn_check_sizes(N, M, K, k, splits);
    if (rc) return rc;
    if (N == 0) return 0;
    if (!q || !q_sq || !d2_out || !idx_out || !status || !ws || (M > 0 && (!bank || !bank_sq))) return JVAE_EINVAL;
    if (!splits) splits = knn_pick_splits(N, M);
    const size_t half = (size_t)N * splits * k * sizeof(float);
    if (ws_bytes < 2 * half) return JVAE_EWORKSPACE;
    if (((uintptr_t)ws) & 3) return JVAE_EINVAL;
    float* pd = (float*)ws;
    int* pi = (int*)((char*)ws + half);
    long per = (M + splits - 1) / splits;
    per = (per + KNN_BT - 1) / KNN_BT * KNN_BT;       // whole tiles; trailing partitions may be empty (their lists stay +inf / -1)
    const dim3 grid((unsigned)cdiv(N, KNN_QT), (unsigned)splits);
    hipStream_t st = (hipStream_t)stream;
    if (normalized)
        knn_partial_kernel<true><<<grid, 256, 0, st>>>(q, q_sq, bank, bank_sq, pd, pi, N, M, K, k, splits, per, status);
    else
        knn_partial_kernel<false><<<grid, 256, 0, st>>>(q, q_sq, bank, bank_sq, pd, pi, N, M, K, k, splits, per, status);
    JVAE_LAUNCH_CHECK();
    knn_merge_kernel<<<cdiv(N, 4), 256, 0, st>>>(pd, pi, q_sq, d2_out, idx_out, N, k, splits, status);
    JVAE_LAUNCH_CHECK();
    return 0;
}
