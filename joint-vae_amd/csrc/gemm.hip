// fp32 MFMA GEMM for gfx950:  C[b](m,n) (+)= sum_k A[b](m,k) * B[b](k,n)  (+ bias, ReLU)
//
// Two bodies, gemm_tile_body and gemm_x3_body, of 256 threads (4 waves as 2 x 2) and K step BK = 32, sixteen variants of them
// (VARIANTS: the table every launch, grouped kernel, LDS size and name is derived from).
//   gemm_tile_body  v_mfma_f32_32x32x2_f32: exact fp32 (k-ordered fmaf chain; a single product comes back as the correctly rounded
//                   fp64 product, 0 ulp in tests/test_24_gemm_sweep_gpu.py::test_single_products_of_the_fp32_kernel), 64
//                   FLOP/clk/SIMD.  Block tile 64 x 64 or 128 x 128; LDS images are k-major (As[k][m], Bs[k][n]) so that every
//                   fragment read is 32 consecutive dwords per half-wave (conflict-free ds_read_b32, MI355X_MICROARCH.md §LDS).
//   gemm_x3_body    the same product on the bf16 matrix cores: every fp32 operand split exactly into three bf16 terms (below).
// Both stage their operands global -> registers -> LDS with the next K step's global loads in flight under the current step's
// MFMAs; which float4 group of an operand tile a thread stages is StageMap, for the load and for the store that consumes it.
// Both take their block's operands and K slice from TileCtx and store through gemm_store().  Arbitrary element strides on A, B
// and C let one kernel serve NN / NT / TN products, per-image batched products (grid.z) and split-K with float-atomic
// accumulation or stored slices.
//
// Serves: Linear layers fwd/dgrad/wgrad (reference: nn.Linear in layers.py:283-296, cvae.py:291-326),
// the 1x1 -> kxk first transposed conv of the upsampler, and the generic (im2col) convolution path.
// Independent products that cannot fill the chip alone (the two latent heads, a linear layer's dgrad and weight gradient) share
// ONE launch through jvae_gemm_group_f32: the same plan, bodies and bits per product as alone.
#include <stdio.h>
#include <stdlib.h>
#include <utility>
#include "common.h"
#include "jvae_hip.h"
#include "conv_x3.h"
#include "jvae_internal.h"
#include "conv_dispatch.h"

namespace {

constexpr int BK = 32;          // K step of both bodies: 64 MFMAs (128x128 tile) between two barriers; keeps the split-bf16 images at
                                // 32 KB -> four workgroups per CU (the products there are latency-bound: few tiles, short K slices)

struct GemmP {
    const float* A; long sAm, sAk, sAb;
    const float* B; long sBk, sBn, sBb;
    float* C; long sCm, sCn, sCb;
    const float* bias;   // nullptr or per-n (mode 1) / per-m (mode 2)
    int bias_mode;
    int bias_div;        // mode 1: bias[n / bias_div] (transposed conv on a 1x1 input: channel = column / (KH*KW))
    int M, N, K;
    int splitk;          // grid.z = batch * splitk
    int kchunk;          // K elements per split (multiple of BK)
    int flags;           // 1 = accumulate into C, 2 = ReLU, 4 = atomic add (split-K), 8 = split s stores to C + s*sCsplit
    long sCsplit;        // (flag 8) element distance between the partial results of consecutive K splits
    int vecA, vecB;      // 16-byte vector loads are legal for this operand
    int xcd;             // gemm_x3_kernel: XCD-aware tile order
};

// What block tile (bx, by, bz) of a BM x BN tiling works on: its rows and columns, its K slice, its batch's operands.  (A
// constructor, and the members in this order: returned from a function, or with the bias slice `split == 0 && !(flags & 8)` as
// a member, the kernels build to other instruction orders - profiles/NOTES.md.)
struct TileCtx {
    int m0, n0;
    int batch, split, kbeg, kend;
    const float* A; const float* B; float* C;     // C: of this slice where the slices are stored (flag 8)
    __device__ __forceinline__ TileCtx(const GemmP& p, int BM, int BN, unsigned bx, unsigned by, unsigned bz)
        : m0(by * BM), n0(bx * BN), batch(bz / p.splitk), split(bz % p.splitk), kbeg(split * p.kchunk),
          kend(min(p.K, kbeg + p.kchunk)), A(p.A + (long)batch * p.sAb), B(p.B + (long)batch * p.sBb),
          C(p.C + (long)batch * p.sCb + ((p.flags & 8) ? (long)split * p.sCsplit : 0L)) {}
};

// One element of the result (bias already added) into C, as the product's flags say.
__device__ __forceinline__ void gemm_store(const GemmP& p, float* dst, float v) {
    if (p.flags & 8) {
        *dst = v;
    } else if (p.flags & 4) {
        atomicAdd(dst, v);
    } else {
        if (p.flags & 1) v += *dst;
        if (p.flags & 2) v = fmaxf(v, 0.f);
        *dst = v;
    }
}

// 4 consecutive elements along the contiguous direction, zero-filled outside [0,lim).
template <bool VEC>
__device__ __forceinline__ f32x4 load4(const float* p, long stride, int i0, int lim, bool row_ok) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!row_ok) return v;
    if (VEC) {
        if (i0 + 3 < lim) return *reinterpret_cast<const f32x4*>(p);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (i0 + j < lim) v[j] = p[j * stride];
    return v;
}

// The staging map: the g-th float4 group that thread tid holds of a ROWS x BK operand tile.  KC: the operand is contiguous along k
// in memory (A with AK, B without BNC), and the groups run along k; otherwise they run along the rows.  The contiguous direction
// runs fastest over the threads.  A global load and the LDS store that consumes it both take their place from here.
template <bool KC, int ROWS>
struct StageMap {
    static constexpr int Q = (KC ? BK : ROWS) / 4;      // groups along the contiguous direction
    static constexpr int G = ROWS * BK / 4 / 256;       // groups per thread
    int fq, sl;                                         // LDS slot: group along the contiguous direction, index along the other
    __device__ __forceinline__ StageMap(int tid, int g) : fq(tid % Q), sl(tid / Q + g * (256 / Q)) {}
    // first element of the group, for the tile at row r0 and the K step at k0
    __device__ __forceinline__ int row(int r0) const { return KC ? r0 + sl : r0 + fq * 4; }
    __device__ __forceinline__ int k(int k0) const { return KC ? k0 + fq * 4 : k0 + sl; }
};

// The group of the map, zero-filled outside the operand and the K slice: any strides, 16-byte loads where the plan allows them
// (vec).  The operand: `rows` rows (M of A, N of B) sR elements apart, k sK apart.  KFIRST: k is the operand's first index (B[k][n];
// A[m][k] has it second) - the order in which the two terms of the address are added.  It decides nothing but the compiler's
// instruction order; so does passing the operand as a struct, which is why it comes as plain arguments (profiles/NOTES.md).
template <bool KC, int ROWS, bool KFIRST>
__device__ __forceinline__ f32x4 stage_load(const float* base, long sR, long sK, int rows, int vec, int tid, int g, int r0, int k0, int kend) {
    const StageMap<KC, ROWS> s(tid, g);
    const int row = s.row(r0), k = s.k(k0);
    const float* src = KFIRST ? base + (long)k * sK + (long)row * sR : base + (long)row * sR + (long)k * sK;
    if (KC) return vec ? load4<true>(src, sK, k, kend, row < rows) : load4<false>(src, sK, k, kend, row < rows);
    return vec ? load4<true>(src, sR, row, rows, k < kend) : load4<false>(src, sR, row, rows, k < kend);
}

// AK: A is contiguous along k (row-major MxK); otherwise thread groups run along m.
// BN_: B is contiguous along n (row-major KxN); otherwise along k.
//
// The body of one block tile is a __device__ function of the tile indices (bx, by, bz) and the grid (gx, gy, gz) they belong to,
// so that the stand-alone kernel (the hardware's own block index) and the grouped kernel (a flat index cut into records,
// gemm_group_tile_kernel) run the same code on the same operands in the same K order.
template <int BM, int BN>
struct TileLds {
    static constexpr int LDA = BM + 4, LDB = BN + 4;
    static constexpr int BYTES = BK * (LDA + LDB) * (int)sizeof(float);
};

// A staged group into the k-major fp32 image img[BK][LD].
template <bool KC, int ROWS, int LD>
__device__ __forceinline__ void tile_lstore(float* img, int tid, int g, const f32x4& v) {
    const StageMap<KC, ROWS> s(tid, g);
    if (KC) {
#pragma unroll
        for (int j = 0; j < 4; ++j) img[(s.fq * 4 + j) * LD + s.sl] = v[j];
    } else {
        *reinterpret_cast<f32x4*>(&img[s.sl * LD + s.fq * 4]) = v;
    }
}

template <int BM, int BN, bool AK, bool BNC>
__device__ __forceinline__ void gemm_tile_body(const GemmP& p, float* __restrict__ lds, unsigned bx, unsigned by, unsigned bz,
                                               unsigned gx, unsigned gy, unsigned gz) {
    constexpr int LDA = TileLds<BM, BN>::LDA, LDB = TileLds<BM, BN>::LDB;
    constexpr int WM = BM / 2, WN = BN / 2;          // wave tile
    constexpr int TM = WM / 32, TN = WN / 32;        // 32x32 MFMA tiles per wave
    constexpr int GA = StageMap<AK, BM>::G, GB = StageMap<!BNC, BN>::G;      // float4 groups per thread
    float* As = lds;                                 // [BK][LDA]
    float* Bs = lds + BK * LDA;                      // [BK][LDB]
    (void)gx; (void)gy; (void)gz;                    // (no tile remap in this kernel)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm0 = (wave >> 1) * WM, wn0 = (wave & 1) * WN;
    const TileCtx t(p, BM, BN, bx, by, bz);
    const int m0 = t.m0, n0 = t.n0, kbeg = t.kbeg, kend = t.kend;
    const float* A = t.A; const float* B = t.B; float* C = t.C;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    f32x4 ra[GA], rb[GB];

    auto gload = [&](int k0) {
#pragma unroll
        for (int g = 0; g < GA; ++g) ra[g] = stage_load<AK, BM, false>(A, p.sAm, p.sAk, p.M, p.vecA, tid, g, m0, k0, kend);
#pragma unroll
        for (int g = 0; g < GB; ++g) rb[g] = stage_load<!BNC, BN, true>(B, p.sBn, p.sBk, p.N, p.vecB, tid, g, n0, k0, kend);
    };
    auto lstore = [&]() {
#pragma unroll
        for (int g = 0; g < GA; ++g) tile_lstore<AK, BM, LDA>(As, tid, g, ra[g]);
#pragma unroll
        for (int g = 0; g < GB; ++g) tile_lstore<!BNC, BN, LDB>(Bs, tid, g, rb[g]);
    };

    const int half = lane >> 5, l31 = lane & 31;
    if (kbeg < kend) gload(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += BK) {
        __syncthreads();                 // previous tile's fragment reads are done
        lstore();
        __syncthreads();
        if (k0 + BK < kend) gload(k0 + BK);   // in flight under the MFMAs below
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            float a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = As[(2 * kk + half) * LDA + wm0 + i * 32 + l31];
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = Bs[(2 * kk + half) * LDB + wn0 + j * 32 + l31];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }

    // epilogue: D[i][j]: j = lane&31, i = (r&3) + 8*(r>>2) + 4*(lane>>5)
    const bool lead = (t.split == 0) && !(p.flags & 8);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wn0 + j * 32 + l31;
            if (n >= p.N) continue;
            float bn = (p.bias_mode == 1 && lead) ? p.bias[n / p.bias_div] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (m >= p.M) continue;
                float v = acc[i][j][r] + bn;
                if (p.bias_mode == 2 && lead) v += p.bias[m];
                gemm_store(p, C + (long)m * p.sCm + (long)n * p.sCn, v);
            }
        }
}

template <int BM, int BN, bool AK, bool BNC>
__global__ __launch_bounds__(256) void gemm_kernel(GemmP p) {
    __shared__ float lds[TileLds<BM, BN>::BYTES / sizeof(float)];
    gemm_tile_body<BM, BN, AK, BNC>(p, lds, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.x, gridDim.y, gridDim.z);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- the same product on the bf16 matrix cores: every fp32 operand split exactly into three bf16 terms, six
// v_mfma_f32_32x32x16_bf16 per fp32 product tile (the arithmetic of conv_x3.hip: dropped terms < 2^-24 of a product).
// 64 x 64 block tile, 4 waves as 2 x 2 (wave tile 32 x 32).  LDS images are bf16 planes:
//   operand contiguous along k in memory   -> [row][k]  (pitch 80 B): a fragment = one ds_read_b128, conflict-free
//   operand contiguous along m / n         -> [k][row]  (pitch 192 B): the fragment is read TRANSPOSED with two
//                                             ds_read_b64_tr_b16 (4 k x 16 rows per 16 lanes, returned k-major per lane)
// so that both memory layouts are staged with 16-byte global loads and 8-byte LDS stores, no shuffles.
typedef __bf16 gx_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 gx_bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int gx_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int gx_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) gx_bf16x4 gx_lds_bf16x4;
// (round 4: two values per conversion / residual instruction - x3_split2, conv_x3.h; the same bits as the scalar form)
__device__ __forceinline__ void gx_split4(const f32x4& v, gx_u32x2 (&out)[3]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        unsigned h, m, l;
        x3_split2(x3_f32x2{v[2 * j], v[2 * j + 1]}, h, m, l);
        out[0][j] = h; out[1][j] = m; out[2][j] = l;
    }
}

template <bool KC>           // KC: the operand is k-contiguous ([row][k] image), else [k][row]
struct GxImg {
    static constexpr int PITCH = KC ? (BK * 2 + 16) : (64 * 2 + 64);
    static constexpr int ROWS = KC ? 64 : BK;            // 64 rows of the tile, or the k of one step
    static constexpr int BYTES = PITCH * ROWS;            // one plane
};

// DEPTH: K steps whose global loads are in flight in registers ahead of the one being multiplied.  The deep variant (3) takes
// 16-byte loads only (vecA && vecB, K range a multiple of 4) and loads UNCONDITIONALLY - out-of-range groups read a valid stand-in
// address and are zeroed when they are stored to LDS - so that the compiler can count the loads in flight (a branch around a load
// forces s_waitcnt vmcnt(0)).  Measured (round 3, profiles/r03_step_trace_no_overlap.txt): -9 ... +7 % per product, -3 us per
// step - these products are bound neither by load latency nor by the operand split but by the L2 / Infinity-Cache traffic of
// 64 x 64 tiles ((64 + 64) K operand elements per 64 * 64 * K multiplications: the 7x7 head's forward moves 205 MB for 32 MB of
// distinct data).  (The one-stage form takes what the 16-byte loads cannot.)
// (the body is a __device__ function of the tile indices and their grid, as gemm_tile_body: the grouped kernel runs it too)
template <bool AK, bool BNC, int DEPTH>
__device__ __forceinline__ void gemm_x3_body(const GemmP& p, unsigned char* __restrict__ gx_lds, unsigned bx, unsigned by, unsigned bz,
                                             unsigned gx, unsigned gy, unsigned gz) {
    using IA = GxImg<AK>;
    using IB = GxImg<!BNC>;
    constexpr int BM = 64, BN = 64, G4 = StageMap<AK, BM>::G;   // float4 groups per thread and operand
    unsigned char* As = gx_lds;                                 // [3 planes][IA::BYTES]
    unsigned char* Bs = gx_lds + 3 * IA::BYTES;                 // [3 planes][IB::BYTES]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int cg = (lane >> 4) & 1, q4 = (lane & 15) >> 2, pp = lane & 3;      // transposed-read roles
    const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 32;
    // XCD-aware tile order: consecutive workgroup ids go round-robin to the 8 XCDs, so the tiles of
    // one (batch, K slice) - which share their A rows and B columns - used to be spread over all eight L2s.  Workgroup
    // w = (xcd, k) takes tile xcd * (tiles / 8) + k of the (z, y, x) order: one XCD works through whole (batch, K slice) planes.
    if (p.xcd) {
        const unsigned lin = (unsigned)xcd_tile(bx + gx * (by + gy * bz), gx * gy * gz);
        bx = lin % gx; by = (lin / gx) % gy; bz = lin / (gx * gy);
    }
    const TileCtx t(p, BM, BN, bx, by, bz);
    const int m0 = t.m0, n0 = t.n0, kbeg = t.kbeg, kend = t.kend;
    const float* A = t.A; const float* B = t.B; float* C = t.C;

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    f32x4 ra[DEPTH][G4], rb[DEPTH][G4];

    // The deep form's (contiguous, other) coordinates of float4 group g of the K step at k0: StageMap's rule written out, with
    // the map's constants.  Read through StageMap::row() / k() the DEPTH = 3 bodies (and only they) come out with another
    // register allocation and other global-load counts, so this one copy stays (profiles/NOTES.md).
    constexpr int QK = StageMap<true, 64>::Q, QR = StageMap<false, 64>::Q;
    auto coordA = [&](int g, int k0, int* fast, int* slow) {
        if (AK) { *fast = k0 + (tid % QK) * 4; *slow = m0 + tid / QK + g * (256 / QK); }          // (k, m)
        else    { *fast = m0 + (tid % QR) * 4; *slow = k0 + tid / QR + g * (256 / QR); }          // (m, k)
    };
    auto coordB = [&](int g, int k0, int* fast, int* slow) {
        if (BNC) { *fast = n0 + (tid % QR) * 4; *slow = k0 + tid / QR + g * (256 / QR); }         // (n, k)
        else     { *fast = k0 + (tid % QK) * 4; *slow = n0 + tid / QK + g * (256 / QK); }         // (k, n)
    };
    auto okA = [&](int fast, int slow) { return AK ? (fast < kend && slow < p.M) : (fast + 3 < p.M && slow < kend); };
    auto okB = [&](int fast, int slow) { return BNC ? (fast + 3 < p.N && slow < kend) : (fast < kend && slow < p.N); };

    auto gload = [&](int st, int k0) {
#pragma unroll
        for (int g = 0; g < G4; ++g) {
            if constexpr (DEPTH > 1) {
                int f, sl;
                coordA(g, k0, &f, &sl);
                const float* sa = AK ? A + (long)sl * p.sAm + f : A + (long)sl * p.sAk + f;
                ra[st][g] = *reinterpret_cast<const f32x4*>(okA(f, sl) ? sa : A);
                coordB(g, k0, &f, &sl);
                const float* sb = BNC ? B + (long)sl * p.sBk + f : B + (long)sl * p.sBn + f;
                rb[st][g] = *reinterpret_cast<const f32x4*>(okB(f, sl) ? sb : B);
                continue;
            }
            ra[st][g] = stage_load<AK, BM, false>(A, p.sAm, p.sAk, p.M, p.vecA, tid, g, m0, k0, kend);
            rb[st][g] = stage_load<!BNC, BN, true>(B, p.sBn, p.sBk, p.N, p.vecB, tid, g, n0, k0, kend);
        }
    };
    auto lstore = [&](int st, int k0) {
#pragma unroll
        for (int g = 0; g < G4; ++g) {
            const StageMap<AK, BM> ma(tid, g);
            const StageMap<!BNC, BN> mb(tid, g);
            f32x4 va = ra[st][g], vb = rb[st][g];
            if constexpr (DEPTH > 1) {               // stand-in loads of out-of-range groups: exact zeros
                int f, sl;
                coordA(g, k0, &f, &sl);
                if (!okA(f, sl)) va = f32x4{0.f, 0.f, 0.f, 0.f};
                coordB(g, k0, &f, &sl);
                if (!okB(f, sl)) vb = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            gx_u32x2 sa[3], sb[3];
            gx_split4(va, sa);
            gx_split4(vb, sb);
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                *reinterpret_cast<gx_u32x2*>(As + pl * IA::BYTES + ma.sl * IA::PITCH + ma.fq * 8) = sa[pl];
                *reinterpret_cast<gx_u32x2*>(Bs + pl * IB::BYTES + mb.sl * IB::PITCH + mb.fq * 8) = sb[pl];
            }
        }
    };
    // fragment of K step ks (16 k) for the wave's 32 rows starting at r0
    auto frag = [&](const unsigned char* img, bool kc, int pitch, int r0, int ks) -> gx_bf16x8 {
        if (kc)
            return __builtin_bit_cast(gx_bf16x8, *reinterpret_cast<const gx_u32x4*>(img + (r0 + l31) * pitch + (ks * 16 + half * 8) * 2));
        const unsigned char* q = img + (ks * 16 + half * 8 + q4) * pitch + (r0 + cg * 16 + pp * 4) * 2;
        const gx_bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((gx_lds_bf16x4*)q);
        const gx_bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((gx_lds_bf16x4*)(q + 4 * pitch));
        return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    };

    auto multiply = [&]() {
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            gx_bf16x8 a[3], b[3];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                a[pl] = frag(As + pl * IA::BYTES, AK, IA::PITCH, wm0, ks);
                b[pl] = frag(Bs + pl * IB::BYTES, !BNC, IB::PITCH, wn0, ks);
            }
            constexpr int APL[6] = {0, 2, 1, 0, 1, 0}, BPL[6] = {2, 0, 1, 1, 0, 0};      // small products first
#pragma unroll
            for (int t = 0; t < 6; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[APL[t]], b[BPL[t]], acc, 0, 0, 0);
        }
    };
    if constexpr (DEPTH > 1) {
        // prologue: DEPTH steps in flight (steps beyond kend load the stand-in address: harmless, never stored)
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) gload(d, kbeg + d * BK);
        // Round 4: the rounds of DEPTH full steps run in a loop WITHOUT branches, the 0 ... DEPTH-1 remaining steps behind it.  With
        // `if (kk < kend)` around every step the loop header was a join of paths with different numbers of loads in flight, and the
        // compiler put s_waitcnt vmcnt(0) in front of the first stage's LDS stores: every third K step waited for the loads that
        // had just been issued for three steps ahead - the deep prefetch was one step deep (tools/e4_probe.py: 37 us for the 7x7
        // head's product, MFMA busy 0.20, and nothing inside the step mattered).
        const int nst = (kend - kbeg + BK - 1) / BK;
        int k0 = kbeg;
        for (int it = 0; it < nst / DEPTH; ++it, k0 += DEPTH * BK) {
#pragma unroll
            for (int d = 0; d < DEPTH; ++d) {
                const int kk = k0 + d * BK;
                __syncthreads();                         // previous tile's fragment reads are done
                lstore(d, kk);
                __syncthreads();
                gload(d, kk + DEPTH * BK);              // stage d is free again: three steps ahead, under the MFMAs below
                multiply();
            }
        }
#pragma unroll
        for (int d = 0; d < DEPTH - 1; ++d) {            // (the loads issued for steps beyond kend read the stand-in address)
            const int kk = k0 + d * BK;
            if (kk < kend) {                             // block-uniform
                __syncthreads();
                lstore(d, kk);
                __syncthreads();
                multiply();
            }
        }
    } else {
        if (kbeg < kend) gload(0, kbeg);
        for (int k0 = kbeg; k0 < kend; k0 += BK) {
            __syncthreads();                 // previous tile's fragment reads are done
            lstore(0, k0);
            __syncthreads();
            if (k0 + BK < kend) gload(0, k0 + BK);   // in flight under the MFMAs below
            multiply();
        }
    }

    // epilogue (as gemm_kernel): D[i][j]: j = lane&31, i = (r&3) + 8*(r>>2) + 4*(lane>>5)
    const bool lead = (t.split == 0) && !(p.flags & 8);
    const int n = n0 + wn0 + l31;
    if (n >= p.N) return;
    const float bn = (p.bias_mode == 1 && lead) ? p.bias[n / p.bias_div] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm0 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (m >= p.M) continue;
        float v = acc[r] + bn;
        if (p.bias_mode == 2 && lead) v += p.bias[m];
        gemm_store(p, C + (long)m * p.sCm + (long)n * p.sCn, v);
    }
}

template <bool AK, bool BNC, int DEPTH = 1>
__global__ __launch_bounds__(256, 4) void gemm_x3_kernel(GemmP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gx_lds[];
    gemm_x3_body<AK, BNC, DEPTH>(p, gx_lds, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.x, gridDim.y, gridDim.z);
}

inline bool gemm_x3_on(int K) {                               // jvae_conv2d_set_split(0): the fp32 matrix-core kernel
    return K >= 64 && jvae_conv5_x3_enabled();
}

// ---- the variants: what a product can run.  The index of a row is the variant number of jvae_gemm_route(); the plan, the LDS
// sizes, the stand-alone launch, the bodies of the grouped kernels and jvae_gemm_variant_name() all read this table.
//   x3 false: gemm_kernel<bm, bm, ak, bnc>            __launch_bounds__(256)
//   x3 true:  gemm_x3_kernel<ak, bnc, depth>          __launch_bounds__(256, 4)
struct Variant {
    bool x3; int bm; bool ak, bnc; int depth;
};
constexpr int NVAR = 16, VAR_X3 = 8;          // VAR_X3: the first split-bf16 variant
constexpr Variant VARIANTS[NVAR] = {
    {false, 64, false, false, 1}, {false, 64, false, true, 1}, {false, 64, true, false, 1}, {false, 64, true, true, 1},
    {false, 128, false, false, 1}, {false, 128, false, true, 1}, {false, 128, true, false, 1}, {false, 128, true, true, 1},
    {true, 64, false, false, 1}, {true, 64, false, false, 3}, {true, 64, false, true, 1}, {true, 64, false, true, 3},
    {true, 64, true, false, 1}, {true, 64, true, false, 3}, {true, 64, true, true, 1}, {true, 64, true, true, 3},
};
constexpr int variant_index(bool x3, int bm, bool ak, bool bnc, int depth) {
    for (int v = 0; v < NVAR; ++v) {
        const Variant& d = VARIANTS[v];
        if (d.x3 == x3 && d.bm == bm && d.ak == ak && d.bnc == bnc && d.depth == depth) return v;
    }
    return -1;
}
// LDS bytes of a workgroup: dynamic for the x3 variants, what the static arrays take for the tile variants
constexpr int variant_lds(int v) {
    const Variant& d = VARIANTS[v];
    if (!d.x3) return d.bm == 128 ? TileLds<128, 128>::BYTES : TileLds<64, 64>::BYTES;
    return 3 * ((d.ak ? GxImg<true>::BYTES : GxImg<false>::BYTES) + (d.bnc ? GxImg<false>::BYTES : GxImg<true>::BYTES));
}
// the largest of the variants in `set` (bit v = variant v)
constexpr int set_lds(unsigned set) {
    int lds = 0;
    for (int v = 0; v < NVAR; ++v)
        if (((set >> v) & 1u) && variant_lds(v) > lds) lds = variant_lds(v);
    return lds;
}
// f(std::integral_constant<int, V>{}) for the variant v (the idiom of jvae_with_aff, jvae_internal.h)
template <class F, int... V>
inline void with_variant_seq(int v, F&& f, std::integer_sequence<int, V...>) {
    ((v == V ? (f(std::integral_constant<int, V>{}), 0) : 0), ...);
}
template <class F>
inline void with_variant(int v, F&& f) { with_variant_seq(v, f, std::make_integer_sequence<int, NVAR>{}); }

// ---- plan: what one product runs - its GemmP, the variant and the grid.  The single-product entries and the grouped entry
// take it from gemm_plan() alone, so a product cannot get another kernel, tile or K slicing because it shares a launch.
// jvae_gemm_route() (at the end of the file) reports this plan without launching.
struct GemmPlan {
    GemmP p;
    int variant;
    unsigned gx, gy, gz;     // the grid of the stand-alone launch = the virtual grid of the record in a group
    int lds;                 // variant_lds(variant)
};

// The plan of one descriptor (jvae_hip.h: JvaeGemmDesc; want_splits > 0 = the stored-slices form: partial products sCsplit apart,
// no bias, splitk = the wanted number, and it has to report its count) and the one argument that only the internal entry has.
// 0: *pl is a launch; 1: nothing to do (an empty product); < 0: invalid.  pl->p.splitk is the number of K slices made.
int gemm_plan(const JvaeGemmDesc& a, int bias_div, GemmPlan* pl) {
    const bool part = a.want_splits > 0;
    if (a.M <= 0 || a.N <= 0 || a.batch <= 0) return 1;
    if (!a.A || !a.B || !a.C) return JVAE_EINVAL;
    if (part ? a.K <= 0 : a.K < 0) return JVAE_EINVAL;
    if (!part && a.bias_mode && !a.bias) return JVAE_EINVAL;
    GemmP& p = pl->p;
    p.A = a.A; p.sAm = a.sAm; p.sAk = a.sAk; p.sAb = a.sAb;
    p.B = a.B; p.sBk = a.sBk; p.sBn = a.sBn; p.sBb = a.sBb;
    p.C = a.C; p.sCm = a.sCm; p.sCn = a.sCn; p.sCb = a.sCb;
    p.bias = part ? nullptr : a.bias;
    p.bias_mode = part ? 0 : a.bias_mode;
    p.bias_div = (!part && bias_div > 0) ? bias_div : 1;
    p.M = a.M; p.N = a.N; p.K = a.K;
    int splitk = part ? a.want_splits : (a.splitk < 1 ? 1 : a.splitk);
    const int ktiles = cdiv(a.K, BK);
    if (splitk > ktiles) splitk = ktiles > 0 ? ktiles : 1;
    p.kchunk = cdiv(ktiles, splitk) * BK;
    splitk = a.K > 0 ? cdiv(a.K, p.kchunk) : 1;
    p.splitk = splitk;
    if (part) {
        p.flags = 8;
        p.sCsplit = a.sCsplit;
    } else {
        p.flags = a.flags & ~8;
        p.sCsplit = 0;
        if (splitk > 1) {
            if (a.flags & 2) return JVAE_EINVAL;      // ReLU cannot follow a partial sum
            p.flags |= 4;                             // caller pre-zeroes C (or wants accumulation)
        }
    }
    // vector loads: contiguous direction has unit stride, everything else keeps 16-byte alignment
    const bool ak = (a.sAk == 1), bnc = (a.sBn == 1);
    p.vecA = aligned16(a.A) && (a.sAb % 4 == 0) && (ak ? (a.sAm % 4 == 0) : (a.sAm == 1 && a.sAk % 4 == 0));
    p.vecB = aligned16(a.B) && (a.sBb % 4 == 0) && (bnc ? (a.sBk % 4 == 0) : (a.sBk == 1 && a.sBn % 4 == 0));
    p.xcd = 0;
    int bm = 64;
    if (gemm_x3_on(a.K)) {
        p.xcd = 1;                                                 // XCD-aware tile order
        // deep prefetch: 16-byte loads on both operands, K range a multiple of 4 (kchunk is a multiple of 32)
        const bool deep = p.vecA && p.vecB && p.K % 4 == 0 && (ak || p.M % 4 == 0) && (!bnc || p.N % 4 == 0);
        pl->variant = variant_index(true, 64, ak, bnc, deep ? 3 : 1);
    } else {
        const long tiles128 = (long)cdiv(a.M, 128) * cdiv(a.N, 128) * a.batch * splitk;
        if (!part && a.M > 64 && a.N > 64 && tiles128 >= 512) bm = 128;
        pl->variant = variant_index(false, bm, ak, bnc, 1);
    }
    pl->gx = cdiv(a.N, bm); pl->gy = cdiv(a.M, bm); pl->gz = (unsigned)a.batch * splitk;
    pl->lds = variant_lds(pl->variant);
    return part && !a.splits ? JVAE_EINVAL : 0;
}

template <typename F>
int set_lds_once(F kernel, int lds, bool* done) {
    if (!*done) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return (int)e;
        *done = true;
    }
    return 0;
}

template <int V>
int launch_variant(const GemmPlan& pl, hipStream_t st) {
    constexpr Variant d = VARIANTS[V];
    if constexpr (d.x3) {
        static bool attr_set = false;
        if (int rc = set_lds_once(&gemm_x3_kernel<d.ak, d.bnc, d.depth>, variant_lds(V), &attr_set)) return rc;
        hipLaunchKernelGGL((gemm_x3_kernel<d.ak, d.bnc, d.depth>), dim3(pl.gx, pl.gy, pl.gz), dim3(256), pl.lds, st, pl.p);
    } else {
        hipLaunchKernelGGL((gemm_kernel<d.bm, d.bm, d.ak, d.bnc>), dim3(pl.gx, pl.gy, pl.gz), dim3(256), 0, st, pl.p);
    }
    JVAE_LAUNCH_CHECK();
    return 0;
}

int launch_plan(const GemmPlan& pl, hipStream_t st) {
    int rc = JVAE_EINVAL;
    with_variant(pl.variant, [&](auto V) { rc = launch_variant<decltype(V)::value>(pl, st); });
    return rc;
}

// ---- grouped launch: up to JVAE_GEMM_GROUP_MAX independent products in ONE flat grid.  The records travel by value in the kernel
// arguments (as PackTable does): nothing to upload, safe under graph capture.  A workgroup finds its record from blockIdx.x
// (uniform over the workgroup) and runs that variant's body with the record's own virtual grid.  Every record starts at a
// multiple of 8 workgroups, so that the XCD a workgroup runs on (flat id % 8) is the one xcd_tile() assumes for its tile; the
// few workgroups of the padding return at once.
// Which variants may share a launch: those with equal __launch_bounds__ - the eight gemm_kernel variants one launch
// (gemm_group_tile_kernel), the eight gemm_x3_kernel variants another (gemm_group_x3_kernel).  A group that holds both kinds is
// two launches.
constexpr int GROUP_MAX = 8;
struct GemmRec {
    GemmP p;
    int variant;
    unsigned gx, gy, gz;
    unsigned first;          // first flat workgroup of the record (a multiple of 8); 0xffffffff in unused records
};
struct GemmGroup {
    GemmRec rec[GROUP_MAX];
};

// The record of this flat workgroup and the workgroup's index within it (GemmGroup, FoldGroup: records with a `first`).
template <class G>
__device__ __forceinline__ unsigned group_record(const G& g, unsigned* local) {
    unsigned r = 0;
#pragma unroll
    for (unsigned i = 1; i < GROUP_MAX; ++i)
        if (blockIdx.x >= g.rec[i].first) r = i;
    *local = blockIdx.x - g.rec[r].first;
    return r;
}
// The unused records of a group with cnt >= 1 records: copies of record 0 that no workgroup reaches.
template <class G>
void pad_records(G* g, int cnt) {
    for (int i = cnt; i < GROUP_MAX; ++i) { g->rec[i] = g->rec[0]; g->rec[i].first = 0xffffffffu; }
}

struct GroupTile { unsigned r, bx, by, bz; bool live; };
__device__ __forceinline__ GroupTile group_tile(const GemmGroup& g) {
    unsigned local;
    GroupTile t;
    t.r = group_record(g, &local);
    const GemmRec& rc = g.rec[t.r];
    t.live = local < rc.gx * rc.gy * rc.gz;
    t.bx = local % rc.gx; t.by = (local / rc.gx) % rc.gy; t.bz = local / (rc.gx * rc.gy);
    return t;
}

// The body of variant V, when it is in SET (bit v = variant v is compiled in) and the record asks for it: true if it ran.  The
// grouped kernels run these as consecutive tests: behind one `switch` the split-bf16 bodies spilled.  STOP: no test after the one
// that ran.  The tile kernel stops (without, its 64 x 64 form takes 50 VGPRs and loses a wave per SIMD), the split-bf16 kernel
// does not (with, it spills one to seven VGPRs more): profiles/NOTES.md.
template <unsigned SET, int V>
__device__ __forceinline__ bool group_case(const GemmRec& rc, unsigned char* lds, const GroupTile& t) {
    constexpr Variant d = VARIANTS[V];
    if constexpr ((SET >> V) & 1u) {
        if (rc.variant == V) {
            if constexpr (d.x3) gemm_x3_body<d.ak, d.bnc, d.depth>(rc.p, lds, t.bx, t.by, t.bz, rc.gx, rc.gy, rc.gz);
            else gemm_tile_body<d.bm, d.bm, d.ak, d.bnc>(rc.p, reinterpret_cast<float*>(lds), t.bx, t.by, t.bz, rc.gx, rc.gy, rc.gz);
            return true;
        }
    }
    return false;
}
template <unsigned SET, bool STOP, int... V>
__device__ __forceinline__ void group_cases(const GemmGroup& g, unsigned char* lds, std::integer_sequence<int, V...>) {
    const GroupTile t = group_tile(g);
    if (!t.live) return;
    if constexpr (STOP) (void)(group_case<SET, V>(g.rec[t.r], lds, t) || ...);
    else (group_case<SET, V>(g.rec[t.r], lds, t), ...);
}

// BIG: the 128 x 128 variants are compiled in.  They take 76-80 VGPRs + 64 AGPRs (occupancy 3) where the 64 x 64 variants take
// 38-42 + 16 (occupancy 8), so a group of 64 x 64 tiles only has a kernel of its own.
constexpr unsigned tile_set(bool big) {
    unsigned set = 0;
    for (int v = 0; v < VAR_X3; ++v)
        if (big || VARIANTS[v].bm == 64) set |= 1u << v;
    return set;
}
template <bool BIG>
__global__ __launch_bounds__(256) void gemm_group_tile_kernel(GemmGroup g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char grp_lds[];
    group_cases<tile_set(BIG), true>(g, grp_lds, std::make_integer_sequence<int, NVAR>{});
}

// MASK: bit (variant - VAR_X3) set = that variant's body is compiled in.  The union of all eight takes the registers of its largest
// member (128 VGPRs, three of them spilled; occupancy 4 as every DEPTH = 3 variant has alone), so the variant sets the training
// step uses have kernels of their own, which build to their members' counts: the two forward products of a pair of linear
// layers (X3_FWD) and the dgrads and weight gradients of linear layers (X3_BWD).  Any other set takes the union.
constexpr unsigned x3_bit(bool ak, bool bnc, int depth) { return 1u << (variant_index(true, 64, ak, bnc, depth) - VAR_X3); }
constexpr unsigned X3_FWD = x3_bit(true, false, 3), X3_BWD = x3_bit(true, true, 3) | x3_bit(false, true, 3), X3_ALL = 0xffu;

template <unsigned MASK>
__global__ __launch_bounds__(256, 4) void gemm_group_x3_kernel(GemmGroup g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char grp_lds[];
    group_cases<(MASK << VAR_X3), false>(g, grp_lds, std::make_integer_sequence<int, NVAR>{});
}

// One grouped kernel, compiled for the variants in SET: its dynamic-LDS limit is that of the largest of them.
template <unsigned SET, class K>
int launch_group_set(K kernel, const GemmGroup& g, unsigned total, int lds, hipStream_t st) {
    static bool attr_set = false;
    if (int rc = set_lds_once(kernel, set_lds(SET), &attr_set)) return rc;
    hipLaunchKernelGGL(kernel, dim3(total), dim3(256), lds, st, g);
    JVAE_LAUNCH_CHECK();
    return 0;
}
template <bool BIG>
int launch_group_tile(const GemmGroup& g, unsigned total, int lds, hipStream_t st) {
    return launch_group_set<tile_set(BIG)>(&gemm_group_tile_kernel<BIG>, g, total, lds, st);
}
template <unsigned MASK>
int launch_group_x3(const GemmGroup& g, unsigned total, int lds, hipStream_t st) {
    return launch_group_set<(MASK << VAR_X3)>(&gemm_group_x3_kernel<MASK>, g, total, lds, st);
}

// The plans of one kind (x3 or tile variants) as one launch; a single plan goes through the stand-alone kernel.
int launch_group_kind(const GemmPlan* plans, int n, bool x3, hipStream_t st) {
    GemmGroup g;
    int cnt = 0, lds = 0, last = -1;
    unsigned set = 0;
    unsigned long total = 0;
    for (int i = 0; i < n; ++i) {
        if (VARIANTS[plans[i].variant].x3 != x3) continue;
        GemmRec& rc = g.rec[cnt++];
        rc.p = plans[i].p; rc.variant = plans[i].variant;
        rc.gx = plans[i].gx; rc.gy = plans[i].gy; rc.gz = plans[i].gz;
        rc.first = (unsigned)total;
        total += ((unsigned long)rc.gx * rc.gy * rc.gz + 7) & ~7ul;
        if (total > 0x7fffffffUL) return JVAE_ENOTSUP;
        if (plans[i].lds > lds) lds = plans[i].lds;
        set |= 1u << rc.variant;
        last = i;
    }
    if (cnt == 0) return 0;
    if (cnt == 1) return launch_plan(plans[last], st);
    pad_records(&g, cnt);
    if (x3) {
        const unsigned mask = set >> VAR_X3;
        if ((mask & ~X3_FWD) == 0) return launch_group_x3<X3_FWD>(g, (unsigned)total, lds, st);
        if ((mask & ~X3_BWD) == 0) return launch_group_x3<X3_BWD>(g, (unsigned)total, lds, st);
        return launch_group_x3<X3_ALL>(g, (unsigned)total, lds, st);
    }
    if (set & ~tile_set(false)) return launch_group_tile<true>(g, (unsigned)total, lds, st);
    return launch_group_tile<false>(g, (unsigned)total, lds, st);
}

int launch_group(const GemmPlan* plans, int n, hipStream_t st) {
    if (int rc = launch_group_kind(plans, n, true, st)) return rc;
    return launch_group_kind(plans, n, false, st);
}

// [lo, hi] byte range a plan's product may write (a hull: strided outputs that interleave count as overlapping)
void plan_out_range(const GemmPlan& pl, uintptr_t* lo, uintptr_t* hi) {
    const GemmP& p = pl.p;
    const long batch = pl.gz / p.splitk;
    long neg = 0, pos = 0;
    auto span = [&](long stride, long count) {
        const long d = stride * (count - 1);
        if (d < 0) neg += d; else pos += d;
    };
    span(p.sCm, p.M); span(p.sCn, p.N); span(p.sCb, batch);
    if (p.flags & 8) span(p.sCsplit, p.splitk);
    *lo = reinterpret_cast<uintptr_t>(p.C + neg);
    *hi = reinterpret_cast<uintptr_t>(p.C + pos) + sizeof(float) - 1;
}

// Plan, then launch: one product alone.  *d.splits (where the caller wants it) is the number of K slices made, 0 if none was.
int plan_and_launch(const JvaeGemmDesc& d, int bias_div, hipStream_t st) {
    if (d.splits) *d.splits = 0;
    GemmPlan pl;
    const int rc = gemm_plan(d, bias_div, &pl);
    if (rc) return rc < 0 ? rc : 0;
    if (d.splits) *d.splits = pl.p.splitk;
    return launch_plan(pl, st);
}

}  // namespace

int jvae_gemm_launch(int M, int N, int K, int batch,
                     const float* A, long sAm, long sAk, long sAb,
                     const float* B, long sBk, long sBn, long sBb,
                     float* C, long sCm, long sCn, long sCb,
                     const float* bias, int bias_mode, int flags, int splitk, hipStream_t st) {
    return jvae_gemm_launch_ex(M, N, K, batch, A, sAm, sAk, sAb, B, sBk, sBn, sBb, C, sCm, sCn, sCb, bias, bias_mode, 1,
                               flags, splitk, st);
}

// Internal entry used by the other translation units (see jvae_internal.h).
int jvae_gemm_launch_ex(int M, int N, int K, int batch,
                        const float* A, long sAm, long sAk, long sAb,
                        const float* B, long sBk, long sBn, long sBb,
                        float* C, long sCm, long sCn, long sCb,
                        const float* bias, int bias_mode, int bias_div, int flags, int splitk, hipStream_t st) {
    JvaeGemmDesc d = {};
    d.M = M; d.N = N; d.K = K; d.batch = batch;
    d.A = A; d.sAm = sAm; d.sAk = sAk; d.sAb = sAb;
    d.B = B; d.sBk = sBk; d.sBn = sBn; d.sBb = sBb;
    d.C = C; d.sCm = sCm; d.sCn = sCn; d.sCb = sCb;
    d.bias = bias; d.bias_mode = bias_mode; d.flags = flags; d.splitk = splitk;
    return plan_and_launch(d, bias_div, st);
}

// Deterministic split-K: K is cut into *splits pieces whose partial products are STORED side by side (part + s*sCsplit,
// same strides as C); no atomics, no bias.  Fold them with jvae_splitk_fold.  Returns the number of pieces in *splits.
int jvae_gemm_launch_part(int M, int N, int K, int batch,
                          const float* A, long sAm, long sAk, long sAb,
                          const float* B, long sBk, long sBn, long sBb,
                          float* part, long sCm, long sCn, long sCb, long sCsplit, int want_splits, int* splits,
                          hipStream_t st) {
    JvaeGemmDesc d = {};
    d.M = M; d.N = N; d.K = K; d.batch = batch;
    d.A = A; d.sAm = sAm; d.sAk = sAk; d.sAb = sAb;
    d.B = B; d.sBk = sBk; d.sBn = sBn; d.sBb = sBb;
    d.C = part; d.sCm = sCm; d.sCn = sCn; d.sCb = sCb;
    d.want_splits = want_splits < 1 ? 1 : want_splits; d.sCsplit = sCsplit; d.splits = splits;
    return plan_and_launch(d, 1, st);
}

// Plans for n <= 8 descriptors (jvae_hip.h: JvaeGemmDesc), checked as a whole before anything is launched: an invalid descriptor or
// two outputs that overlap return JVAE_EINVAL, more than 8 JVAE_ENOTSUP.  Empty products are dropped.
extern "C" int jvae_gemm_group_f32(const JvaeGemmDesc* descs, int n, void* stream) {
    if (n == 0) return 0;
    if (n < 0 || !descs) return JVAE_EINVAL;
    if (n > GROUP_MAX) return JVAE_ENOTSUP;
    GemmPlan plans[GROUP_MAX];
    uintptr_t lo[GROUP_MAX], hi[GROUP_MAX];
    int* splits[GROUP_MAX];
    int cnt = 0;
    for (int i = 0; i < n; ++i) {
        const JvaeGemmDesc& d = descs[i];
        if (d.splits) *d.splits = 0;
        const int rc = gemm_plan(d, 1, &plans[cnt]);
        if (rc < 0) return rc;
        if (rc) continue;
        plan_out_range(plans[cnt], &lo[cnt], &hi[cnt]);
        for (int j = 0; j < cnt; ++j)
            if (lo[cnt] <= hi[j] && lo[j] <= hi[cnt]) return JVAE_EINVAL;
        splits[cnt++] = d.splits;
    }
    // (the numbers of slices are reported only once the whole group is known to be valid)
    for (int k = 0; k < cnt; ++k)
        if (splits[k]) *splits[k] = plans[k].p.splitk;
    return launch_group(plans, cnt, (hipStream_t)stream);
}

// y[i] = [relu](bias[i % N] + sum_s part[s][i]) in a fixed order: the deterministic second half of a split-K product
// whose S partial products were written side by side by a batched launch (batch = K slices).  `block` of `blocks`: the
// workgroup's place in the job's own grid (the hardware's in the stand-alone kernel, the record's in the grouped one).
__device__ __forceinline__ void splitk_fold_body(const float* __restrict__ part, const float* __restrict__ bias, float* __restrict__ y,
                                                 int S, long MN, int N, int relu, int accumulate, int bias_div, unsigned block,
                                                 unsigned blocks) {
    for (long i = (long)block * blockDim.x + threadIdx.x; i < MN; i += (long)blocks * blockDim.x) {
        float v = bias ? bias[(i / bias_div) % N] : 0.f;
        for (int s = 0; s < S; ++s) v += part[(long)s * MN + i];
        if (accumulate) v += y[i];
        y[i] = relu ? fmaxf(v, 0.f) : v;
    }
}

__global__ __launch_bounds__(256) void splitk_fold_kernel(const float* __restrict__ part, const float* __restrict__ bias,
                                                          float* __restrict__ y, int S, long MN, int N, int relu,
                                                          int accumulate, int bias_div) {
    splitk_fold_body(part, bias, y, S, MN, N, relu, accumulate, bias_div, blockIdx.x, gridDim.x);
}

// Up to 8 such folds in one flat grid: the records by value in the kernel arguments, as GemmGroup.
struct FoldRec {
    const float* part; const float* bias; float* y;
    long MN;
    int S, N, relu, accumulate, bias_div;
    unsigned first, blocks;      // first flat workgroup (0xffffffff: unused record) and the job's own grid
};
struct FoldGroup {
    FoldRec rec[GROUP_MAX];
};

__global__ __launch_bounds__(256) void splitk_fold_group_kernel(FoldGroup g) {
    unsigned local;
    const FoldRec& rc = g.rec[group_record(g, &local)];
    splitk_fold_body(rc.part, rc.bias, rc.y, rc.S, rc.MN, rc.N, rc.relu, rc.accumulate, rc.bias_div, local, rc.blocks);
}

// the grid of a fold (and of the fold below) over `elems` elements
inline int fold_blocks(long elems) { return (int)((elems + 255) / 256 > 4096 ? 4096 : (elems + 255) / 256); }

// The same for partial products stored [slice][position q][image n][channel cs] - rows of cs: the product's lanes run along cs, so its
// stores are 128-byte segments; in the OUTPUT's own layout [n][cs][q] they were 4-byte stores 4 * Ps bytes apart (26 MB of
// partial-sector writes for 6.5 MB of partial products, ~6 of the 36 us of the 7x7 head's forward product) - folded into
// y[n][cs][q] = bias[cs] + sum_s part[s][q][n][cs]: coalesced reads, the small output written with the stride.
__global__ __launch_bounds__(256) void splitk_fold_qn_kernel(const float* __restrict__ part, const float* __restrict__ bias,
                                                             float* __restrict__ y, int S, int N, int Cs, int Ps) {
    const long total = (long)Ps * N * Cs;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int cs = (int)(i % Cs);
        const long r = i / Cs;
        const int n = (int)(r % N), q = (int)(r / N);
        float v = bias ? bias[cs] : 0.f;
        for (int s = 0; s < S; ++s) v += part[(long)s * total + i];
        y[((long)n * Cs + cs) * Ps + q] = v;
    }
}

int jvae_splitk_fold_qn(const float* part, const float* bias, float* y, int S, int N, int Cs, int Ps, hipStream_t st) {
    const long total = (long)Ps * N * Cs;
    if (total == 0) return 0;
    hipLaunchKernelGGL(splitk_fold_qn_kernel, dim3(fold_blocks(total)), dim3(256), 0, st, part, bias, y, S, N, Cs, Ps);
    JVAE_LAUNCH_CHECK();
    return 0;
}

int jvae_splitk_fold(const float* part, const float* bias, float* y, int S, long MN, int N, int relu, int accumulate,
                     hipStream_t st, int bias_div) {
    if (MN == 0) return 0;
    hipLaunchKernelGGL(splitk_fold_kernel, dim3(fold_blocks(MN)), dim3(256), 0, st, part, bias, y, S, MN, N, relu, accumulate,
                       bias_div > 0 ? bias_div : 1);
    JVAE_LAUNCH_CHECK();
    return 0;
}

extern "C" int jvae_splitk_fold_f32(const float* part, const float* bias, float* y, int S, long MN, int N, int relu,
                                    int accumulate, void* stream) {
    if (!part || !y || S < 1 || MN < 0 || N < 1) return JVAE_EINVAL;
    return jvae_splitk_fold(part, bias, y, S, MN, N, relu, accumulate, (hipStream_t)stream);
}

extern "C" int jvae_splitk_fold_group_f32(const JvaeFoldDesc* descs, int n, void* stream) {
    if (n == 0) return 0;
    if (n < 0 || !descs) return JVAE_EINVAL;
    if (n > GROUP_MAX) return JVAE_ENOTSUP;
    FoldGroup g;
    int cnt = 0, last = -1;
    unsigned total = 0;
    for (int i = 0; i < n; ++i) {
        const JvaeFoldDesc& d = descs[i];
        if (!d.part || !d.y || d.S < 1 || d.MN < 0 || d.N < 1) return JVAE_EINVAL;
        for (int j = 0; j < i; ++j) {            // outputs of one launch must not overlap
            const JvaeFoldDesc& e = descs[j];
            if (d.MN > 0 && e.MN > 0 && d.y < e.y + e.MN && e.y < d.y + d.MN) return JVAE_EINVAL;
        }
        if (d.MN == 0) continue;
        FoldRec& rc = g.rec[cnt++];
        rc.part = d.part; rc.bias = d.bias; rc.y = d.y; rc.MN = d.MN;
        rc.S = d.S; rc.N = d.N; rc.relu = d.relu; rc.accumulate = d.accumulate; rc.bias_div = 1;
        rc.first = total; rc.blocks = (unsigned)fold_blocks(d.MN);
        total += rc.blocks;
        last = i;
    }
    if (cnt == 0) return 0;
    if (cnt == 1) {
        const JvaeFoldDesc& d = descs[last];
        return jvae_splitk_fold(d.part, d.bias, d.y, d.S, d.MN, d.N, d.relu, d.accumulate, (hipStream_t)stream);
    }
    pad_records(&g, cnt);
    hipLaunchKernelGGL(splitk_fold_group_kernel, dim3(total), dim3(256), 0, (hipStream_t)stream, g);
    JVAE_LAUNCH_CHECK();
    return 0;
}

extern "C" int jvae_gemm_f32(int M, int N, int K, int batch,
                             const float* A, long sAm, long sAk, long sAb,
                             const float* B, long sBk, long sBn, long sBb,
                             float* C, long sCm, long sCn, long sCb,
                             const float* bias, int bias_mode, int flags, int splitk, void* stream) {
    return jvae_gemm_launch(M, N, K, batch, A, sAm, sAk, sAb, B, sBk, sBn, sBb, C, sCm, sCn, sCb,
                            bias, bias_mode, flags, splitk, (hipStream_t)stream);
}

// Host-only: the plan the launch entries take for this descriptor.  Nothing is launched, the operands are not read.
extern "C" int jvae_gemm_route(const JvaeGemmDesc* d, JvaeGemmRoute* out) {
    if (!d || !out) return JVAE_EINVAL;
    *out = JvaeGemmRoute{-1, 0, 0, 0, 0, 0, 0, 0, 0};
    GemmPlan pl;
    const int rc = gemm_plan(*d, 1, &pl);
    if (rc) return rc < 0 ? rc : 0;
    *out = JvaeGemmRoute{pl.variant, (int)pl.gx, (int)pl.gy, (int)pl.gz, pl.p.splitk, pl.p.kchunk, pl.p.vecA, pl.p.vecB, pl.lds};
    return 0;
}

// "TILE64_AM_BK" ... "X3_AK_BN_D3" (jvae_hip.h), spelled from the table
extern "C" const char* jvae_gemm_variant_name(int variant) {
    struct Names {
        char s[NVAR][16];
        Names() {
            for (int v = 0; v < NVAR; ++v) {
                const Variant& d = VARIANTS[v];
                const char *a = d.ak ? "AK" : "AM", *b = d.bnc ? "BN" : "BK";
                if (d.x3) snprintf(s[v], sizeof s[v], "X3_%s_%s_D%d", a, b, d.depth);
                else snprintf(s[v], sizeof s[v], "TILE%d_%s_%s", d.bm, a, b);
            }
        }
    };
    static const Names names;
    return (variant >= 0 && variant < NVAR) ? names.s[variant] : nullptr;
}
