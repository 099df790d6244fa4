// fp32 5x5 convolution on the bf16 matrix cores by 3-way operand splitting ("x3").
//
//   out[n][o][y][x] = bias[o] + sum_{c,kh,kw} in[n][c][y*S + kh - P][x*S + kw - P] * W[c][kh*5+kw][o]
//
// Same operator, tensors (fp32 NCHW in, fp32 NCHW out) and weight roles (swap / flip) as conv_mfma.hip; only the
// arithmetic unit differs.  v_mfma_f32_32x32x2_f32 retires 64 FLOP/cycle/SIMD (157 TFLOP/s per MI355X),
// v_mfma_f32_32x32x16_bf16 1024 (2.5 PFLOP/s).  Every fp32 operand is written EXACTLY as a sum of three bf16 numbers
//      v = hi + mid + lo,   hi = bf16(v), mid = bf16(v - hi), lo = bf16(v - hi - mid)      (8 + 8 + 8 significand bits)
// and a product x*w is accumulated (fp32 accumulators inside the MFMA) from the six partial products whose weight is
// >= 2^-24 of the full one: x_lo w_hi, x_hi w_lo, x_mid w_mid, x_mid w_hi, x_hi w_mid, x_hi w_hi.  Products of bf16
// numbers are exact in fp32, the three dropped terms are <= 2^-24 |x w|: the result differs from an fp32 FMA chain
// by less than that chain's own rounding (measured against an fp64 convolution on wide-dynamic-range data: 3-15e-7 of the
// output scale for the fp32-MFMA kernel, 2-13e-7 for this one: both are the fp32 ACCUMULATION; tests/test_ops_gpu.py).  Six bf16 MFMAs cover K = 16 in 6*32 = 192 cycles, the fp32 MFMA needs
// 8*64 = 512: the fp32-equivalent ceiling is 2.5 PFLOP/s / 6 = 417 TFLOP/s.
//
// Mapping (one workgroup = 4 waves = MT*128 output pixels x 32 output channels, K step = 16 input channels):
//  * the input patch (with zero halo) is loaded as fp32 NCHW rows (8-byte loads, 2 pixels x 8 channels per thread),
//    the deferred BatchNorm(+ReLU) of conv_mfma.hip is applied in registers, the value is split and stored as three
//    planes of 16-byte units (8 channels of one pixel = one lane's MFMA operand): every fragment read is one
//    ds_read_b128 at lane offset + immediate;
//  * weights are split once per call by the re-pack kernel ([K step][kernel row][plane][kw][half][o] units) and
//    staged per KERNEL ROW (5 taps, 15 KB) into a double-buffered LDS area: one barrier per 60 MFMAs, two workgroups
//    per CU (77 KB each);
//  * accumulators, bias, BatchNorm partial sums and the coalesced NCHW epilogue are those of the fp32 kernel.
// Default since round 4 (maps up to 32 wide): the 16x16x32 form (template argument SH) - K = 2 consecutive taps x 16 channels per
// MFMA, a wave-uniform channel block per staging item (the deferred BatchNorm's coefficients are scalar operands), two tiles per
// workgroup on the large launches.  Since round 6 its weights are NOT staged in LDS: they are packed in fragment order, every wave
// loads its six 16-byte units of a tap pair from global memory (L1 / L2) straight into the fragment registers, one pair ahead,
// and the 13 pairs of a K step run without a barrier - one LDS barrier pair per K step is left, around the patch restage
// (77 KB -> 59 KB of LDS per workgroup).  See the comments at pairStep, lstoreX and the tile loop, and DESIGN.md section 4.
#include <stdlib.h>
#include "common.h"
#include "jvae_internal.h"
#include "conv_dispatch.h"
#include "conv_x3.h"
#include <type_traits>
#include "pack_elems.h"
#include "conv_stats.h"

namespace {

typedef x3_bf16x8 bf16x8;
typedef x3_u32x4 u32x4;
typedef x3_f32x2 f32x2;

// Wp[(kb*5 + kh)][(plane*5 + kw)*2 + half][o][ci] = plane(W[o][c = kb*16 + half*8 + ci][tap = kh*5 + kw])  (o < OP)
// swap: source is [c][o][tap] (ConvTranspose2d layout / role swap), flip: tap -> 24 - tap
__global__ __launch_bounds__(256) void x3_wpack_kernel(const float* __restrict__ w, __bf16* __restrict__ wp,
                                                       int C, int O, int KB, int OP, int swap, int flip) {
    const long total = (long)KB * 25 * 2 * OP * 8;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x)
        jvae_pack_x3_elem(w, wp, i, C, O, swap, flip);
}

__global__ __launch_bounds__(256) void x3s_wpack_kernel(const float* __restrict__ w, __bf16* __restrict__ wp,
                                                        int C, int O, long total, int swap, int flip) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x)
        jvae_pack_x3s_elem(w, wp, i, C, O, swap, flip);
}

struct X3P {
    const float* in;     // (N, Cin, H, W) fp32
    const u32x4* wp;     // packed split weights: (KB*5, 30, OP) units | 16x16x32 form: (KB*14 pairs, 3 planes, 4 lane groups, OP)
    const float* bias;   // (CoutReal) or null
    float* out;          // (N, CoutReal, OH, OW) fp32
    int N, Cin, H, W, OP, P, CoutReal;
    float* stats;        // optional (CoutReal, gridDim.x, 2)
    InAff aff;           // deferred BatchNorm(+ReLU) of the input (sc == nullptr: none)
    int tpw;             // tiles per workgroup (16x16x32 form: 1, or 2 = tiles w and w + gridDim.x; gridDim.x * tpw = number of tiles)
#ifdef JVAE_X3_STAMPS
    unsigned long long* dbg;   // DIAGNOSTIC BUILD ONLY (tools/x3_stamps.py): 96 s_memtime stamps of wave 0 per workgroup
#endif
};

// In-kernel anatomy (cdna_hip_programming.md section 7, In-kernel stamps): a separate diagnostic build (-DJVAE_X3_STAMPS, make stamps)
// records s_memtime at the phase boundaries of wave 0 of every workgroup into a buffer of its own; the product build contains
// no stamp.
#ifdef JVAE_X3_STAMPS
#define X3_STAMP(i)                                                                                              \
    do {                                                                                                         \
        if (p.dbg && threadIdx.x == 0)                                                                           \
            p.dbg[((long)blockIdx.y * gridDim.x + blockIdx.x) * 96 + (i)] = __builtin_amdgcn_s_memtime();        \
    } while (0)
#define X3_STAMP_RT(i)                                                                                           \
    do {                                                                                                         \
        if (p.dbg && threadIdx.x == 0)                                                                           \
            p.dbg[((long)blockIdx.y * gridDim.x + blockIdx.x) * 96 + (i)] = __builtin_amdgcn_s_memrealtime();    \
    } while (0)
#else
#define X3_STAMP(i) do {} while (0)
#define X3_STAMP_RT(i) do {} while (0)
#endif

// SH = false: v_mfma_f32_32x32x16_bf16, K index = 16 channels of one tap, weights staged per kernel row (5 taps).
// SH = true:  v_mfma_f32_16x16x32_bf16, K index = 2 CONSECUTIVE taps (of the 25-tap sequence) x 16 channels - lane group
//             kq = lane >> 4 supplies tap 2*pair + (kq >> 1), channel block kq & 1 - weights staged per GROUP of 2 tap pairs
//             (7 groups per K step: 12 pairs + tap 24 with an all-zero partner; pack_elems.h JVAE_PACK_X3S).  Same output tile
//             per wave, same patch image, same LDS reads per MFMA cycle; 4 % more MFMA cycles (the empty half pair).  The chip
//             holds a higher clock on this shape (MI355X_MICROARCH.md, DVFS give-back item 7).
//             (A stride-2 variant of this form on a de-interleaved 64-pixel patch was built in round 4, never beat the fp32 kernel and
//             left the tree in round 5: profiles/NOTES.md.)
template <int S, int OW, int MT, bool SH = false>
struct X3Geom {
    static constexpr int OH = OW;
    static constexpr int PIX = MT * 128;
    static constexpr int OHW = OH * OW;
    static constexpr int NIMG = PIX >= OHW ? PIX / OHW : 1;
    static constexpr int TH = PIX >= OHW ? OH : PIX / OW;
    static constexpr int ROWS = (TH - 1) * S + 5;
    static constexpr int WIN = OW * S;
    static constexpr int WP0 = (OW - 1) * S + 9;
    static constexpr int WP1 = WIN + 4;
    static constexpr int WP = WP0 > WP1 ? WP0 : WP1;           // units per patch row
    static constexpr int CH = ROWS * WP;                       // units per 8-channel block per image
    static constexpr int XS = NIMG * 2 * CH;                   // patch units of one plane (16 channels)
    static constexpr int WGS = SH ? 0                          // the 16x16x32 form stages no weights (fragments come from global memory)
                                  : 3 * 5 * 2 * 32;            // weight units of one kernel row (3 planes x 5 taps x 2 halves)
    static constexpr int GPK = SH ? 7 : 5;                     // groups per K step: 6 x 2 tap pairs + 1 | kernel rows (staged weight groups)
    static constexpr int NPT = SH ? PIX / 64 : MT;             // pixel tiles per wave (16 pixels each in the SH form, else 32)
    static constexpr int LDS_BYTES = (3 * XS + 2 * WGS) * 16;
};

template <bool SH, int NPT> struct X3Acc { f32x16 t[NPT]; };
template <int NPT> struct X3Acc<true, NPT> { f32x4 t[NPT][2]; };        // [16-pixel tile][16-channel tile]

template <int S, int OW, int MT, int AFF, bool SH = false>      // AFF: 0 plain input, 1 deferred BatchNorm (+ReLU by flag), 2 ... + leaky ReLU
__global__ __launch_bounds__(256, 2) void conv5_x3_kernel(X3P p) {
    using G = X3Geom<S, OW, MT, SH>;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    u32x4* Xs = reinterpret_cast<u32x4*>(lds_raw);            // [3 planes][XS]
    u32x4* Ws = Xs + 3 * G::XS;                                // [2 buffers][WGS] (32x32x16 form only)
    __shared__ float bias_s[32];                              // this workgroup's 32 bias values: fetched while the first patch
                                                              // loads are in flight (a global load in the epilogue is an exposed
                                                              // round trip per workgroup: 36 us of the 32-wide layer)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    X3_STAMP(0);
    X3_STAMP_RT(64);
    constexpr int TILES_PER_IMG = G::OHW >= G::PIX ? G::OHW / G::PIX : 1;
    // XCD-aware tile order: consecutive workgroup ids go round-robin to the 8 XCDs (each with its own L2), so the row tiles
    // of ONE image - which share their halo rows - used to sit on different XCDs and every halo row came from HBM again
    // (profiles/r02_x3_fwd_pmc.json: 188 MB read for 134 MB of input).  Workgroup w = (xcd, k) takes tile xcd * (tiles / 8) + k:
    // neighbouring tiles run on the same XCD at about the same time, the halo is an L2 hit.
    // Two tiles per workgroup (16x16x32 form, p.tpw = 2; round 4), so that the second tile's first patch is loaded
    // under the last tap pair of the first one and its prologue (entry, address set-up, zero
    // fill, the round trip of the first loads: 3 500 of a tile's 63 000 cycles) is paid once.
    // Its tiles are w and w + gridDim.x, NOT 2w and 2w + 1: the workgroups that run side by side then hold neighbouring tiles in both
    // passes and share their halo rows in L2 (with consecutive tiles per workgroup the PMC passes read 172 MB instead of 136).
    const int TPW = SH ? p.tpw : 1;
    int bx = xcd_tile(blockIdx.x, gridDim.x);
    const int ntiles = gridDim.x * TPW;
    int img0 = (G::OHW >= G::PIX) ? bx / TILES_PER_IMG : bx * G::NIMG;
    int row0 = (G::OHW >= G::PIX) ? (bx % TILES_PER_IMG) * G::TH : 0;
    const int o0 = blockIdx.y * 32;
    const int KB = (p.Cin + 15) / 16;
    const int NG = KB * G::GPK;                                // groups: (K step, kernel row | group of 2 tap pairs)

    if (tid < 32) bias_s[tid] = (p.bias && o0 + tid < p.CoutReal) ? p.bias[o0 + tid] : 0.f;
    // pixel tiles of this wave: MT groups of 32 pixels (32x32x16: the pixel on lane & 31, channel block `half`), or 2*MT tiles of 16
    // (16x16x32: the pixel on lane & 15, lane group kq = lane >> 4 = (tap of the pair, channel block))
    constexpr int NPT = G::NPT, TPX = SH ? 16 : 32;
    const int l15 = lane & 15, kq = lane >> 4;
    int pixoff[NPT];
#pragma unroll
    for (int mt = 0; mt < NPT; ++mt) {
        const int pix = (wave * NPT + mt) * TPX + (SH ? l15 : l31);
        const int im = pix / (G::TH * OW), rem = pix % (G::TH * OW);
        const int r = rem / OW, c = rem % OW;
        pixoff[mt] = im * (2 * G::CH) + (SH ? (kq & 1) : half) * G::CH + (r * S) * G::WP + c * S + 4 - p.P;
    }

    // two accumulator sets: the three small partial products are summed apart from the three large ones (added in
    // the epilogue), which also doubles the distance between dependent MFMAs
    X3Acc<SH, NPT> accA, accS;
    auto& acc = accA.t;
    auto& acs = accS.t;
    if constexpr (SH) {
#pragma unroll
        for (int b = 0; b < NPT; ++b)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) { acc[b][ct][r] = 0.f; acs[b][ct][r] = 0.f; }
    } else {
#pragma unroll
        for (int b = 0; b < MT; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[b][r] = 0.f; acs[b][r] = 0.f; }
    }

    int in_row0 = row0 * S - p.P;
    constexpr int W2 = G::WIN / 2;
    // Staging items = (2 pixels x 8 channels).  The 8-channel block `hq` of an item is WAVE-UNIFORM (round 4): waves 0, 1 stage
    // block 0, waves 2, 3 block 1, each pair walking the PERH (image, row, pixel pair) items of its block in XU passes of 128 - so
    // the channel of rx[k][ci] is the same for every lane of a wave and the deferred BatchNorm's coefficients are SCALAR operands
    // (s_load from the coefficient vectors, no LDS table).  The first mapping (block = a per-lane function of the item index) read
    // them from LDS inside the per-lane `live` branch: 16 dependent ds_read_b32 per item, 3 600 + 2 400 of a workgroup's 74 000
    // cycles (tools/x3_stamps.py with AFF=0 / 1).
    constexpr int PERH = G::NIMG * G::ROWS * W2;               // items per 8-channel block and K step
    constexpr int XU = (PERH + 127) / 128, WU = (G::WGS + 255) / 256, WUA = WU ? WU : 1;      // (WU = 0 in the 16x16x32 form)
    const int hq = __builtin_amdgcn_readfirstlane(tid >> 7);   // this wave's channel block (scalar)
    f32x2 rx[XU][8];
    u32x4 rw[WUA];

    // Loads are unconditional (out-of-range items read a valid stand-in address and are zeroed when they are stored to
    // LDS): with branches around them the compiler cannot count outstanding loads and falls back to vmcnt(0).  Their
    // addresses are computed once: per K step / weight group only a uniform stride is added.
    const float* xsrc[XU];
    const float* xsrcN[XU];                                    // ... of the workgroup's next tile
    const u32x4* wsrc[WUA];
    const long cstride = (long)p.H * p.W;
    auto tile_src = [&](int timg0, int tin_row0, const float* (&dst)[XU]) {
#pragma unroll
        for (int k = 0; k < XU; ++k) {
            const int u = (tid & 127) + k * 128;
            const int xp = u % W2;
            const int t = u / W2;
            const int lr = t % G::ROWS, im = t / G::ROWS;
            const int ir = tin_row0 + lr, n = timg0 + im;
            const bool ok = u < PERH && ir >= 0 && ir < p.H && n < p.N;
            dst[k] = p.in + (((long)(ok ? n : 0) * p.Cin + hq * 8) * p.H + (ok ? ir : 0)) * p.W + 2 * xp;
        }
    };
    tile_src(img0, in_row0, xsrc);
#pragma unroll
    for (int k = 0; k < XU; ++k) xsrcN[k] = xsrc[k];
#pragma unroll
    for (int k = 0; k < WU; ++k) {
        const int u = min(tid + k * 256, G::WGS - 1);          // the tail threads re-read the last unit (not stored)
        wsrc[k] = p.wp + (long)(u / 32) * p.OP + o0 + u % 32;
    }
    auto gloadX = [&](int kb, bool next_tile = false) {
        // channels beyond Cin: a clamped (valid) channel is loaded instead and zeroed in lstoreX - pure address arithmetic on
        // wave-uniform values, so that the loads stay unconditional (a per-lane select between two ADDRESSES was compiled into
        // branches around the loads with a vmcnt(0) behind each: 16 serialised round trips in the prologue)
        const int cmax = p.Cin - 1 - (kb * 16 + hq * 8);       // last valid ci of this block (< 0: the whole block is beyond Cin)
        const int cm = cmax < 0 ? 0 : (cmax > 7 ? 7 : cmax);
#pragma unroll
        for (int k = 0; k < XU; ++k) {
            const float* base = next_tile ? xsrcN[k] : xsrc[k];       // (uniform select)
            const float* src = cmax < 0 ? base : base + (long)kb * 16 * cstride;
#pragma unroll
            for (int ci = 0; ci < 8; ++ci)
                rx[k][ci] = *reinterpret_cast<const f32x2*>(src + (long)(ci < cm ? ci : cm) * cstride);
        }
    };
    auto gloadW = [&](int g) {
#pragma unroll
        for (int k = 0; k < WU; ++k) rw[k] = wsrc[k][(long)g * (G::WGS / 32) * p.OP];
    };
    auto lstoreX = [&](int kb) {                    // kb: the K step whose data sits in rx
        // deferred BatchNorm: (scale, shift) of this wave's 8 channels as scalars (uniform addresses in the constant address space)
        typedef const __attribute__((address_space(4))) float* const_f32_p;
        float csc[8], csh[8];
        const float relu_lo = p.aff.relu ? 0.f : -__builtin_inff();
        if constexpr (AFF != 0) {
            const const_f32_p gsc = (const_f32_p)(unsigned long long)p.aff.sc, gsh = (const_f32_p)(unsigned long long)p.aff.sh;
#pragma unroll
            for (int ci = 0; ci < 8; ++ci) {
                const int ch = kb * 16 + hq * 8 + ci;
                const int cc = ch < p.Cin ? ch : p.Cin - 1;                // (clamped: the value is zeroed below)
                csc[ci] = gsc[cc]; csh[ci] = gsh[cc];
            }
        }
#pragma unroll
        for (int k = 0; k < XU; ++k) {
            const int u = (tid & 127) + k * 128;
            if (u < PERH) {
                const int xp = u % W2;
                const int t = u / W2;
                const int lr = t % G::ROWS, im = t / G::ROWS;
                const int h = hq;
                // out-of-image rows / missing images / channels were loaded from a stand-in address: exact zeros
                const int ir = in_row0 + lr, n = img0 + im;
                const bool live = ir >= 0 && ir < p.H && n < p.N;
                f32x2 vv[8];                                               // [channel](pixel 0, pixel 1)
#pragma unroll
                for (int ci = 0; ci < 8; ++ci) {
                    const bool keep = live && kb * 16 + h * 8 + ci < p.Cin;
                    f32x2 v = rx[k][ci];                                   // (a stand-in value where !keep: replaced below)
                    if constexpr (AFF == 1) {                              // ReLU as max(., lo) with lo = 0 or -inf: no select
                        v = f32x2{fmaxf(fmaf(v[0], csc[ci], csh[ci]), relu_lo), fmaxf(fmaf(v[1], csc[ci], csh[ci]), relu_lo)};
                    } else if constexpr (AFF == 2) {                       // leaky ReLU: max(a, 0.01 a)
                        const float a0 = fmaf(v[0], csc[ci], csh[ci]), a1 = fmaf(v[1], csc[ci], csh[ci]);
                        v = f32x2{fmaxf(a0, JVAE_LEAKY_SLOPE * a0), fmaxf(a1, JVAE_LEAKY_SLOPE * a1)};
                    }
                    vv[ci] = keep ? v : f32x2{0.f, 0.f};                   // padding rows / missing channels stay exact zeros
                }
                u32x4 s[2][3];                                             // [pixel][plane]: 8 channels = 4 packed pairs
#pragma unroll
                for (int cp = 0; cp < 4; ++cp)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                    {
                        unsigned hh, mm, ll;
                        x3_split2(f32x2{vv[2 * cp][j], vv[2 * cp + 1][j]}, hh, mm, ll);
                        s[j][0][cp] = hh; s[j][1][cp] = mm; s[j][2][cp] = ll;
                    }
                const int base = (im * 2 + h) * G::CH + lr * G::WP + 4 + 2 * xp;
#pragma unroll
                for (int pl = 0; pl < 3; ++pl)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        Xs[pl * G::XS + base + j] = s[j][pl];
            }
        }
    };
    auto lstoreW = [&](int buf) {
#pragma unroll
        for (int k = 0; k < WU; ++k) {
            const int u = tid + k * 256;
            if (u < G::WGS) Ws[buf * G::WGS + u] = rw[k];
        }
    };

    // one kernel row (5 taps) of one K step: 6 MFMAs per tap and pixel group, fragments of tap kw+1 read ahead
    auto compute = [&](int buf, int rowoff) {
      if constexpr (!SH) {
        const u32x4* Wb = Ws + buf * G::WGS + half * 32 + l31;
        u32x4 fa[2][3], fb[2][3][MT];
        auto frag = [&](int kw, u32x4 (&a)[3], u32x4 (&b)[3][MT]) {
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                a[pl] = Wb[(pl * 5 + kw) * 64];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) b[pl][mt] = Xs[pl * G::XS + pixoff[mt] + rowoff + kw];
            }
        };
        frag(0, fa[0], fb[0]);
#pragma unroll
        for (int kw = 0; kw < 5; ++kw) {
            if (kw + 1 < 5) frag(kw + 1, fa[(kw + 1) & 1], fb[(kw + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
            // (weight plane, input plane): small terms (even t) -> acs, large terms (odd t) -> acc
            constexpr int WPL[6] = {0, 0, 2, 1, 1, 0}, XPL[6] = {2, 1, 0, 0, 1, 0};
#pragma unroll
            for (int t = 0; t < 6; ++t)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    f32x16& d = (t & 1) ? acc[mt] : acs[mt];
                    d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[kw & 1][WPL[t]]),
                                                                __builtin_bit_cast(bf16x8, fb[kw & 1][XPL[t]][mt]), d, 0, 0, 0);
                }
            __builtin_amdgcn_sched_barrier(0);
        }
      }
    };

    // 16x16x32 form.  The 13 tap pairs of a K step (12 pairs + tap 24 with an all-zero partner) run as ONE free sequence (round 6):
    // the patch image is read-only during a K step and the weight fragments do not pass through LDS, so nothing inside a K step
    // needs a barrier - the one barrier pair left sits around lstoreX at the K-step change.  Per pair the wave issues 6 products x
    // NPT pixel tiles x 2 channel tiles; the pair is worked through in halves of 2 pixel tiles (24 MFMAs), the patch fragments of
    // the next half are read ahead.  Lane group kq reads tap 2*pair + (kq >> 1): the second tap of a pair lies one unit to the
    // right, or - when the pair crosses a kernel row (taps 4|5, 14|15) - one row down and four units to the left; tap 25 does not
    // exist (its weights are zero): those lanes re-read tap 24 so that no value from outside the receptive field enters a 0 * x.
    // Weight fragments: the packed buffer is in fragment order ([K step][pair][plane][kq][o] 16-byte units, pack_elems.h
    // JVAE_PACK_X3S), so the lane's operand of (pair, plane, channel tile) is ONE unit at
    //     uniform base (a buffer descriptor + a scalar offset: K step, pair, plane, channel tile) + a 32-bit lane offset (kq, o:
    //     the same register for every load)
    // and is loaded from global memory (L1 / L2: the 8 waves of a CU walk the same 77 KB per K step in loose lock step) straight
    // into fa, one pair ahead as the LDS reads were, into the buffer the pair before has left.  The loads are
    // unconditional and every pair is straight-line code, so the compiler's s_waitcnt vmcnt(N) is counted: a pair waits for its
    // own six loads (issued in front of the previous pair's last 24 MFMAs; nothing else is in flight behind them).  The pair
    // count of a step and the buffer a pair reads are COMPILE-TIME constants (round 4: as run-time values they put the read-ahead
    // behind a branch, and at the join the s_waitcnt had to assume the path without the new reads).
    constexpr int TPH = NPT >= 2 ? 2 : 1;                        // pixel tiles per half
    constexpr int NH = SH ? NPT / TPH : 1;                       // halves per pair
    [[maybe_unused]] u32x4 fa[2][3][2], fb[2][3][TPH];
    const unsigned wlane = (unsigned)(kq * p.OP + l15) * 16u;    // byte offset of the lane's unit inside a (pair, plane, channel tile)
    const int wplane = 4 * p.OP * 16;                            // bytes of one plane of a pair (4 lane groups x OP channels)
    // buffer descriptor of this workgroup's 32-channel column of the packed weights: base and the per-load stream offset are scalar
    // operands, the lane offset is one 32-bit register, reads beyond the packed form would return zeros instead of faulting
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<u32x4*>(p.wp + o0), 0, KB * JVAE_X3S_PAIRS * 3 * wplane - o0 * 16, 0x00020000);
    [[maybe_unused]] auto fragA = [&](int pi, u32x4 (&a)[3][2]) {     // pi = K step * JVAE_X3S_PAIRS + pair (uniform)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
                a[pl][ct] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wlane, (pi * 3 + pl) * wplane + ct * 256, 0));
    };
    [[maybe_unused]] auto fragB = [&](int off, int hp, u32x4 (&b)[3][TPH]) {
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
#pragma unroll
            for (int j = 0; j < TPH; ++j) b[pl][j] = Xs[pl * G::XS + pixoff[(hp * TPH + j) % NPT] + off];
    };
    [[maybe_unused]] auto offs = [&](int pair) {                 // LDS unit offset of THIS lane's tap of a pair (tap 25: tap 24 again)
        auto tapoff = [&](int t) {                               // ... of tap t relative to the lane's pixel
            const int kh = t / 5, kw = t - 5 * kh;
            return kh * G::WP + kw;
        };
        const int ta = 2 * pair;
        const int oa = tapoff(ta), ob = ta == 24 ? oa : tapoff(ta + 1);
        return (kq >> 1) ? ob : oa;
    };
    // One tap pair with its weight fragments in fa[slot] and its first half's patch fragments in fb[...] (both issued earlier).
    // ahead: issue the NEXT pair's weight fragments (stream index pin) in front of this pair's MFMAs and its first patch fragments
    // (offset offn) in front of the last half's; false for the last pair of a K step (the patch changes behind it).
    // hook(): issued behind the read-ahead of the pair's last half and in front of that half's MFMAs (the next patch's global loads).
    [[maybe_unused]] auto pairStep = [&](auto slot_c, auto ahead_c, int off, int offn, int pin, auto&& hook) {
        constexpr int slot = decltype(slot_c)::value;
        constexpr bool ahead = decltype(ahead_c)::value;
#pragma unroll
        for (int hp = 0; hp < NH; ++hp) {
            const int cur = (slot * NH + hp) & 1;
            if (ahead && hp + 1 == NH) fragA(pin, fa[slot ^ 1]);
            if (hp + 1 < NH) fragB(off, hp + 1, fb[cur ^ 1]);
            else if (ahead) fragB(offn, 0, fb[cur ^ 1]);
            if (hp + 1 == NH) { __builtin_amdgcn_sched_barrier(0); hook(); }
            __builtin_amdgcn_sched_barrier(0);
            constexpr int WPL[6] = {0, 0, 2, 1, 1, 0}, XPL[6] = {2, 1, 0, 0, 1, 0};
#pragma unroll
            for (int t = 0; t < 6; ++t)
#pragma unroll
                for (int j = 0; j < TPH; ++j)
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) {
                        if constexpr (SH) {
                            f32x4& d = (t & 1) ? acc[hp * TPH + j][ct] : acs[hp * TPH + j][ct];
                            d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fa[slot][WPL[t]][ct]),
                                                                        __builtin_bit_cast(bf16x8, fb[cur][XPL[t]][j]), d, 0, 0, 0);
                        }
                    }
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    // LDS-only barrier: __syncthreads() also waits for vmcnt(0), i.e. for the global prefetches in flight
    auto lds_barrier = [] { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };

    // ---- epilogue of one tile, 16x16x32 form (called per tile; resets the accumulators)
    __shared__ float red_s[SH ? 4 * 32 * 2 : 1];
    auto epilogueSH = [&] {
      if constexpr (SH) {
        // ---- epilogue, 16x16x32: lane holds pixel l15 of each 16-pixel tile, channels ct*16 + kq*4 + r
#pragma unroll
        for (int b = 0; b < NPT; ++b)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) acc[b][ct] += acs[b][ct];
        float bv[2][4];                            // (bias_s holds zeros without a bias)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) bv[ct][r] = bias_s[ct * 16 + kq * 4 + r];
        const bool fullc = o0 + 32 <= p.CoutReal;
#pragma unroll
        for (int pt = 0; pt < NPT; ++pt) {
            const int pix = (wave * NPT + pt) * 16 + l15;
            const int im = pix / (G::TH * OW), rem = pix % (G::TH * OW);
            const int n = img0 + im;
            if (n >= p.N) continue;
            const int oy = row0 + rem / OW, ox = rem % OW;
            // one base address per pixel tile, the lane's 8 channels at constant strides from it; a full 32-channel block (the
            // uniform, usual case) needs no per-channel bound check - it was a compare + exec branch + 64-bit address chain in
            // front of each of the 32 stores
            float* const dst = p.out + (((long)n * p.CoutReal + o0 + kq * 4) * G::OH + oy) * OW + ox;
            if (fullc) {
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) dst[(ct * 16 + r) * G::OHW] = acc[pt][ct][r] + bv[ct][r];
            } else {
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (o0 + ct * 16 + kq * 4 + r < p.CoutReal) dst[(ct * 16 + r) * G::OHW] = acc[pt][ct][r] + bv[ct][r];
            }
        }
        X3_STAMP(6);                               // output stores issued
        if (p.stats) {
            float* red = red_s;                                   // [4 waves][32][2] (not the patch area: its halo cells stay zero
                                                                  // for the workgroup's next tile)
            float sv[16];                                         // [sum | sum of squares][channel tile][register]
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float s1 = 0.f, s2 = 0.f;
#pragma unroll
                    for (int pt = 0; pt < NPT; ++pt) { const float v = acc[pt][ct][r]; s1 += v; s2 += v * v; }
                    sv[ct * 4 + r] = s1;
                    sv[8 + ct * 4 + r] = s2;
                }
            stats_stage16(sv, red, wave, l15, kq);
            lds_barrier();                                        // LDS only: the output stores keep draining
            stats_fold<4, 32>(red, p.stats, tid, o0, p.CoutReal, ntiles, bx);
        }
#pragma unroll
        for (int b = 0; b < NPT; ++b)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) { acc[b][ct][r] = 0.f; acs[b][ct][r] = 0.f; }
      }
    };

    X3_STAMP(1);                                   // 0 = kernel entry (below the declarations), 1 = zero fill issued
    gloadX(0);
    if constexpr (!SH) gloadW(0);
    // The halo COLUMNS (4 units left of the image row, WP - 4 - WIN right of it) are zeroed once and never written again;
    // every other cell - out-of-image rows, missing images and channels included - is rewritten by lstoreX at every K step.
    // Issued behind the first global loads (they fly meanwhile).  Round 4: the whole 46 KB image used to be cleared, in front
    // of the loads: 2 200 of a workgroup's 73 500 cycles (tools/x3_stamps.py).
    {
        constexpr int HALO = G::WP - G::WIN, NROW = 3 * G::NIMG * 2 * G::ROWS;
        for (int i = tid; i < NROW * HALO; i += 256) {
            const int r = i / HALO, c = i % HALO;
            const int pl = r / (G::NIMG * 2 * G::ROWS), rr = r % (G::NIMG * 2 * G::ROWS);
            Xs[pl * G::XS + rr * G::WP + (c < 4 ? c : c + G::WIN)] = u32x4{0u, 0u, 0u, 0u};
        }
    }
    __syncthreads();                               // halo zero fill complete (it overlaps nothing lstoreX writes, but orders bias_s)
    X3_STAMP(2);
    lstoreX(0);
    if constexpr (SH) {
        fragA(0, fa[0]);                           // the first pair's weight fragments
    } else {
        lstoreW(0);
        __builtin_amdgcn_sched_barrier(0);
        if (NG > 1) gloadW(1);
    }
    lds_barrier();
    X3_STAMP(3);
    if constexpr (SH) {
        // 16x16x32 form: K steps outside; the six two-pair groups of a K step inside (a loop: the pair -> buffer mapping repeats
        // every two pairs), its 13th pair with the K-step change behind them - so that the registers of the next patch (rx: loaded
        // in front of the 13th pair's last MFMAs, split and stored behind them) are live in that tail only and not across the two-pair
        // code, which needs the room for its read-ahead
        typedef std::integral_constant<int, 0> slot0;
        typedef std::integral_constant<int, 1> slot1;
        int g = 0;                                     // group inside the tile (stamps)
        bool has_next = false;
        for (int ti = 0; ti < TPW; ++ti) {
            has_next = ti + 1 < TPW;
            if (has_next) {                                // the next tile's coordinates and patch addresses
                const int nb = bx + gridDim.x;
                const int nimg0 = (G::OHW >= G::PIX) ? nb / TILES_PER_IMG : nb * G::NIMG;
                const int nrow0 = (G::OHW >= G::PIX) ? (nb % TILES_PER_IMG) * G::TH : 0;
                tile_src(nimg0, nrow0 * S - p.P, xsrcN);
            }
            g = 0;
            for (int kb = 0; kb < KB; ++kb) {
                // invariant: patch of K step kb in Xs, the weight fragments of its pair 0 on their way into fa[0] (issued behind lstoreX)
                const int pi0 = kb * JVAE_X3S_PAIRS;
                int off = offs(0);
                fragB(off, 0, fb[0]);
                for (int gi = 0; gi < G::GPK - 1; ++gi, ++g) {
                    if (g < 14) X3_STAMP(8 + 4 * g);           // group start
                    const int off1 = offs(2 * gi + 1);
                    pairStep(slot0{}, std::true_type{}, off, off1, pi0 + 2 * gi + 1, [&] {
                        if (g < 14) X3_STAMP(9 + 4 * g);       // read-ahead issued
                    });
                    off = offs(2 * gi + 2);
                    pairStep(slot1{}, std::true_type{}, off1, off, pi0 + 2 * gi + 2, [] {});
                    if (g < 14) X3_STAMP(10 + 4 * g);          // MFMAs issued
                    if (g < 14) X3_STAMP(11 + 4 * g);          // (no barrier)
                }
                const bool nextk = kb + 1 < KB;
                if (g < 14) X3_STAMP(8 + 4 * g);
                // The next patch's loads (the next tile's first patch behind the last K step) go out in front of this pair's LAST half:
                // by then its weight fragments have all been waited for, so nothing in front of lstoreX waits on the vector-memory
                // counter again.  In front of the first half, the branch around them would join ahead of MFMAs that still wait
                // for fa[0], and that wait has to assume the path without the loads behind it: vmcnt(0), the patch's round trip.
                // (Hoisting the condition around the whole pair - two copies of it - cost 180 bytes of scratch.)
                pairStep(slot0{}, std::false_type{}, off, off, 0, [&] {
                    if (nextk || has_next) gloadX(nextk ? kb + 1 : 0, !nextk);
                    if (g < 14) X3_STAMP(9 + 4 * g);
                });
                if (g < 14) X3_STAMP(10 + 4 * g);
                lds_barrier();                                 // every wave is past the patch
                if (g < 14) X3_STAMP(11 + 4 * g);
                if (nextk) {                                   // K step change: the patch is fully consumed
                    lstoreX(kb + 1);
                    fragA(pi0 + JVAE_X3S_PAIRS, fa[0]);        // behind the split (its registers are the kernel's peak), under the barrier
                    lds_barrier();
                    X3_STAMP(4);                               // (first) K step change done
                }
                ++g;
            }
            epilogueSH();                                      // (its LDS use is red_s; the stores drain under what follows)
            if (has_next) {                                    // enter the next tile: its first patch sits in rx
                bx += gridDim.x;
                img0 = (G::OHW >= G::PIX) ? bx / TILES_PER_IMG : bx * G::NIMG;
                row0 = (G::OHW >= G::PIX) ? (bx % TILES_PER_IMG) * G::TH : 0;
                in_row0 = row0 * S - p.P;
#pragma unroll
                for (int k = 0; k < XU; ++k) xsrc[k] = xsrcN[k];
                lstoreX(0);
                fragA(0, fa[0]);                               // the weight stream starts again
                lds_barrier();
            }
        }
    } else {
        int kb = 0, kh = 0;
        for (int g = 0; g < NG; ++g) {
            // invariant: patch of K step kb in Xs, weight group g in buffer g&1, rw = weight group g+1 (in flight)
            const bool more = g + 1 < NG, last_row = kh == G::GPK - 1;
            if (more) lstoreW((g + 1) & 1);                // (the store, which waits for rw, ahead of the next loads: the scheduler
                                                           // would otherwise issue them first and wait for all)
            __builtin_amdgcn_sched_barrier(0);
            if (g + 2 < NG) gloadW(g + 2);
            if (kh == G::GPK - 2 && kb + 1 < KB) gloadX(kb + 1);
            __builtin_amdgcn_sched_barrier(0);
            compute(g & 1, kh * G::WP);
            lds_barrier();
            if (more && last_row) {                        // K step change: the patch is fully consumed
                lstoreX(kb + 1);
                lds_barrier();
            }
            if (++kh == G::GPK) { kh = 0; ++kb; }
        }
    }

    X3_STAMP(5);                                   // main loop done
    if constexpr (SH) {
        X3_STAMP(7);                               // end of the workgroup's program
        X3_STAMP_RT(65);
    } else {
#pragma unroll
    for (int b = 0; b < MT; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] += acs[b][r];

    // ---- epilogue: lane holds pixel l31 of each 32-pixel group, rows (channels) (r&3) + 8*(r>>2) + 4*half
    auto store_tile = [&](const float (&bv)[16], bool biased) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int pix = (wave * MT + mt) * 32 + l31;
            const int im = pix / (G::TH * OW), rem = pix % (G::TH * OW);
            const int n = img0 + im;
            if (n >= p.N) continue;
            const int oy = row0 + rem / OW, ox = rem % OW;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = o0 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (o >= p.CoutReal) continue;
                p.out[(((long)n * p.CoutReal + o) * G::OH + oy) * OW + ox] = biased ? acc[mt][r] + bv[r] : acc[mt][r];
            }
        }
    };
    float bv[16];
    if (p.bias) {
        // the lane's 16 bias values from LDS; the bias-free directions keep the plain stores
#pragma unroll
        for (int r = 0; r < 16; ++r) bv[r] = bias_s[(r & 3) + 8 * (r >> 2) + 4 * half];
        store_tile(bv, true);
    } else {
        store_tile(bv, false);
    }

    // ---- optional BatchNorm statistics of this workgroup's tile (the loop ended with a barrier: LDS is free).  AFTER the
    // output stores: they drain while the sums are reduced, and no wave waits at the reduction's barrier with its tile unsent
    if (p.stats) {
        float* red = reinterpret_cast<float*>(lds_raw);       // [4 waves][32][2]
        float sv[32];                                         // [sum | sum of squares][register row]
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) { const float v = acc[mt][r]; s1 += v; s2 += v * v; }
            sv[r] = s1;
            sv[16 + r] = s2;
        }
        stats_stage32<32>(sv, red, wave, 0, l31, half);
        lds_barrier();                                        // LDS only: the output stores keep draining
        stats_fold<4, 32>(red, p.stats, tid, o0, p.CoutReal, gridDim.x, bx);
    }
    }
}

template <int S, int OW, int MT, bool SH = false>
int launch_x3(const X3P& p, hipStream_t st, int* nsplit) {
    using G = X3Geom<S, OW, MT, SH>;
    static_assert(S == 1 && G::LDS_BYTES + 2048 <= 80 * 1024, "two workgroups per CU");
    static bool attr_set = false;
    auto kernel = [](auto A) { return &conv5_x3_kernel<S, OW, MT, decltype(A)::value, SH>; };
    if (const int rc = jvae_aff_lds_attr(attr_set, G::LDS_BYTES, kernel)) return rc;
    const long pixels = (long)p.N * G::OHW;
    dim3 grid((unsigned)((pixels + G::PIX - 1) / G::PIX), (unsigned)(p.OP / 32));
    if (G::OHW < G::PIX) grid.x = (unsigned)((p.N + G::NIMG - 1) / G::NIMG);
    const int tiles = (int)grid.x;                             // BatchNorm partial sums: one per TILE
    // Two tiles per workgroup (16x16x32 form, stride 1) when that still leaves two residency rounds of 512 workgroups:
    // the second tile's prologue hides under the first one's last tap pairs.
    X3P q = p;
    q.tpw = 1;
    if (SH && grid.x % 2 == 0 && (long)grid.x * grid.y >= 2048) { q.tpw = 2; grid.x /= 2; }
    jvae_with_aff(jvae_aff_inst(q.aff), [&](auto A) { hipLaunchKernelGGL(kernel(A), grid, dim3(256), G::LDS_BYTES, st, q); });
    JVAE_LAUNCH_CHECK();
    if (nsplit) *nsplit = tiles;
    return 0;
}

}  // namespace

#ifdef JVAE_X3_STAMPS
static unsigned long long* g_x3_dbg = nullptr;
extern "C" void jvae_x3_set_stamp_buffer(void* buf) { g_x3_dbg = (unsigned long long*)buf; }     // diagnostic build only
#endif
// JVAE_X3=0 (read once, when the library is loaded) or jvae_conv2d_set_split(0): every layer, dense product and weight gradient
// stays on the fp32 matrix-core kernels - the one selector left, exercised by the parity tests through the setter
static int g_x3 = [] { const char* e = getenv("JVAE_X3"); return (e && e[0] == '0') ? 0 : 1; }();
static int g_x3_sh16 = 1;    // jvae_conv2d_set_split_shape16(0): the 32x32x16 MFMA shape also for maps up to 32 wide (tests run both)

// Layers the split kernel takes over from conv_mfma.hip: stride 1, at least one full K step of input channels.
int jvae_conv5_x3_set(int mode) {
    const int old = g_x3;
    g_x3 = mode ? 1 : 0;
    return old;
}

bool jvae_conv5_x3_enabled() {
    return g_x3 != 0;
}

static bool x3_sh16() { return g_x3_sh16 != 0; }

// MFMA shape of the stride-1 forward-type kernel: 1 = v_mfma_f32_16x16x32_bf16 (K = 2 taps x 16 channels), 0 = 32x32x16.
// Returns the previous setting.
int jvae_conv5_x3_set_shape16(int on) {
    const int old = x3_sh16() ? 1 : 0;
    g_x3_sh16 = on ? 1 : 0;
    return old;
}

// split weights for conv5_x3_kernel / convt2_x3_kernel: ws must hold jvae_conv5_x3_pack_bytes(C, O)
int jvae_conv5_x3_wpack(const float* w, float* ws, int C, int O, int swap, int flip, hipStream_t st) {
    const int KB = (C + 15) / 16, OP = (O + 31) / 32 * 32;
    const long total = (long)KB * 25 * 2 * OP * 8;
    const int blocks = (int)((total + 255) / 256 > 1024 ? 1024 : (total + 255) / 256);
    hipLaunchKernelGGL(x3_wpack_kernel, dim3(blocks), dim3(256), 0, st, w, (__bf16*)ws, C, O, KB, OP, swap, flip);
    JVAE_LAUNCH_CHECK();
    return 0;
}

bool jvae_conv5_x3_ok(int Cin, int H, int W, int Cout, int OH, int OW, int S, int P) {
    if (!g_x3) return false;
    if (Cin < 16 || Cin > 256) return false;
    // Stride-2 forward-type layers (E1 / E3 forward, D2 / D4 dgrad of conv32 / deconv32) stay on the fp32 matrix-core kernel: their
    // patch is 4x the output pixels, and both split-bf16 forms built for them (round 3: 128-pixel tile, one workgroup per CU; round 4:
    // 16x16x32 on a de-interleaved 64-pixel patch, two per CU) measured at best at parity with it (profiles/NOTES.md).
    if (S != 1) return false;
    if (OW != 8 && OW != 16 && OW != 32 && OW != 64) return false;
    return jvae_conv5_fwd_ok(Cin, H, W, Cout, OH, OW, S, P);
}

// bytes of the largest of the packed forms (kernel-row groups / tap-pair groups / position-sorted taps of the 4-phase kernel)
size_t jvae_conv5_x3_pack_bytes(int Cin, int Cout) {
    const size_t a = jvae_pack_bytes(JVAE_PACK_X3, Cin, Cout), b = jvae_pack_bytes(JVAE_PACK_X3S, Cin, Cout);
    const size_t c = jvae_pack_bytes(JVAE_PACK_T2S, Cin, Cout);      // (conv_t2_x3.hip's 32-channel K step)
    return a > b ? (a > c ? a : c) : (b > c ? b : c);
}

static int x3s_wpack(const float* w, float* ws, int C, int O, int swap, int flip, hipStream_t st) {
    const long total = jvae_pack_elems(JVAE_PACK_X3S, C, O);
    const int blocks = (int)((total + 255) / 256 > 1024 ? 1024 : (total + 255) / 256);
    hipLaunchKernelGGL(x3s_wpack_kernel, dim3(blocks), dim3(256), 0, st, w, (__bf16*)ws, C, O, total, swap, flip);
    JVAE_LAUNCH_CHECK();
    return 0;
}

int jvae_conv5_x3_fwd(const float* in, const float* w, int swap, int flip, const float* bias, float* out,
                      int N, int Cin, int H, int W, int Cout, int OW, int S, int P, float* ws, hipStream_t st,
                      float* stats, int* nsplit, const InAff* aff) {
    const int OP = (Cout + 31) / 32 * 32;
    const bool sh = OW <= 32 && x3_sh16();                  // 64-wide maps (config 5 in fp32) keep the 32x32x16 form
    // split weights: the step's cache slot (refreshed once per step, pack_cache.hip) or this call's workspace
    int rc = 0;
    ws = (float*)jvae_packed(sh ? JVAE_PACK_X3S : JVAE_PACK_X3, w, Cin, Cout, swap, flip, ws, [&](void* dst) {
        return (sh ? x3s_wpack : jvae_conv5_x3_wpack)(w, (float*)dst, Cin, Cout, swap, flip, st);
    }, &rc);
    if (!ws) return rc ? rc : JVAE_EINVAL;
    X3P p{in, (const u32x4*)ws, bias, out, N, Cin, H, W, OP, P, Cout, stats, aff ? *aff : InAff{nullptr, nullptr, 0}, 1};
#ifdef JVAE_X3_STAMPS
    p.dbg = g_x3_dbg;
#endif
    if (S != 1) return JVAE_ENOTSUP;
    if (sh) {
        switch (OW) {
            case 8: return launch_x3<1, 8, 1, true>(p, st, nsplit);
            case 16: return launch_x3<1, 16, 2, true>(p, st, nsplit);
            case 32: return launch_x3<1, 32, 2, true>(p, st, nsplit);
        }
    }
    switch (OW) {
        case 8: return launch_x3<1, 8, 1>(p, st, nsplit);
        case 16: return launch_x3<1, 16, 2>(p, st, nsplit);
        case 32: return launch_x3<1, 32, 2>(p, st, nsplit);
        case 64: return launch_x3<1, 64, 1>(p, st, nsplit);
    }
    return JVAE_ENOTSUP;
}
