// Device-resident image sets (jvae_compat/torch_load.py): a list of sample indices -> a ready float32 NCHW batch and its
// int64 labels in ONE launch, with the static transform chain of the set (utils/torch_load.py:347-426) and, when asked, the
// random flip / edge-padded crop of augment.hip.  The set's raw uint8 images stay on the device; nothing but the index list
// comes from the host per batch.
//
// The chain is walked BACKWARDS from the output coordinate, stage by stage, in integer arithmetic:
//   output <- post transform (zero pad 2 | centre crop | none) <- random part (crop at (dy, dx) of the edge-padded image, flip)
//          <- g2c <- quarter-turn/flip element B <- zero padding p0 <- resize (PIL 8-bit bilinear, two passes) <- element A
//          <- data[idx[i]]
// A coordinate that lands in zero padding is 0.0f; everything else is (float)v / 255.0f of one source byte, or of the resized
// byte.  The result is a pure function of its inputs: bit-exact against the torchvision chain.
//
// A MIXED batch (the moving sets of jvae_compat/ft_datasets.py) takes its images from several resident sets with different
// layouts and chains, and from the synthetic const / uniform sets: imageset_mixed_kernel reads, per image, the record of its
// leaf (pointers + the 20 descriptor words) from a table on the device and walks that leaf's chain with the same
// chain_value() as the single-set kernel - the resize is chosen per image there, not per launch.
#include "common.h"
#include "jvae_internal.h"

namespace {

constexpr int IMAGESET_DESC_WORDS = 20;
constexpr int IMAGESET_MAX_TAPS = 8;

// One of the eight compositions of k counter-clockwise quarter turns followed by a horizontal flip, as the map from a
// coordinate of its OUTPUT to the coordinate of its input: ys = ay * y + by * x + cy, xs = ax * y + bx * x + cx.
struct Turn { int ay, by, cy, ax, bx, cx; };

struct Chain {
    int nhwc, Hs, Ws, Cs;      // source layout and extents
    Turn A;                    // first element, input (Hs, Ws)
    int H1, W1;                // extents after A
    int Hr, Wr, kh, kv;        // resize target and taps per axis (RESIZE only)
    int p0;                    // zero padding on all four sides
    int H2, W2;                // extents after resize (or H1, W1) and before p0
    Turn B;                    // second element, input (H2 + 2 p0, W2 + 2 p0)
    int g2c;                   // one source channel repeated
    int H6, W6;                // extents after B = extents of the random part
    int pa;                    // edge padding of the random crop
    int py, px;                // post transform: output (y, x) -> (y + py, x + px) of the (H6, W6) image, outside = zero
    int C, H, W;               // output
};

__host__ __device__ inline Turn make_turn(int e, int Hi, int Wi, int* Ho, int* Wo) {
    const int k = e & 3, f = e >> 2;
    *Ho = (k & 1) ? Wi : Hi;
    *Wo = (k & 1) ? Hi : Wi;
    // rot90^k: out[y][x] = in[ys][xs]
    Turn t;
    switch (k) {
        case 0: t = {1, 0, 0, 0, 1, 0}; break;
        case 1: t = {0, 1, 0, -1, 0, Wi - 1}; break;
        case 2: t = {-1, 0, Hi - 1, 0, -1, Wi - 1}; break;
        default: t = {0, -1, Hi - 1, 1, 0, 0}; break;
    }
    if (f) {                   // the flip acts on the turned image: x -> Wo - 1 - x in front of the turn
        t.cy += t.by * (*Wo - 1); t.by = -t.by;
        t.cx += t.bx * (*Wo - 1); t.bx = -t.bx;
    }
    return t;
}

__device__ inline int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// byte (c, y, x) of image `img` as it is after element A
__device__ inline int fetch_a(const Chain& ch, const unsigned char* __restrict__ img, int c, int y, int x) {
    const int ys = ch.A.ay * y + ch.A.by * x + ch.A.cy;
    const int xs = ch.A.ax * y + ch.A.bx * x + ch.A.cx;
    const long src = ch.nhwc ? ((long)ys * ch.Ws + xs) * ch.Cs + c : ((long)c * ch.Hs + ys) * ch.Ws + xs;
    return img[src];
}

// The backward walk for ONE output element (c, y, x) of one image: shared by the single-set and the mixed kernel.  `oy`, `ox`
// are the crop offsets of the random part (ch.pa = centred), `flipped` its flip.
template <bool RESIZE>
__device__ inline float chain_value(const Chain& ch, const unsigned char* __restrict__ img, const int* __restrict__ coef_h,
                                    const int* __restrict__ bounds_h, const int* __restrict__ coef_v,
                                    const int* __restrict__ bounds_v, int c, int y, int x, int oy, int ox, bool flipped) {
    // post transform
    y += ch.py; x += ch.px;
    if (y < 0 || y >= ch.H6 || x < 0 || x >= ch.W6) return 0.0f;
    // random part: crop of the edge-padded image, then the flip that came before the padding
    y += oy - ch.pa;
    x += ox - ch.pa;
    y = y < 0 ? 0 : (y >= ch.H6 ? ch.H6 - 1 : y);
    x = x < 0 ? 0 : (x >= ch.W6 ? ch.W6 - 1 : x);
    if (flipped) x = ch.W6 - 1 - x;
    if (ch.g2c) c = 0;
    // element B, then the zero padding in front of it
    const int yb = ch.B.ay * y + ch.B.by * x + ch.B.cy - ch.p0;
    const int xb = ch.B.ax * y + ch.B.bx * x + ch.B.cx - ch.p0;
    if (yb < 0 || yb >= ch.H2 || xb < 0 || xb >= ch.W2) return 0.0f;
    int v;
    if constexpr (RESIZE) {
        // PIL's two passes for this one pixel: the horizontal pass of every source row the vertical pass reads, each
        // rounded and clipped to 8 bits, then the vertical pass; 22-bit fixed-point coefficients, sums in int32
        const int y0 = bounds_v[2 * yb], ny = bounds_v[2 * yb + 1];
        const int x0 = bounds_h[2 * xb], nx = bounds_h[2 * xb + 1];
        int acc = 1 << 21;
        for (int a = 0; a < ny; ++a) {
            int row = 1 << 21;
            for (int b = 0; b < nx; ++b) row += coef_h[xb * ch.kh + b] * fetch_a(ch, img, c, y0 + a, x0 + b);
            acc += coef_v[yb * ch.kv + a] * clip8(row >> 22);
        }
        v = clip8(acc >> 22);
    } else {
        v = fetch_a(ch, img, c, yb, xb);
    }
    return (float)v / 255.0f;
}

template <bool RESIZE>
__global__ __launch_bounds__(256) void imageset_kernel(const unsigned char* __restrict__ data, const long long* __restrict__ idx,
                                                       const long long* __restrict__ targets, const long long* __restrict__ lut,
                                                       const int* __restrict__ coef_h, const int* __restrict__ bounds_h,
                                                       const int* __restrict__ coef_v, const int* __restrict__ bounds_v,
                                                       const unsigned char* __restrict__ flip, const int* __restrict__ dy,
                                                       const int* __restrict__ dx, float* __restrict__ out,
                                                       long long* __restrict__ yout, int N, Chain ch) {
    const long per_image = (long)ch.Cs * ch.Hs * ch.Ws;
    const long total = (long)N * ch.C * ch.H * ch.W;
    const long stride = (long)gridDim.x * blockDim.x;
    const long first = (long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long i = first; i < N; i += stride) {
        const long long t = targets[idx[i]];
        yout[i] = lut ? lut[t] : t;
    }
    for (long i = first; i < total; i += stride) {
        const int x = (int)(i % ch.W);
        long r = i / ch.W;
        const int y = (int)(r % ch.H); r /= ch.H;
        const int c = (int)(r % ch.C);
        const int n = (int)(r / ch.C);
        out[i] = chain_value<RESIZE>(ch, data + (long)idx[n] * per_image, coef_h, bounds_h, coef_v, bounds_v, c, y, x,
                                     dy ? dy[n] : ch.pa, dx ? dx[n] : ch.pa, flip && flip[n]);
    }
}

// desc (host): [0] nhwc [1] Hs [2] Ws [3] Cs [4] A [5] resize [6] Hr [7] Wr [8] kh [9] kv [10] p0 [11] B [12] g2c [13] pa
//              [14] post (0 none, 1 zero pad 2, 2 centre crop) [15] oy [16] ox (crop offsets) [17] C [18] H [19] W
__host__ __device__ inline int chain_from_desc(const int* d, Chain* out) {
    Chain ch{};
    ch.nhwc = d[0]; ch.Hs = d[1]; ch.Ws = d[2]; ch.Cs = d[3];
    const int A = d[4], resize = d[5], B = d[11], post = d[14];
    if ((ch.nhwc != 0 && ch.nhwc != 1) || ch.Hs <= 0 || ch.Ws <= 0 || (ch.Cs != 1 && ch.Cs != 3)) return JVAE_EINVAL;
    if (A < 0 || A > 7 || B < 0 || B > 7 || (resize != 0 && resize != 1) || d[10] < 0 || d[13] < 0) return JVAE_EINVAL;
    if (post < 0 || post > 2 || (d[12] != 0 && d[12] != 1) || (d[12] && ch.Cs != 1)) return JVAE_EINVAL;
    ch.A = make_turn(A, ch.Hs, ch.Ws, &ch.H1, &ch.W1);
    ch.H2 = ch.H1; ch.W2 = ch.W1;
    if (resize) {
        ch.Hr = d[6]; ch.Wr = d[7]; ch.kh = d[8]; ch.kv = d[9];
        if (ch.Hr <= 0 || ch.Wr <= 0 || ch.kh <= 0 || ch.kv <= 0) return JVAE_EINVAL;
        if (ch.kh > IMAGESET_MAX_TAPS || ch.kv > IMAGESET_MAX_TAPS) return JVAE_ENOTSUP;
        ch.H2 = ch.Hr; ch.W2 = ch.Wr;
    }
    ch.p0 = d[10];
    ch.B = make_turn(B, ch.H2 + 2 * ch.p0, ch.W2 + 2 * ch.p0, &ch.H6, &ch.W6);
    ch.g2c = d[12];
    ch.pa = d[13];
    ch.C = ch.g2c ? 3 : ch.Cs;
    if (post == 1) {
        ch.py = ch.px = -2;
        ch.H = ch.H6 + 4; ch.W = ch.W6 + 4;
    } else if (post == 2) {                        // offsets as torchvision rounds them, worked out by the caller
        ch.py = d[15]; ch.px = d[16];
        ch.H = d[18]; ch.W = d[19];
        if (ch.H <= 0 || ch.W <= 0 || ch.py < 0 || ch.px < 0 || ch.py + ch.H > ch.H6 || ch.px + ch.W > ch.W6) return JVAE_EINVAL;
    } else {
        ch.H = ch.H6; ch.W = ch.W6;
    }
    if (d[17] != ch.C || d[18] != ch.H || d[19] != ch.W) return JVAE_EINVAL;      // the caller allocated another output
    *out = ch;
    return 0;
}

// ---- mixed batches: one record per leaf, laid out by jvae_hip/ops.py (ImagesetMixTable) exactly like this
struct MixLeaf {
    int kind;                                      // 0 image set, 1 const, 2 uniform
    int border;                                    // synthetic leaves: zero border of 2 (the 'pad' transformer)
    const unsigned char* data;
    const long long* targets;
    const long long* lut;
    const int* coef_h;
    const int* bounds_h;
    const int* coef_v;
    const int* bounds_v;
    int desc[IMAGESET_DESC_WORDS];                 // synthetic leaves: only [17..19], the output extents
};

// VEC consecutive x of one row per thread (W % VEC == 0).  The leaf changes from image to image, and an image boundary falls
// inside a wave whenever C*H*W is no multiple of 64: nothing of a leaf is taken to be uniform over the wave; each thread
// keeps the chain of the leaf it met last and builds another one only when the leaf changes.
template <int VEC>
__global__ __launch_bounds__(256) void imageset_mixed_kernel(const MixLeaf* __restrict__ leaves, const int* __restrict__ leaf,
                                                             const long long* __restrict__ index,
                                                             const long long* __restrict__ tag, const long long* __restrict__ pos,
                                                             const float* __restrict__ u, long u_step, float* __restrict__ out,
                                                             long long* __restrict__ tagout, long long* __restrict__ yout, int N,
                                                             int C, int H, int W) {
    const long total = (long)N * C * H * W / VEC;
    const long stride = (long)gridDim.x * blockDim.x;
    const long first = (long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long i = first; i < N; i += stride) {
        const long long p = pos[i];
        const MixLeaf& L = leaves[leaf[p]];
        long long t = 0;
        if (L.kind == 0) {
            t = L.targets[index[p]];
            if (L.lut) t = L.lut[t];
        }
        yout[i] = t;
        tagout[i] = tag[p];
    }
    int current = -1, kind = 0, resize = 0;
    long per_image = 0;
    Chain ch{};
    for (long i = first; i < total; i += stride) {
        const long e = i * VEC;
        const int x = (int)(e % W);
        long r = e / W;
        const int y = (int)(r % H); r /= H;
        const int c = (int)(r % C);
        const int n = (int)(r / C);
        const long long p = pos[n];
        const int l = leaf[p];
        const MixLeaf& L = leaves[l];
        if (l != current) {
            current = l;
            kind = L.kind;
            if (kind == 0) {
                chain_from_desc(L.desc, &ch);      // checked on the host before the launch
                resize = L.desc[5];
                per_image = (long)ch.Cs * ch.Hs * ch.Ws;
            }
        }
        float v[VEC];
        if (kind == 0) {
            const unsigned char* img = L.data + (long)index[p] * per_image;
#pragma unroll
            for (int k = 0; k < VEC; ++k)
                v[k] = resize ? chain_value<true>(ch, img, L.coef_h, L.bounds_h, L.coef_v, L.bounds_v, c, y, x + k, ch.pa, ch.pa, false)
                              : chain_value<false>(ch, img, nullptr, nullptr, nullptr, nullptr, c, y, x + k, ch.pa, ch.pa, false);
        } else {
            const bool rows_in = !L.border || (y >= 2 && y < H - 2);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const bool in = rows_in && (!L.border || (x + k >= 2 && x + k < W - 2));
                v[k] = !in ? 0.0f : (kind == 1 ? u[((long)n * C + c) * u_step] : u[e + k]);
            }
        }
        if constexpr (VEC == 4) {
            *reinterpret_cast<float4*>(out + e) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int k = 0; k < VEC; ++k) out[e + k] = v[k];
        }
    }
}

}  // namespace

extern "C" int jvae_imageset_desc_words(void) { return IMAGESET_DESC_WORDS; }

extern "C" int jvae_imageset_batch_u8_f32(const unsigned char* data, const long long* idx, const long long* targets,
                                          const long long* lut, const int* desc, const int* coef_h, const int* bounds_h,
                                          const int* coef_v, const int* bounds_v, const unsigned char* flip, const int* dy,
                                          const int* dx, float* x, long long* y, long n, int N, void* stream) {
    if (!data || !idx || !targets || !desc || !x || !y || n <= 0 || N < 0) return JVAE_EINVAL;
    Chain ch;
    const int rc = chain_from_desc(desc, &ch);
    if (rc) return rc;
    if (desc[5] && (!coef_h || !bounds_h || !coef_v || !bounds_v)) return JVAE_EINVAL;
    if ((dy == nullptr) != (dx == nullptr)) return JVAE_EINVAL;
    if (N == 0) return 0;
    const long total = (long)N * ch.C * ch.H * ch.W;
    long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (desc[5])
        hipLaunchKernelGGL(imageset_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, data, idx, targets,
                           lut, coef_h, bounds_h, coef_v, bounds_v, flip, dy, dx, x, y, N, ch);
    else
        hipLaunchKernelGGL(imageset_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, data, idx, targets,
                           lut, coef_h, bounds_h, coef_v, bounds_v, flip, dy, dx, x, y, N, ch);
    JVAE_LAUNCH_CHECK();
    return 0;
}

extern "C" int jvae_imageset_mix_leaf_bytes(void) { return (int)sizeof(MixLeaf); }

extern "C" int jvae_imageset_mixed_u8_f32(const void* leaves_host, const void* leaves_dev, int n_leaves, const int* leaf,
                                          const long long* index, const long long* tag, const long long* pos, const float* u,
                                          int u_dims, float* x, long long* tagout, long long* y, int N, int vec, void* stream) {
    if (!leaves_host || !leaves_dev || n_leaves <= 0 || !leaf || !index || !tag || !pos || !x || !tagout || !y || N < 0)
        return JVAE_EINVAL;
    const MixLeaf* rec = static_cast<const MixLeaf*>(leaves_host);
    const int C = rec[0].desc[17], H = rec[0].desc[18], W = rec[0].desc[19];
    if (C <= 0 || H <= 0 || W <= 0) return JVAE_EINVAL;
    int synthetic = 0;
    for (int l = 0; l < n_leaves; ++l) {
        const MixLeaf& L = rec[l];
        if (L.desc[17] != C || L.desc[18] != H || L.desc[19] != W) return JVAE_EINVAL;
        if (L.kind == 0) {
            Chain ch;
            const int rc = chain_from_desc(L.desc, &ch);
            if (rc) return rc;
            if (!L.data || !L.targets || L.desc[13]) return JVAE_EINVAL;          // no random part in a mixed batch
            if (L.desc[5] && (!L.coef_h || !L.bounds_h || !L.coef_v || !L.bounds_v)) return JVAE_EINVAL;
        } else if (L.kind == 1 || L.kind == 2) {
            if ((L.border != 0 && L.border != 1) || (L.border && (H <= 4 || W <= 4))) return JVAE_EINVAL;
            synthetic |= L.kind;
        } else {
            return JVAE_EINVAL;
        }
    }
    if (synthetic && (!u || (u_dims != 2 && u_dims != 4) || ((synthetic & 2) && u_dims != 4))) return JVAE_EINVAL;
    if (vec == 0) vec = 1;
    if ((vec != 1 && vec != 4) || W % vec) return JVAE_EINVAL;
    if (N == 0) return 0;
    const long total = (long)N * C * H * W / vec;
    long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    const long u_step = u_dims == 4 ? (long)H * W : 1;
    const MixLeaf* dev = static_cast<const MixLeaf*>(leaves_dev);
    if (vec == 4)
        hipLaunchKernelGGL(imageset_mixed_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dev, leaf, index,
                           tag, pos, u, u_step, x, tagout, y, N, C, H, W);
    else
        hipLaunchKernelGGL(imageset_mixed_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dev, leaf, index,
                           tag, pos, u, u_step, x, tagout, y, N, C, H, W);
    JVAE_LAUNCH_CHECK();
    return 0;
}
