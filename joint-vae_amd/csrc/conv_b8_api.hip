// C-ABI entry points of the bf16 "B8" convolution path: argument checks, then the geometry and the route of conv_dispatch.hip.
// A direction without a native bf16 kernel returns JVAE_ENOTSUP (jvae_conv2d_native_b8 tells in advance); the host then runs that
// layer through the fp32 kernels between two layout conversions.
#include "common.h"
#include "jvae_internal.h"
#include "conv_b8.h"
#include "conv_dispatch.h"

namespace {

// the kernel sizes of the bf16 kernel families (the route decides which geometries of them run)
inline bool has_b8_family(const ConvGeom& g) { return g.KH == g.KW && (g.KH == 5 || (g.KH == 3 && g.P == 1)); }
inline size_t chsum_ws_bytes(int C) { return (size_t)((C + 7) / 8) * 8 * 64 * 4; }
inline ConvRoute route(const ConvGeom& g, int transposed, ConvDir dir, CallFlags f = {}) {
    return jvae_conv_route(g, transposed, dir, CONV_B8, f);
}

// the forward-type directions: in B8 -> out B8 (or fp32 NCHW when y_f32)
int run_fwd(const ConvRoute& r, const ConvGeom& g, const void* in, const float* w, const float* bias, void* out, int y_f32,
            void* ws, hipStream_t st, float* stats = nullptr, int* nsplit = nullptr, const InAff* aff = nullptr) {
    const int sw = r.swap ? 1 : 0;
    if (r.k == CK_T2_B8) return jvae_convt2_b8(in, w, bias, out, g.N, g.Cs, g.Ws, g.Cb, ws, st, stats, nsplit, aff, g.KH);
    if (r.swap)
        return jvae_conv5_b8_fwd(in, w, sw, sw, bias, out, y_f32, g.N, g.Cs, g.Hs, g.Ws, g.Cb, g.Wb, r.S, r.P, ws, st, stats, nsplit, aff,
                                 g.KH);
    return jvae_conv5_b8_fwd(in, w, sw, sw, bias, out, y_f32, g.N, g.Cb, g.Hb, g.Wb, g.Cs, g.Ws, r.S, r.P, ws, st, stats, nsplit, aff,
                             g.KH);
}

int fwd_b8(const void* x, const float* w, const float* bias, void* y, int y_f32, float* stats, int* nsplit, const InAff* aff,
           int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
           void* ws, size_t ws_bytes, void* stream) {
    ConvGeom g; int oh, ow;
    if (stats && !nsplit) return JVAE_EINVAL;
    if (!jvae_make_geom(N, Cin, H, W, Cout, KH, KW, S, P, OP, transposed, &g, &oh, &ow)) return JVAE_EINVAL;
    if (N == 0) return 0;
    const ConvRoute r = route(g, transposed, CONV_FWD, {bias != nullptr, stats != nullptr, y_f32 != 0, jvae_aff_kind(aff)});
    if (r.k == CK_NONE || (aff && !r.aff_ok)) return JVAE_ENOTSUP;
    if (jvae_ws_short(r, ws, ws_bytes)) return JVAE_EWORKSPACE;
    return run_fwd(r, g, x, w, bias, y, y_f32, ws, (hipStream_t)stream, stats, nsplit, aff);
}

// x, dy: B8 (layer input / gradient of the layer output); dw fp32 in the layer's own layout; dbias may be NULL
int wgrad_b8(const void* x, const void* dy, float* dw, float* dbias, int accumulate, const InAff* aff,
             int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
             void* ws, size_t ws_bytes, void* stream) {
    ConvGeom g; int oh, ow;
    if (!dw || (N > 0 && (!x || !dy))) return JVAE_EINVAL;
    if (!jvae_make_geom(N, Cin, H, W, Cout, KH, KW, S, P, OP, transposed, &g, &oh, &ow)) return JVAE_EINVAL;
    const ConvRoute r = route(g, transposed, CONV_WGRAD, {false, false, false, jvae_aff_kind(aff)});
    if (r.k == CK_NONE || (aff && !r.aff_ok)) return JVAE_ENOTSUP;
    if (N > 0 && (!ws || ws_bytes < r.ws + (dbias ? chsum_ws_bytes(Cout) : 0))) return JVAE_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (!accumulate) {
        hipError_t e = hipMemsetAsync(dw, 0, sizeof(float) * (size_t)Cin * Cout * KH * KW, st);
        if (e != hipSuccess) return (int)e;
        if (dbias && (e = hipMemsetAsync(dbias, 0, sizeof(float) * (size_t)Cout, st)) != hipSuccess) return (int)e;
    }
    if (N == 0) return 0;
    const void *ps, *q;
    const InAff *aff_p, *aff_q;
    jvae_wgrad_operands(r, transposed, x, dy, aff, &ps, &q, &aff_p, &aff_q);
    const int Ca = r.swap ? g.Cb : g.Cs, WS = r.swap ? g.Wb : g.Ws, Cb = r.swap ? g.Cs : g.Cb;
    int rc = r.k == CK_WG_B8X
        ? jvae_conv5_wgrad_b8x(ps, q, dw, 1, r.swap, g.N, Ca, WS, Cb, r.S, r.P, (float*)ws, st, aff_p, aff_q)
        : jvae_conv5_wgrad_b8(ps, q, dw, 1, r.swap, g.N, Ca, WS, Cb, r.S, r.P, (float*)ws, st, aff_p, aff_q, KH);
    if (rc) return rc;
    if (dbias) rc = jvae_b8_channel_sum(dy, dbias, N, Cout, (long)oh * ow, 1, (float*)((char*)ws + r.ws), st);
    return rc;
}

int native_mask(const ConvGeom& g, int transposed) {
    int m = 0;
    for (ConvDir d : {CONV_FWD, CONV_DGRAD, CONV_WGRAD})
        if (route(g, transposed, d).k != CK_NONE) m |= d;
    return m;
}

}  // namespace

extern "C" {

int jvae_b8_pack_f32(const float* x, void* y, int N, int C, long HW, void* stream) {
    if (!x || !y || N < 0 || C <= 0 || HW <= 0) return JVAE_EINVAL;
    return jvae_b8_pack(x, y, N, C, HW, (hipStream_t)stream);
}

int jvae_b8_unpack_f32(const void* y, float* x, int N, int C, long HW, int accumulate, void* stream) {
    if (!x || !y || N < 0 || C <= 0 || HW <= 0) return JVAE_EINVAL;
    return jvae_b8_unpack(y, x, N, C, HW, accumulate, (hipStream_t)stream);
}

int jvae_conv2d_native_b8(int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed) {
    ConvGeom g; int oh, ow;
    if (!jvae_make_geom(N, Cin, H, W, Cout, KH, KW, S, P, OP, transposed, &g, &oh, &ow)) return 0;
    return native_mask(g, transposed);
}

size_t jvae_conv2d_workspace_bytes_b8(int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP,
                                      int transposed) {
    ConvGeom g; int oh, ow;
    if (!jvae_make_geom(N, Cin, H, W, Cout, KH, KW, S, P, OP, transposed, &g, &oh, &ow)) return 0;
    if (!has_b8_family(g)) return 0;
    // the weight re-pack of either forward-type direction; the weight gradient's slabs + its bias gradient's sum
    size_t a = jvae_conv5_b8_pack_bytes(g.Cb, g.Cs, g.KH), b = jvae_conv5_b8_pack_bytes(g.Cs, g.Cb, g.KH);
    if (b > a) a = b;
    const ConvRoute r = route(g, transposed, CONV_WGRAD);
    if (r.k != CK_NONE && (b = r.ws + chsum_ws_bytes(Cout)) > a) a = b;
    return a;
}

int jvae_conv2d_stats_splits_b8(int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed) {
    ConvGeom g; int oh, ow;
    if (!jvae_make_geom(N, Cin, H, W, Cout, KH, KW, S, P, OP, transposed, &g, &oh, &ow)) return 0;
    return route(g, transposed, CONV_FWD, {false, true, false, 0}).splits;
}

// x: B8; y: B8, or fp32 NCHW when y_f32.  stats (Cout, cap, 2) / nsplit as jvae_conv2d_fwd_stats_f32 (both may be NULL).
int jvae_conv2d_fwd_b8(const void* x, const float* w, const float* bias, void* y, int y_f32, float* stats, int* nsplit,
                       int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                       void* ws, size_t ws_bytes, void* stream) {
    if (nsplit) *nsplit = 0;
    if (!w || (N > 0 && (!x || !y))) return JVAE_EINVAL;          // an empty batch has no activations to point at
    return fwd_b8(x, w, bias, y, y_f32, stats, nsplit, nullptr, N, Cin, H, W, Cout, KH, KW, S, P, OP, transposed, ws, ws_bytes,
                  stream);
}

// ---- deferred BatchNorm(+ReLU) on the B8 layer input: in_scale / in_shift hold ceil(Cin/8)*8 floats (jvae_bn_finalize_b8)
int jvae_conv2d_affine_ok_b8(int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed) {
    ConvGeom g; int oh, ow;
    if (!jvae_make_geom(N, Cin, H, W, Cout, KH, KW, S, P, OP, transposed, &g, &oh, &ow)) return 0;
    const CallFlags f{false, false, false, 1};
    return route(g, transposed, CONV_FWD, f).aff_ok && route(g, transposed, CONV_WGRAD, f).aff_ok ? 1 : 0;
}

// in_relu = 2 (leaky ReLU): JVAE_ENOTSUP, the bf16 kernels have ReLU only
int jvae_conv2d_fwd_aff_b8(const void* x, const float* w, const float* bias, void* y, int y_f32, float* stats, int* nsplit,
                           const float* in_scale, const float* in_shift, int in_relu,
                           int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                           void* ws, size_t ws_bytes, void* stream) {
    if (nsplit) *nsplit = 0;
    if (!w || !in_scale || !in_shift || (N > 0 && (!x || !y))) return JVAE_EINVAL;
    const InAff aff{in_scale, in_shift, in_relu};
    return fwd_b8(x, w, bias, y, y_f32, stats, nsplit, &aff, N, Cin, H, W, Cout, KH, KW, S, P, OP, transposed, ws, ws_bytes,
                  stream);
}

// dy: B8 -> dx: B8
int jvae_conv2d_dgrad_b8(const void* dy, const float* w, void* dx,
                         int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                         void* ws, size_t ws_bytes, void* stream) {
    ConvGeom g; int oh, ow;
    if (!w || (N > 0 && (!dy || !dx))) return JVAE_EINVAL;
    if (!jvae_make_geom(N, Cin, H, W, Cout, KH, KW, S, P, OP, transposed, &g, &oh, &ow)) return JVAE_EINVAL;
    if (N == 0) return 0;
    const ConvRoute r = route(g, transposed, CONV_DGRAD);
    if (r.k == CK_NONE) return JVAE_ENOTSUP;
    if (jvae_ws_short(r, ws, ws_bytes)) return JVAE_EWORKSPACE;
    return run_fwd(r, g, dy, w, nullptr, dx, 0, ws, (hipStream_t)stream);
}

int jvae_conv2d_wgrad_b8(const void* x, const void* dy, float* dw, float* dbias, int accumulate,
                         int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                         void* ws, size_t ws_bytes, void* stream) {
    return wgrad_b8(x, dy, dw, dbias, accumulate, nullptr, N, Cin, H, W, Cout, KH, KW, S, P, OP, transposed, ws, ws_bytes, stream);
}

// in_relu = 2 (leaky ReLU): JVAE_ENOTSUP before anything is written, as jvae_conv2d_fwd_aff_b8
int jvae_conv2d_wgrad_aff_b8(const void* x, const void* dy, float* dw, float* dbias, int accumulate,
                             const float* in_scale, const float* in_shift, int in_relu,
                             int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                             void* ws, size_t ws_bytes, void* stream) {
    if (!in_scale || !in_shift) return JVAE_EINVAL;
    const InAff aff{in_scale, in_shift, in_relu};
    return wgrad_b8(x, dy, dw, dbias, accumulate, &aff, N, Cin, H, W, Cout, KH, KW, S, P, OP, transposed, ws, ws_bytes, stream);
}

}  // extern "C"
