// C-ABI entry points for (transposed) fp32 convolution: argument checks, then the geometry and the route of conv_dispatch.hip,
// the workspace checked against the route's need, the route executed.  See include/jvae_hip.h for the contract of each function.
#include "common.h"
#include "jvae_internal.h"
#include "conv_dispatch.h"

namespace {

inline ConvRoute route(const ConvGeom& g, int transposed, ConvDir dir, CallFlags f = {}) {
    return jvae_conv_route(g, transposed, dir, CONV_F32, f);
}

// Forward AND weight gradient of this layer can apply a deferred BatchNorm to the layer input while staging it (the route
// of one of the two directions given: r)
bool affine_ok(const ConvGeom& g, int transposed, ConvDir other, const ConvRoute& r) {
    return r.aff_ok && route(g, transposed, other, {false, false, false, 1}).aff_ok;
}

// the three forward entry points; nsplit: host int or NULL
int fwd_f32(const float* x, const float* w, const float* bias, float* y, float* stats, int* nsplit, const InAff* aff,
            int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
            void* ws, size_t ws_bytes, void* stream) {
    ConvGeom g; int oh, ow;
    if (nsplit) *nsplit = 0;
    if (!jvae_make_geom(N, Cin, H, W, Cout, KH, KW, S, P, OP, transposed, &g, &oh, &ow)) return JVAE_EINVAL;
    const ConvRoute r = route(g, transposed, CONV_FWD, {bias != nullptr, stats != nullptr, false, jvae_aff_kind(aff)});
    if (aff && !affine_ok(g, transposed, CONV_WGRAD, r)) return JVAE_ENOTSUP;
    if (N == 0) return 0;
    if (jvae_ws_short(r, ws, ws_bytes)) return JVAE_EWORKSPACE;
    return jvae_conv_run_fwd(r, g, x, w, bias, y, (float*)ws, ws_bytes, (hipStream_t)stream, stats, nsplit, aff);
}

int wgrad_f32(const float* x, const float* dy, float* dw, float* dbias, int accumulate, const InAff* aff,
              int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
              void* ws, size_t ws_bytes, void* stream) {
    ConvGeom g; int oh, ow;
    if (!dw || (N > 0 && (!x || !dy))) return JVAE_EINVAL;
    if (!jvae_make_geom(N, Cin, H, W, Cout, KH, KW, S, P, OP, transposed, &g, &oh, &ow)) return JVAE_EINVAL;
    const ConvRoute r = route(g, transposed, CONV_WGRAD, {false, false, false, jvae_aff_kind(aff)});
    if (aff && !affine_ok(g, transposed, CONV_FWD, r)) return JVAE_ENOTSUP;
    if (N > 0 && jvae_ws_short(r, ws, ws_bytes)) return JVAE_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (!accumulate) {
        hipError_t e = hipMemsetAsync(dw, 0, sizeof(float) * (size_t)Cin * Cout * KH * KW, st);
        if (e != hipSuccess) return (int)e;
    }
    if (N == 0) {
        if (dbias && !accumulate) {
            hipError_t e = hipMemsetAsync(dbias, 0, sizeof(float) * (size_t)Cout, st);
            if (e != hipSuccess) return (int)e;
        }
        return 0;
    }
    int rc = jvae_conv_run_wgrad(r, g, transposed, x, dy, dw, (float*)ws, ws_bytes, st, aff);
    if (rc) return rc;
    if (dbias) rc = jvae_channel_sum(dy, dbias, N, Cout, oh * ow, accumulate, (float*)ws, ws_bytes, st);   // ws is free again
    return rc;
}

}  // namespace

extern "C" {

int jvae_conv2d_set_split_bf16(int mode) { return jvae_conv5_x3_set(mode); }
int jvae_conv2d_set_split_shape16(int on) { return jvae_conv5_x3_set_shape16(on); }

size_t jvae_conv2d_workspace_bytes(int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP,
                                   int transposed) {
    ConvGeom g; int oh, ow;
    if (!jvae_make_geom(N, Cin, H, W, Cout, KH, KW, S, P, OP, transposed, &g, &oh, &ow)) return 0;
    return jvae_conv_ws(g, transposed);
}

// Host-only: the route the entry points of either layout take for this call (nothing is initialised on the device)
int jvae_conv2d_route(int dir, int layout, int bias, int stats, int y_f32, int aff_kind,
                      int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                      int* kernel, int* swap, size_t* ws_bytes, int* splits, int* aff_ok) {
    ConvGeom g; int oh, ow;
    if (dir != CONV_FWD && dir != CONV_DGRAD && dir != CONV_WGRAD) return JVAE_EINVAL;
    if ((layout != CONV_F32 && layout != CONV_B8) || aff_kind < 0 || aff_kind > 2) return JVAE_EINVAL;
    if (!jvae_make_geom(N, Cin, H, W, Cout, KH, KW, S, P, OP, transposed, &g, &oh, &ow)) return JVAE_EINVAL;
    const ConvRoute r = jvae_conv_route(g, transposed, (ConvDir)dir, (ConvLayout)layout,
                                        {bias != 0, stats != 0, y_f32 != 0, aff_kind});
    if (kernel) *kernel = (int)r.k;
    if (swap) *swap = r.swap ? 1 : 0;
    if (ws_bytes) *ws_bytes = r.ws;
    if (splits) *splits = r.splits;
    if (aff_ok) *aff_ok = r.aff_ok ? 1 : 0;
    return 0;
}

const char* jvae_conv2d_kernel_name(int kernel) {
    switch (kernel) {
#define JVAE_CK_NAME(k) case k: return #k;
        JVAE_CK_NAME(CK_NONE) JVAE_CK_NAME(CK_GENERIC) JVAE_CK_NAME(CK_POINT) JVAE_CK_NAME(CK_SMALLCO)
        JVAE_CK_NAME(CK_SMALLCI) JVAE_CK_NAME(CK_FWD5) JVAE_CK_NAME(CK_FWD5_X3) JVAE_CK_NAME(CK_T2) JVAE_CK_NAME(CK_T2_X3)
        JVAE_CK_NAME(CK_WG5) JVAE_CK_NAME(CK_WG5_X3) JVAE_CK_NAME(CK_B8) JVAE_CK_NAME(CK_T2_B8) JVAE_CK_NAME(CK_WG_B8)
        JVAE_CK_NAME(CK_WG_B8X) JVAE_CK_NAME(CK_SMALLCO_DG)
#undef JVAE_CK_NAME
        default: return nullptr;
    }
}

int jvae_conv2d_out_shape(int H, int W, int KH, int KW, int S, int P, int OP, int transposed, int* OH, int* OW) {
    ConvGeom g;
    if (!OH || !OW) return JVAE_EINVAL;
    return jvae_make_geom(1, 1, H, W, 1, KH, KW, S, P, OP, transposed, &g, OH, OW) ? 0 : JVAE_EINVAL;
}

int jvae_conv2d_fwd_f32(const float* x, const float* w, const float* bias, float* y,
                        int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                        void* ws, size_t ws_bytes, void* stream) {
    if (!w || (N > 0 && (!x || !y))) return JVAE_EINVAL;          // an empty batch has no activations to point at
    return fwd_f32(x, w, bias, y, nullptr, nullptr, nullptr, N, Cin, H, W, Cout, KH, KW, S, P, OP, transposed, ws, ws_bytes,
                   stream);
}

// Forward that also emits BatchNorm partial statistics of (y - bias) when the selected kernel can produce them.
// stats: (Cout, stats_cap, 2) floats with stats_cap >= jvae_conv2d_stats_splits(...); *nsplit (HOST int) receives the
// number of partials per channel actually written, laid out as (Cout, *nsplit, 2); 0 = not produced (run the BN
// statistics kernel instead).
int jvae_conv2d_stats_splits(int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed) {
    ConvGeom g; int oh, ow;
    if (!jvae_make_geom(N, Cin, H, W, Cout, KH, KW, S, P, OP, transposed, &g, &oh, &ow)) return 0;
    return route(g, transposed, CONV_FWD, {false, true, false, 0}).splits;
}

int jvae_conv2d_fwd_stats_f32(const float* x, const float* w, const float* bias, float* y, float* stats, int* nsplit,
                              int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                              void* ws, size_t ws_bytes, void* stream) {
    if (!w || !nsplit || (N > 0 && (!x || !y))) return JVAE_EINVAL;
    return fwd_f32(x, w, bias, y, stats, nsplit, nullptr, N, Cin, H, W, Cout, KH, KW, S, P, OP, transposed, ws, ws_bytes, stream);
}

// ---- deferred BatchNorm on the layer input (DESIGN.md "Streams, fusion"): a = [relu](x*in_scale[c] + in_shift[c]) is
// applied while the kernel stages x, for the layers whose forward AND weight gradient run on the implicit kernels.
int jvae_conv2d_affine_ok(int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed) {
    ConvGeom g; int oh, ow;
    if (!jvae_make_geom(N, Cin, H, W, Cout, KH, KW, S, P, OP, transposed, &g, &oh, &ow)) return 0;
    return affine_ok(g, transposed, CONV_WGRAD, route(g, transposed, CONV_FWD, {false, false, false, 1})) ? 1 : 0;
}

int jvae_conv2d_fwd_aff_f32(const float* x, const float* w, const float* bias, float* y, float* stats, int* nsplit,
                            const float* in_scale, const float* in_shift, int in_relu,
                            int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                            void* ws, size_t ws_bytes, void* stream) {
    if (!w || !in_scale || !in_shift || (N > 0 && (!x || !y))) return JVAE_EINVAL;
    if (stats && !nsplit) return JVAE_EINVAL;
    const InAff aff{in_scale, in_shift, in_relu};
    return fwd_f32(x, w, bias, y, stats, nsplit, &aff, N, Cin, H, W, Cout, KH, KW, S, P, OP, transposed, ws, ws_bytes, stream);
}

int jvae_conv2d_wgrad_aff_f32(const float* x, const float* dy, float* dw, float* dbias, int accumulate,
                              const float* in_scale, const float* in_shift, int in_relu,
                              int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                              void* ws, size_t ws_bytes, void* stream) {
    if (!in_scale || !in_shift) return JVAE_EINVAL;
    const InAff aff{in_scale, in_shift, in_relu};
    return wgrad_f32(x, dy, dw, dbias, accumulate, &aff, N, Cin, H, W, Cout, KH, KW, S, P, OP, transposed, ws, ws_bytes, stream);
}

int jvae_conv2d_dgrad_f32(const float* dy, const float* w, float* dx,
                          int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                          void* ws, size_t ws_bytes, void* stream) {
    ConvGeom g; int oh, ow;
    if (!w || (N > 0 && (!dy || !dx))) return JVAE_EINVAL;
    if (!jvae_make_geom(N, Cin, H, W, Cout, KH, KW, S, P, OP, transposed, &g, &oh, &ow)) return JVAE_EINVAL;
    if (N == 0) return 0;
    const ConvRoute r = route(g, transposed, CONV_DGRAD);
    if (jvae_ws_short(r, ws, ws_bytes)) return JVAE_EWORKSPACE;
    return jvae_conv_run_fwd(r, g, dy, w, nullptr, dx, (float*)ws, ws_bytes, (hipStream_t)stream);
}

int jvae_conv2d_wgrad_f32(const float* x, const float* dy, float* dw, float* dbias, int accumulate,
                          int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                          void* ws, size_t ws_bytes, void* stream) {
    return wgrad_f32(x, dy, dw, dbias, accumulate, nullptr, N, Cin, H, W, Cout, KH, KW, S, P, OP, transposed, ws, ws_bytes, stream);
}

// out[c] (+)= sum over n, q of t[n][c][q]   (bias gradients of conv / linear layers)
size_t jvae_channel_sum_workspace_bytes(int C) { return jvae_channel_sum_ws_bytes(C); }

int jvae_channel_sum_f32(const float* t, float* out, int N, int C, int P, int accumulate, void* ws, size_t ws_bytes,
                         void* stream) {
    if (!t || !out || N < 0 || C <= 0 || P <= 0) return JVAE_EINVAL;
    return jvae_channel_sum(t, out, N, C, P, accumulate, (float*)ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
