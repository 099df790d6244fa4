// Kernel selection for one (transposed) convolution, fp32 and bf16: geometry, the route, and the fp32 executors.
// Direction -> primitive mapping: see the conv_generic.hip header.
//
// Fast paths exist for the 5x5 "same-size / half-size" layers that carry >95 % of the FLOPs of conv32 / deconv32, in fp32 and
// bf16.  The bf16 layout also has kernels for the 3x3 padding-1 layers of vgg* / ivgg* / conv32- / deconv32- (the same kernel
// families at K = 3).  Everything else (7x7, 8x8, 4x4 heads, 3x3 padding-0 heads, odd sizes, and every 3x3 layer in fp32)
// takes the unfold + GEMM path in fp32 and has no bf16 kernel.
#include "common.h"
#include "conv_dispatch.h"
#include "conv_b8.h"
#include "pack_elems.h"

namespace {

inline bool is5(const ConvGeom& g) { return g.KH == 5 && g.KW == 5; }
// the 3x3 layers with a bf16 kernel: padding 1 ('same' at stride 1, half size at stride 2)
inline bool is3p1(const ConvGeom& g) { return g.KH == 3 && g.KW == 3 && g.P == 1; }
inline size_t max_sz(size_t a, size_t b) { return a > b ? a : b; }

// Transposed convolution of a 1x1 input with no padding (imager.0 of deconv32: 64 x 1 x 1 -> 64 x 8 x 8): the
// output IS the product x[n][ci] . w[ci][(co,kh,kw)] and the dgrad its transpose: plain GEMMs, no fold pass.
inline bool point_input(const ConvGeom& g) {
    return g.Hs == 1 && g.Ws == 1 && g.P == 0 && g.S == 1 && g.Hb == g.KH && g.Wb == g.KW;
}
// its weight gradient: few tiles, long K -> this many K pieces side by side
inline int point_wgrad_pieces(const ConvGeom& g) {
    const int want = (int)(1024 / ((long)cdiv(g.Cs, 64) * cdiv(g.Cb * g.KH * g.KW, 64)));
    return want < 1 ? 1 : (want > 8 ? 8 : want);
}

// The forward-type operator in (Ci, H, W) -> out (Co, OH, OW): from the big side (conv forward, transposed dgrad) or from the
// small side (conv dgrad, transposed forward)
struct FwdOp { int Ci, H, W, Co, OH, OW; };
inline FwdOp fwd_op(const ConvGeom& g, bool small_in) {
    return small_in ? FwdOp{g.Cs, g.Hs, g.Ws, g.Cb, g.Hb, g.Wb} : FwdOp{g.Cb, g.Hb, g.Wb, g.Cs, g.Hs, g.Ws};
}
// The weight-gradient operator dW[a][b][tap] = sum Ps[a] Q[b]: Ps on the folded grid, Q unfolded; swapped, the big side is Ps
struct WgOp { int Ca, HS, WS, Cb, HB, WB; };
inline WgOp wg_op(const ConvGeom& g, bool swap) {
    return swap ? WgOp{g.Cb, g.Hb, g.Wb, g.Cs, g.Hs, g.Ws} : WgOp{g.Cs, g.Hs, g.Ws, g.Cb, g.Hb, g.Wb};
}

// The deferred BatchNorm's coefficient table of smallco and of the bf16 kernels holds 256 input channels; the bf16 kernels have
// ReLU only (cvae.set_compute_dtype refuses 'leaky')
inline bool b8_aff_ok(int Cin, const CallFlags& f) { return (Cin + 7) / 8 * 8 <= 256 && f.aff != 2; }

ConvRoute fwd_route(const ConvGeom& g, int transposed, ConvDir dir, bool b8, const CallFlags& f) {
    const bool small_in = (dir == CONV_FWD) == (transposed != 0);
    const FwdOp o = fwd_op(g, small_in);
    ConvRoute r{CK_NONE, small_in, small_in ? 1 : g.S, small_in ? g.KH - 1 - g.P : g.P, 0, 0, false};
    if (!b8 && transposed && point_input(g)) {
        r.k = CK_POINT;
        if (!small_in) r.ws = 4 * (size_t)16 * g.N * g.Cs;         // dgrad: K pieces of dx
        return r;
    }
    if (!b8 && dir == CONV_FWD && !transposed && jvae_conv5_smallco_ok(g.Cb, g.Hb, g.Wb, g.Cs, g.KH, g.KW, g.S, g.P)) {
        r.k = CK_SMALLCO;
        r.aff_ok = g.Cb <= 256;
        return r;
    }
    // The gradient with respect to the input IMAGE (features.0 of conv32 / conv32+: dy with 32 channels -> dx with 3): the training step
    // never asks for it (its input needs no gradient); before this route it took CK_FWD5_X3 - the split-bf16 matrix-core kernel with 3
    // useful output channels of its 32-wide tile.  The vector-ALU kernel of the image head, weights read swapped and flipped.
    if (!b8 && dir == CONV_DGRAD && !transposed && g.Hs == g.Hb && g.Ws == g.Wb &&
        jvae_conv5_smallco_ok(g.Cs, g.Hb, g.Wb, g.Cb, g.KH, g.KW, g.S, g.P)) {
        r.k = CK_SMALLCO_DG;
        return r;
    }
    if (small_in && g.S == 2) {     // stride-2 small -> big: the 4-phase kernels
        if (b8 && jvae_convt2_b8_ok(g.Cs, g.Hs, g.Ws, g.Cb, g.Hb, g.Wb, g.KH, g.KW, g.S, g.P) && !f.y_f32) {
            r = ConvRoute{CK_T2_B8, true, 2, g.P, jvae_conv5_b8_pack_bytes(g.Cs, g.Cb, g.KH), jvae_conv5_b8_max_splits(g.N, g.Ws),
                          b8_aff_ok(g.Cs, f)};
        } else if (!b8 && jvae_convt2_ok(g.Cs, g.Hs, g.Ws, g.Cb, g.Hb, g.Wb, g.KH, g.KW, g.S, g.P)) {
            r = ConvRoute{jvae_convt2_x3_ok(g.N, g.Cs, g.Ws, g.Cb) ? CK_T2_X3 : CK_T2, true, 2, g.P,
                          4 * jvae_conv5_pack_floats(g.Cs, g.Cb), jvae_conv5_fwd_max_splits(g.N, g.Ws), true};
        }
    } else if ((is5(g) || (b8 && is3p1(g))) && (!small_in || g.S == 1)) {      // the implicit 5x5 (and bf16 3x3) kernels
        if (b8 && jvae_conv5_b8_fwd_ok(o.Ci, o.H, o.W, o.Co, o.OH, o.OW, r.S, r.P, g.KH)) {
            r.k = CK_B8;
            r.ws = jvae_conv5_b8_pack_bytes(o.Ci, o.Co, g.KH);
            r.splits = jvae_conv5_b8_max_splits(g.N, o.OW);
            r.aff_ok = b8_aff_ok(o.Ci, f);
        } else if (!b8 && jvae_conv5_fwd_ok(o.Ci, o.H, o.W, o.Co, o.OH, o.OW, r.S, r.P)) {
            // stride-1 layers with >= 16 input channels: the split-bf16 kernel (conv_x3.hip).  <= 4 input channels: vector ALUs
            // (conv_smallco.hip) - for the DGRAD role only (no bias, no BatchNorm sums: the image head's dgrad, 68 -> 56 us).  The first
            // layer's FORWARD gains 3 us there (47 -> 44) and stays on the fp32 kernel: another summation order moves its outputs by 1e-7,
            // which at the small-batch goldens flips single ReLU units further up (b2_n8_vib: one unit of features.13, global gradient
            // norm 3e-4 off instead of 2e-6; tests/diagnostics/vib_grad_diag.py).
            if (jvae_conv5_x3_ok(o.Ci, o.H, o.W, o.Co, o.OW, o.OW, r.S, r.P)) r.k = CK_FWD5_X3;
            else if (!f.aff && jvae_conv5_smallci_ok(o.Ci, o.H, o.W, o.Co, o.OW, r.S, r.P, !f.bias && !f.stats)) r.k = CK_SMALLCI;
            else r.k = CK_FWD5;
            r.ws = 4 * jvae_conv5_pack_floats(o.Ci, o.Co);            // any of the three packed forms
            r.splits = jvae_conv5_fwd_max_splits(g.N, o.OW);
            r.aff_ok = true;
        }
    }
    if (r.k == CK_NONE && !b8) r = ConvRoute{CK_GENERIC, small_in, g.S, g.P, 0, 0, false};
    return r;
}

ConvRoute wgrad_route(const ConvGeom& g, int transposed, bool b8, const CallFlags& f) {
    // role swap when the folded side has very few channels (Conv 32 -> 3): fp32 < 16, bf16 <= 8 (the 8-channel side becomes `b`)
    const int few = b8 ? 8 : 15;
    const bool swap = g.S == 1 && g.Cs <= few && g.Cb > few && g.Hs == g.Hb;
    const WgOp o = wg_op(g, swap);
    ConvRoute r{CK_NONE, swap, swap ? 1 : g.S, swap ? g.KH - 1 - g.P : g.P, 0, 0, false};
    if ((is5(g) || is3p1(g)) && b8 && jvae_conv5_wgrad_b8_ok(o.Ca, o.HS, o.WS, o.Cb, o.HB, o.WB, r.S, r.P, g.KH)) {
        // the LDS image and read-ahead pipeline of the split-bf16 kernel, one plane (conv_wgrad_x3.hip, 5x5 only); the older
        // kernel otherwise
        const bool x = is5(g) && jvae_conv5_wgrad_b8x_ok(o.Ca, o.WS, o.WS, o.Cb, o.WS * r.S, o.WS * r.S, r.S, r.P);
        r.k = x ? CK_WG_B8X : CK_WG_B8;
        r.ws = 4 * jvae_conv5_wgrad_b8_ws_floats(g.N, o.Ca, o.Cb, g.KH);
        r.aff_ok = f.aff != 2;
    } else if (is5(g) && !b8 && jvae_conv5_wgrad_ok(o.Ca, o.HS, o.WS, o.Cb, o.HB, o.WB, r.S, r.P)) {
        const bool x = jvae_conv5_wgrad_x3_ok(o.Ca, o.WS, o.WS, o.Cb, o.WS * r.S, o.WS * r.S, r.S, r.P);
        r.k = x ? CK_WG5_X3 : CK_WG5;
        r.ws = 4 * jvae_conv5_wgrad_ws_floats(g.N, o.Ca, o.Cb, r.S, o.WS);
        r.aff_ok = true;
    } else if (!b8 && transposed && point_input(g)) {
        r.k = CK_POINT;
        r.ws = 4 * (size_t)point_wgrad_pieces(g) * g.Cs * g.Cb * g.KH * g.KW;
    } else if (!b8) {
        r.k = CK_GENERIC;
    }
    return r;
}

// fp32 operand of the 4-phase kernel: the step's cache slot (pack_cache.hip) or the call's workspace; nullptr: launch error
inline const float* packed_f32(const float* w, float* ws, int C, int O, int swap, int flip, hipStream_t st) {
    return (const float*)jvae_packed(JVAE_PACK_F32, w, C, O, swap, flip, ws,
                                     [&](void* dst) { return jvae_conv5_pack(w, (float*)dst, C, O, swap, flip, st); });
}

}  // namespace

bool jvae_make_geom(int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                    ConvGeom* g, int* OH, int* OW) {
    if (N < 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || KH <= 0 || KW <= 0 || S <= 0 || P < 0 || OP < 0)
        return false;
    g->N = N; g->KH = KH; g->KW = KW; g->S = S; g->P = P;
    if (!transposed) {
        if (OP != 0) return false;
        *OH = (H + 2 * P - KH) / S + 1;
        *OW = (W + 2 * P - KW) / S + 1;
        g->Cb = Cin; g->Hb = H; g->Wb = W;
        g->Cs = Cout; g->Hs = *OH; g->Ws = *OW;
    } else {
        if (OP >= S && OP != 0) return false;
        *OH = (H - 1) * S - 2 * P + KH + OP;
        *OW = (W - 1) * S - 2 * P + KW + OP;
        g->Cs = Cin; g->Hs = H; g->Ws = W;
        g->Cb = Cout; g->Hb = *OH; g->Wb = *OW;
    }
    return *OH > 0 && *OW > 0;
}

ConvRoute jvae_conv_route(const ConvGeom& g, int transposed, ConvDir dir, ConvLayout layout, CallFlags f) {
    if (dir == CONV_WGRAD) return wgrad_route(g, transposed, layout == CONV_B8, f);
    return fwd_route(g, transposed, dir, layout == CONV_B8, f);
}

size_t jvae_conv_ws(const ConvGeom& g, int transposed) {
    size_t a = max_sz(jvae_conv_generic_ws(g), jvae_channel_sum_ws_bytes(g.Cb > g.Cs ? g.Cb : g.Cs));   // + the bias gradient's sum
    for (ConvDir d : {CONV_FWD, CONV_DGRAD, CONV_WGRAD}) a = max_sz(a, jvae_conv_route(g, transposed, d, CONV_F32, {}).ws);
    // reserved beyond the routes' needs, as the query has always been sized: the 5x5 weight re-pack of the big -> small role and
    // the point-input weight gradient's largest number of K pieces
    if (is5(g)) a = max_sz(a, 4 * jvae_conv5_pack_floats(g.Cb, g.Cs));
    if (transposed && point_input(g)) a = max_sz(a, 4 * (size_t)8 * g.Cs * g.Cb * g.KH * g.KW);
    return a;
}

int jvae_conv_run_fwd(const ConvRoute& r, const ConvGeom& g, const float* in, const float* w, const float* bias, float* out,
                      float* ws, size_t ws_bytes, hipStream_t st, float* stats, int* nsplit, const InAff* aff) {
    const FwdOp o = fwd_op(g, r.swap);
    const int sw = r.swap ? 1 : 0;
    switch (r.k) {
        case CK_SMALLCO: return jvae_conv5_smallco(in, w, bias, out, g.N, g.Cb, g.Wb, g.Cs, st, aff);
        case CK_SMALLCO_DG: return jvae_conv5_smallco_dgrad(in, w, out, g.N, g.Cs, g.Wb, g.Cb, st);
        case CK_SMALLCI: return jvae_conv5_smallci(in, w, sw, sw, bias, out, g.N, o.Ci, o.W, o.Co, ws, st, stats, nsplit);
        case CK_FWD5_X3:
            return jvae_conv5_x3_fwd(in, w, sw, sw, bias, out, g.N, o.Ci, o.H, o.W, o.Co, o.OW, r.S, r.P, ws, st, stats, nsplit, aff);
        case CK_FWD5:
            return jvae_conv5_fwd(in, w, sw, sw, bias, out, g.N, o.Ci, o.H, o.W, o.Co, o.OW, r.S, r.P, ws, st, stats, nsplit, aff);
        case CK_T2_X3: return jvae_convt2_x3(in, w, bias, out, g.N, g.Cs, g.Ws, g.Cb, ws, st, stats, nsplit, aff);
        case CK_T2: {
            const float* wp = packed_f32(w, ws, g.Cs, g.Cb, 1, 0, st);
            if (!wp) return JVAE_EINVAL;
            return jvae_convt2(in, wp, bias, out, g.N, g.Cs, g.Ws, g.Cb, st, stats, nsplit, aff);
        }
        case CK_POINT: {
            const int cols = g.Cb * g.KH * g.KW;
            if (r.swap)     // forward: y[n][(co,kh,kw)] = sum_ci x[n][ci] w[ci][(co,kh,kw)] + bias[co]
                return jvae_gemm_launch_ex(g.N, cols, g.Cs, 1, in, g.Cs, 1, 0, w, cols, 1, 0, out, cols, 1, 0,
                                           bias, bias ? 1 : 0, g.KH * g.KW, 0, 1, st);
            // dgrad: dx[n][ci] = sum_j dy[n][j] w[ci][j]: few tiles, long K -> K pieces, stored side by side and folded in a
            // fixed order (deterministic)
            const long outf = (long)g.N * g.Cs;
            int S = 0;
            int rc = jvae_gemm_launch_part(g.N, g.Cs, cols, 1, in, cols, 1, 0, w, 1, cols, 0, ws, g.Cs, 1, 0, outf, 16, &S, st);
            if (rc) return rc;
            return jvae_splitk_fold(ws, nullptr, out, S, outf, g.Cs, 0, 0, st);
        }
        case CK_GENERIC:
            return r.swap ? jvae_fold_bwd(g, in, w, bias, out, ws, ws_bytes, st) : jvae_fold_fwd(g, in, w, bias, out, ws, ws_bytes, st);
        default: return JVAE_ENOTSUP;
    }
}

int jvae_conv_run_wgrad(const ConvRoute& r, const ConvGeom& g, int transposed, const float* x, const float* dy, float* dw,
                        float* ws, size_t ws_bytes, hipStream_t st, const InAff* aff) {
    const float *ps, *q;
    const InAff *aff_p, *aff_q;
    jvae_wgrad_operands(r, transposed, x, dy, aff, &ps, &q, &aff_p, &aff_q);
    const WgOp o = wg_op(g, r.swap);
    const float* big = transposed ? dy : x;       // unfolded side
    const float* small = transposed ? x : dy;     // folded side
    // the entry point zeroed dw (or holds the value to accumulate onto): always accumulate here
    switch (r.k) {
        case CK_WG5_X3:
            return jvae_conv5_wgrad_x3(ps, q, dw, 1, r.swap, g.N, o.Ca, o.WS, o.Cb, r.S, r.P, ws, st,
                                       aff_p, aff_q);
        case CK_WG5:
            return jvae_conv5_wgrad(ps, q, dw, 1, r.swap, g.N, o.Ca, o.WS, o.Cb, r.S, r.P, ws, st,
                                    aff_p, aff_q);
        case CK_POINT: {
            // ConvTranspose2d of a 1x1 input (imager.0): unfolding the kxk output at its single position is the identity, so
            // dW[ci][j] (+)= sum_n x[n][ci] dy[n][j] is a plain product of the two tensors as they lie in memory (the generic path
            // copied dy into a col buffer first and ran 64 workgroups over K = N: 60 us of a 4 ms step).  K pieces stored side by
            // side, folded onto dw in a fixed order (deterministic).
            const int cols = g.Cb * g.KH * g.KW;
            const long outf = (long)g.Cs * cols;
            int S = 0;
            int rc = jvae_gemm_launch_part(g.Cs, cols, g.N, 1, small, 1, g.Cs, 0, big, cols, 1, 0, ws, cols, 1, 0, outf,
                                           point_wgrad_pieces(g), &S, st);
            if (rc) return rc;
            return jvae_splitk_fold(ws, nullptr, dw, S, outf, cols, 0, 1, st);
        }
        case CK_GENERIC: return jvae_fold_wgrad(g, big, small, dw, ws, ws_bytes, st);
        default: return JVAE_ENOTSUP;
    }
}
