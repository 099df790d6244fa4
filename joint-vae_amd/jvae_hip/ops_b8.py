"""bf16 activation path ("B8" layout) - wrappers around the *_b8 entry points of libjvae_hip.so.

A B8 tensor is a torch.bfloat16 tensor of shape (N, ceil(C/8), H, W, 8): eight consecutive channels of a pixel are
contiguous (csrc/conv_b8.hip).  Master weights, gradients of parameters, BatchNorm statistics and all loss math stay
fp32.  The layer ops themselves (convolution, BatchNorm) are those of ops.py; B8 is their description of this layout.
"""
from ctypes import byref, c_int

import torch

from . import lib as L
from . import ops as O
from .ops import FWD, DGRAD, WGRAD  # noqa: F401


def cblocks(C):
    return (C + 7) // 8


def pack(x):
    """fp32 (N, C, H, W) -> B8 (N, CB, H, W, 8) bf16."""
    x = O._c(O._f32(x, 'b8.pack'))
    N, C, H, W = x.shape
    y = torch.empty((N, cblocks(C), H, W, 8), device=x.device, dtype=torch.bfloat16)
    L.check(L.load().jvae_b8_pack_f32(L.ptr(x), L.ptr(y), N, C, H * W, L.stream_ptr()), 'jvae_b8_pack_f32')
    return y


def unpack(y, C, out=None, accumulate=False):
    """B8 -> fp32 (N, C, H, W)."""
    N, CB, H, W, e = y.shape
    assert e == 8 and CB == cblocks(C) and y.dtype == torch.bfloat16 and y.is_contiguous()
    if out is None:
        out = torch.empty((N, C, H, W), device=y.device, dtype=torch.float32)
        accumulate = False
    L.check(L.load().jvae_b8_unpack_f32(L.ptr(y), L.ptr(out), N, C, H * W, int(accumulate), L.stream_ptr()),
            'jvae_b8_unpack_f32')
    return out


def native_mask(spec, N, H, W):
    return O._geom_query('jvae_conv2d_native_b8', spec.geom(N, H, W))


def _ws(geom, device):
    nbytes = O._geom_query('jvae_conv2d_workspace_bytes_b8', geom)
    ws = L.workspace(max(nbytes, 16), device)
    return ws, ws.numel()


def conv_affine_ok(spec, N, H, W):
    """Forward and weight gradient of this layer run on bf16 kernels that can apply a deferred BatchNorm to the input."""
    return bool(O._geom_query('jvae_conv2d_affine_ok_b8', spec.geom(N, H, W)))


def conv_fwd_raw(x, w, b, spec, out_f32=False, want_stats=False, aff=None):
    """x: B8.  -> (y, stats, nsplit); y is B8, or fp32 NCHW with out_f32.  Raises JvaeHipError(ENOTSUP) when the geometry
    has no native bf16 kernel (ask native_mask first)."""
    lib = L.load()
    N, _, H, W, _ = x.shape
    geom = spec.geom(N, H, W)
    oh, ow = spec.out_hw(H, W)
    if out_f32:
        y = torch.empty((N, spec.cout, oh, ow), device=x.device, dtype=torch.float32)
    else:
        y = torch.empty((N, cblocks(spec.cout), oh, ow, 8), device=x.device, dtype=torch.bfloat16)
    stats, ns = None, c_int(0)
    if want_stats:
        cap = O._geom_query('jvae_conv2d_stats_splits_b8', geom)
        if cap > 0:
            stats = torch.empty((spec.cout * cap * 2,), device=x.device, dtype=torch.float32)
    ws, nb = _ws(geom, x.device)
    if aff is not None:
        rc = lib.jvae_conv2d_fwd_aff_b8(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), int(out_f32), L.ptr(stats), byref(ns),
                                        L.ptr(aff[0]), L.ptr(aff[1]), int(aff[2]), *geom, L.ptr(ws), nb, L.stream_ptr())
    else:
        rc = lib.jvae_conv2d_fwd_b8(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), int(out_f32), L.ptr(stats), byref(ns), *geom,
                                    L.ptr(ws), nb, L.stream_ptr())
    L.check(rc, 'jvae_conv2d_fwd_b8')
    return y, (stats if ns.value > 0 else None), ns.value


def conv_dgrad_raw(gy, w, spec, N, H, W):
    """gy: B8 of the layer output -> B8 gradient of the layer input (N, cblocks(cin), H, W, 8)."""
    gx = torch.empty((N, cblocks(spec.cin), H, W, 8), device=gy.device, dtype=torch.bfloat16)
    geom = spec.geom(N, H, W)
    ws, nb = _ws(geom, gy.device)
    rc = L.load().jvae_conv2d_dgrad_b8(L.ptr(gy), L.ptr(w), L.ptr(gx), *geom, L.ptr(ws), nb, L.stream_ptr())
    L.check(rc, 'jvae_conv2d_dgrad_b8')
    return gx


def conv_wgrad_raw(x, gy, spec, wshape, want_bias, w_slot=None, b_slot=None, aff=None):
    """x, gy: B8.  -> (gw, gb) fp32; with slots the result is ADDED into them (see ops.conv_wgrad_raw).
    aff = (scale, shift, relu): x is a pre-BatchNorm tensor normalised while it is staged."""
    N, _, H, W, _ = x.shape
    inplace = w_slot is not None and (b_slot is not None or not want_bias)
    gw = w_slot if inplace else torch.empty(wshape, device=x.device, dtype=torch.float32)
    gb = None
    if want_bias:
        gb = b_slot if inplace else torch.empty(spec.cout, device=x.device, dtype=torch.float32)
    geom = spec.geom(N, H, W)
    ws, nb = _ws(geom, x.device)
    if aff is not None:
        rc = L.load().jvae_conv2d_wgrad_aff_b8(L.ptr(x), L.ptr(gy), L.ptr(gw), L.ptr(gb), int(inplace),
                                               L.ptr(aff[0]), L.ptr(aff[1]), int(aff[2]), *geom, L.ptr(ws), nb,
                                               L.stream_ptr())
    else:
        rc = L.load().jvae_conv2d_wgrad_b8(L.ptr(x), L.ptr(gy), L.ptr(gw), L.ptr(gb), int(inplace), *geom, L.ptr(ws), nb,
                                           L.stream_ptr())
    L.check(rc, 'jvae_conv2d_wgrad_b8')
    return (None, None) if inplace else (gw, gb)


# ----------------------------------------------------------------------------------------- layout
def is_b8(t):
    return t.dtype == torch.bfloat16 and t.dim() == 5 and t.shape[-1] == 8


class _Pack(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.C = x.shape[1]
        return pack(x)

    @staticmethod
    def backward(ctx, gy):
        return unpack(O._c(gy), ctx.C)


class _Unpack(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xb, C):
        return unpack(xb, C)

    @staticmethod
    def backward(ctx, gy):
        return pack(gy), None


def to_b8(x):
    return _Pack.apply(x)


def from_b8(xb, C):
    return _Unpack.apply(xb, C)


class B8Layout(O.Layout):
    """ops.Layout of the B8 layout: its own entry points and workspace query, C passed in, coefficient rows padded to whole
    channel blocks, native directions from native_mask, ReLU as its only activation."""
    sfx = ws_sfx = '_b8'
    acts = {O.IDENT: 0, O.RELU: 1}

    def dims(self, x, C):
        N, _, H, W, _ = x.shape
        return N, C, H * W

    def coef_width(self, C):
        return cblocks(C) * 8

    def prep(self, x, what):
        return O._c(x)

    def to_f32(self, t, C):
        return unpack(t, C)

    def from_f32(self, t):
        return pack(t)

    def native(self, spec, N, H, W):
        return native_mask(spec, N, H, W)

    def affine_ok(self, spec, N, H, W):
        return conv_affine_ok(spec, N, H, W)

    def conv_fwd(self, x, w, b, spec, want_stats, aff, out_f32):
        return conv_fwd_raw(x, w, b, spec, out_f32=out_f32, want_stats=want_stats, aff=aff)

    def conv_dgrad(self, gy, w, spec, N, H, W):
        return conv_dgrad_raw(gy, w, spec, N, H, W)

    def conv_wgrad(self, *args):
        return conv_wgrad_raw(*args)

    def bn_fwd(self, *args, ext, ws):
        self.bn('jvae_bn_fwd', *args, *ext, ws=ws)            # nullable sums

    def coef_args(self, coef):
        return (L.ptr(coef),)                                  # one (2, CB*8) block

    def bn_bwd_sync(self, *args, ws):
        self.bn('jvae_bn_bwd_sync', *args, ws=ws)


B8 = B8Layout()


# the BatchNorm ops of ops.py on a B8 tensor of C channels (same arguments after C)
def batchnorm_act(x, C, *args, **kw):
    return O.batchnorm_act(x, *args, C=C, **kw)


def batchnorm_defer(x, C, *args, **kw):
    return O.batchnorm_defer(x, *args, C=C, **kw)


def sync_batchnorm_act(x, C, *args, **kw):
    return O.sync_batchnorm_act(x, *args, C=C, **kw)


class _ReluB8(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = O._c(x)
        y = torch.empty_like(x)
        L.check(L.load().jvae_relu_fwd_b8(L.ptr(x), L.ptr(y), x.numel() // 8, L.stream_ptr()), 'jvae_relu_fwd_b8')
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, gy):
        y, = ctx.saved_tensors
        gy = O._c(gy)
        gx = torch.empty_like(gy)
        L.check(L.load().jvae_relu_bwd_b8(L.ptr(gy), L.ptr(y), L.ptr(gx), y.numel() // 8, L.stream_ptr()), 'jvae_relu_bwd_b8')
        return gx


def relu(x):
    return _ReluB8.apply(x)


# ------------------------------------------------------------------------------- pooling / up-sampling
def pool2d_fwd_raw(x, K, S, P, mode):
    """x: B8 -> (y B8, idx int32 (N, CB, OH, OW, 8) for max pooling, else None)."""
    x = O._c(x)
    N, CB, H, W, _ = x.shape
    oh, ow = c_int(0), c_int(0)
    L.check(L.load().jvae_pool2d_out_shape(H, W, K, S, P, byref(oh), byref(ow)), 'pool2d_out_shape')
    y = torch.empty((N, CB, oh.value, ow.value, 8), device=x.device, dtype=torch.bfloat16)
    idx = torch.empty(y.shape, device=x.device, dtype=torch.int32) if mode == O.POOL_MAX else None
    L.check(L.load().jvae_pool2d_fwd_b8(L.ptr(x), L.ptr(y), L.ptr(idx), N * CB, H, W, K, S, P, mode, L.stream_ptr()),
            'jvae_pool2d_fwd_b8')
    return y, idx


def pool2d_bwd_raw(gy, idx, H, W, K, S, P, mode):
    gy = O._c(gy)
    N, CB = gy.shape[:2]
    gx = torch.empty((N, CB, H, W, 8), device=gy.device, dtype=torch.bfloat16)
    L.check(L.load().jvae_pool2d_bwd_b8(L.ptr(gy), L.ptr(idx), L.ptr(gx), N * CB, H, W, K, S, P, mode, L.stream_ptr()),
            'jvae_pool2d_bwd_b8')
    return gx


def upsample_nearest_fwd_raw(x, scale):
    x = O._c(x)
    N, CB, H, W, _ = x.shape
    y = torch.empty((N, CB, H * scale, W * scale, 8), device=x.device, dtype=torch.bfloat16)
    L.check(L.load().jvae_upsample_nearest_fwd_b8(L.ptr(x), L.ptr(y), N * CB, H, W, scale, L.stream_ptr()),
            'jvae_upsample_nearest_fwd_b8')
    return y


def upsample_nearest_bwd_raw(gy, scale):
    gy = O._c(gy)
    N, CB, OH, OW, _ = gy.shape
    gx = torch.empty((N, CB, OH // scale, OW // scale, 8), device=gy.device, dtype=torch.bfloat16)
    L.check(L.load().jvae_upsample_nearest_bwd_b8(L.ptr(gy), L.ptr(gx), N * CB, OH // scale, OW // scale, scale,
                                                  L.stream_ptr()), 'jvae_upsample_nearest_bwd_b8')
    return gx


class _Pool2dB8(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, K, S, P, mode):
        y, idx = pool2d_fwd_raw(x, K, S, P, mode)
        ctx.save_for_backward(idx)
        ctx.cfg = (x.shape[2], x.shape[3], K, S, P, mode)
        return y

    @staticmethod
    def backward(ctx, gy):
        idx, = ctx.saved_tensors
        return pool2d_bwd_raw(gy, idx, *ctx.cfg), None, None, None, None


class _UpsampleNearestB8(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale):
        ctx.scale = scale
        return upsample_nearest_fwd_raw(x, scale)

    @staticmethod
    def backward(ctx, gy):
        return upsample_nearest_bwd_raw(gy, ctx.scale), None


def pool2d(x, kernel_size, stride=None, padding=0, mode=O.POOL_MAX):
    """ops.pool2d on a B8 tensor (same window order / tie rule / fp32 sums, bf16 result)."""
    return _Pool2dB8.apply(x, int(kernel_size), int(stride or kernel_size), int(padding), mode)


def upsample_nearest(x, scale):
    """ops.upsample_nearest on a B8 tensor."""
    if int(scale) != scale or scale < 1:
        raise L.JvaeHipError('nearest up-sampling is built for integer scale factors')
    return _UpsampleNearestB8.apply(x, int(scale))
