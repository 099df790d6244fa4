"""Host-only checks of the convolution kernel selection (csrc/conv_dispatch.hip) through jvae_conv2d_route: every case of
tests/conv_cases.py reaches the kernel it names, the GPU sweep reaches every kernel in every direction it can occur in, a
route never needs more workspace or BatchNorm-sum slots than the public queries hand out, and the public predicates agree
with the route.  Needs the built library, no device."""
import itertools
from ctypes import byref, c_int, c_size_t

import pytest
import torch

import conv_cases as cc
from jvae_hip import lib, ops, ops_b8

DIRS = ('fwd', 'dgrad', 'wgrad')
# the directions a kernel can occur in (csrc/conv_dispatch.hip: fwd_route serves forward and dgrad, wgrad_route the rest).  A
# hand copy of what those two functions can return: a kernel that gains a direction is entered here as well, and the coverage
# test below then asks the sweep for a case of it.
OCCURS = {'CK_GENERIC': DIRS, 'CK_POINT': DIRS, 'CK_SMALLCO': ('fwd',), 'CK_SMALLCI': ('fwd', 'dgrad'),
          'CK_FWD5': ('fwd', 'dgrad'), 'CK_FWD5_X3': ('fwd', 'dgrad'), 'CK_T2': ('fwd', 'dgrad'), 'CK_T2_X3': ('fwd', 'dgrad'),
          'CK_WG5': ('wgrad',), 'CK_WG5_X3': ('wgrad',), 'CK_B8': ('fwd', 'dgrad'), 'CK_T2_B8': ('fwd', 'dgrad'),
          'CK_WG_B8': ('wgrad',), 'CK_WG_B8X': ('wgrad',), 'CK_SMALLCO_DG': ('dgrad',)}


@pytest.fixture(autouse=True)
def _switches():
    L = lib.load()
    old = L.jvae_conv2d_set_split_bf16(1), L.jvae_conv2d_set_split_shape16(1)
    yield
    L.jvae_conv2d_set_split_bf16(old[0])
    L.jvae_conv2d_set_split_shape16(old[1])


def kernel_enum():
    L, names = lib.load(), []
    while L.jvae_conv2d_kernel_name(len(names)) is not None:
        names.append(L.jvae_conv2d_kernel_name(len(names)).decode())
    return names


def test_kernel_names_cover_the_enum():
    names = kernel_enum()
    assert names[0] == 'CK_NONE' and set(names[1:]) == set(OCCURS) and len(set(names)) == len(names)
    L = lib.load()
    assert L.jvae_conv2d_kernel_name(-1) is None and L.jvae_conv2d_kernel_name(len(names)) is None


def test_route_query_refuses_what_the_entry_points_refuse():
    L = lib.load()
    k = c_int(-7)
    q = lambda d, lay, aff, *geom: L.jvae_conv2d_route(d, lay, 0, 0, 0, aff, *geom, byref(k), None, None, None, None)
    good = (2, 32, 16, 16, 64, 5, 5, 1, 2, 0, 0)
    assert q(1, 0, 0, *good) == 0 and L.jvae_conv2d_kernel_name(k.value) == b'CK_FWD5_X3'
    assert q(1, 0, 0, 2, 32, 3, 3, 64, 5, 5, 1, 0, 0, 0) == -1            # no output pixel
    assert q(1, 0, 0, 2, 32, 16, 16, 64, 5, 5, 1, 2, 1, 0) == -1          # output_padding on a plain convolution
    assert q(1, 0, 0, 2, 32, 16, 16, 64, 5, 5, 2, 2, 2, 1) == -1          # output_padding >= stride
    assert q(1, 0, 0, -1, 32, 16, 16, 64, 5, 5, 1, 2, 0, 0) == -1
    assert q(3, 0, 0, *good) == -1 and q(1, 2, 0, *good) == -1 and q(1, 0, 3, *good) == -1
    assert q(1, 0, 0, 0, *good[1:]) == 0                                   # an empty batch is a valid geometry
    with pytest.raises(lib.JvaeHipError):
        ops.conv_route(ops.ConvSpec(32, 64, 5, 1, 0), 2, 3, 3, 'fwd')


def test_every_case_reaches_the_kernel_it_names():
    """Pinned routes: kernel and swap of all three directions of every row, under the row's switch settings."""
    L, wrong = lib.load(), []
    for c in cc.ROWS:
        L.jvae_conv2d_set_split_bf16(c.split)
        L.jvae_conv2d_set_split_shape16(c.sh16)
        for d in DIRS:
            r = c.route(d)
            if (r.kernel, r.swap) != c.expect[d]:
                wrong.append(f'{c.name} [{d}]: expected {c.expect[d][0]} swap={c.expect[d][1]}, routed to {r.kernel} swap={r.swap}')
    assert not wrong, '\n'.join(wrong)


def test_sweep_reaches_every_kernel_in_every_direction():
    """The GPU sweep runs every ConvKernel but CK_NONE, in every direction it can occur in; the kernels with two MFMA shapes
    under both, every fp32 family under both settings of the split-bf16 switch."""
    reached = {}
    for c in cc.SWEEP:
        for d in DIRS:
            reached.setdefault(c.expect[d][0], set()).add(d)
    reached.pop('CK_NONE', None)
    print('reached by the sweep:', {k: sorted(v) for k, v in sorted(reached.items())})
    assert set(reached) == set(kernel_enum()) - {'CK_NONE'}
    assert {k: set(v) for k, v in OCCURS.items()} == reached
    for sh16 in (0, 1):
        assert any(c.sh16 == sh16 and c.expect['fwd'][0] == 'CK_FWD5_X3' and c.expect['dgrad'][0] == 'CK_FWD5_X3' for c in cc.SWEEP)
    assert {c.split for c in cc.SWEEP if c.layout == 'f32'} == {0, 1}
    # a geometry the bf16 layout refuses is part of the sweep too (asserted there as a refusal)
    assert any(c.expect[d][0] == 'CK_NONE' for c in cc.SWEEP for d in DIRS)


def test_real_layer_rows_are_the_layers_the_models_build():
    """The 'arch@size.i' rows carry the geometry of the i-th (transposed) convolution that module.vae_layers builds for that
    architecture: conv32 / conv32- / vgg11 / conv32+ on 3x32x32, conv32+ on 3x64x64 (BASELINE.json configuration 5), and
    their decoders from the latent widths of those configurations (64; 200 at 64x64)."""
    from module.vae_layers.conv import (build_de_conv_layers, find_input_shape, HipConv2d, HipConvTranspose2d, HipPool2d,
                                        HipUpsamplingNearest2d)
    built = {}
    for name, where, size, K in (('conv32', 'input', 32, 0), ('deconv32', 'output', 32, 64), ('conv32+', 'input', 64, 0),
                                 ('deconv32+', 'output', 64, 200), ('conv32-', 'input', 32, 0), ('deconv32-', 'output', 32, 64),
                                 ('vgg11', 'input', 32, 0), ('ivgg', 'output', 32, 64), ('conv32+', 'input', 32, 0),
                                 ('deconv32+', 'output', 32, 64)):
        shape = (3, size, size)
        if where == 'output':
            hw = find_input_shape(name, shape[1:])
            shape = (K // (hw[0] * hw[1]), *hw)
        stack = build_de_conv_layers(shape, name, batch_norm=True, where=where)
        at, i = 0, 0                      # stack.shapes: the input, then one entry per convolution / pooling / up-sampling layer
        for m in stack:
            if isinstance(m, (HipConv2d, HipConvTranspose2d)):
                tr = isinstance(m, HipConvTranspose2d)
                key = f'{name}@{size}.{i}' if where == 'input' else f'{name}@out{size}.{i}'
                built[key] = (m.in_channels, m.out_channels, m.kernel_size[0], m.kernel_size[1], m.stride[0], m.padding[0],
                              m.output_padding[0] if tr else 0, tr, stack.shapes[at][1], stack.shapes[at][2])
                i += 1
            if isinstance(m, (HipConv2d, HipConvTranspose2d, HipPool2d, HipUpsamplingNearest2d)):
                at += 1
    rows = {}
    for c in cc.ROWS:
        if '@' in c.name:
            sp = c.spec
            rows.setdefault(c.name.split(' ')[0], set()).add((sp.cin, sp.cout, sp.k, sp.kw, sp.s, sp.p, sp.op, sp.transposed, c.H, c.W))
    assert set(rows) == set(built)
    for key, geos in rows.items():
        assert geos == {built[key]}, (key, geos, built[key])
    # each at a training batch and at a ragged one, in both layouts
    for key in built:
        have = {(c.N, c.layout) for c in cc.ROWS if c.name.split(' ')[0] == key}
        assert {(512, 'f32'), (37, 'f32'), (256, 'b8'), (37, 'b8')} <= have, key


# ---- workspace and BatchNorm-sum slots: what a route may use against what the queries hand out ------------------------------
CH_IN = (1, 3, 4, 5, 15, 16, 17, 24, 31, 32, 33, 48, 255, 256, 257, 264)
CH_OUT = CH_IN + (8, 9, 40, 200)
KINDS = ((1, 0, 0), (2, 0, 0), (1, 0, 1), (2, 1, 1), (2, 0, 1))                # (stride, output_padding, transposed)


def contract_geometries():
    """(Cin, Cout, H, W, KH, KW, S, P, OP, transposed): on-grid maps with the 5x5 and the 3x3 padding-1 kernels over the full
    channel cross product.  Off-grid widths (12, 24), non-square maps, the 3x5 kernel and the heads take the channel DIAGONAL
    only, not the cross product: every one of those routes is CK_GENERIC or CK_POINT today (ws = 0 for the generic one, which
    chunks by what it is given), so the contract is vacuous there until a kernel claims them - the pinned rows of
    conv_cases.py would then fail first and say so."""
    for cin, cout in itertools.product(CH_IN, CH_OUT):
        for W in (4, 8, 16, 32, 64):
            for (s, op, tr) in KINDS:
                yield (cin, cout, W, W, 5, 5, s, 2, op, tr)
            for (s, op, tr) in ((1, 0, 0), (2, 0, 0), (2, 1, 1)):
                yield (cin, cout, W, W, 3, 3, s, 1, op, tr)
    for cin, cout in zip(CH_IN + CH_IN[:4], CH_OUT):
        for hw in ((12, 12), (24, 24), (16, 32), (32, 16), (9, 13)):
            for (s, op, tr) in KINDS:
                yield (cin, cout, *hw, 5, 5, s, 2, op, tr)
            yield (cin, cout, *hw, 3, 5, 1, 1, 0, 0)
        yield (cin, cout, 8, 8, 7, 7, 1, 0, 0, 0)
        yield (cin, cout, 1, 1, 8, 8, 1, 0, 0, 1)
        yield (cin, cout, 1, 1, 4, 4, 1, 0, 0, 1)


def test_routes_stay_inside_the_queried_workspace_and_splits():
    """For every flag combination and both settings of the split-bf16 switch: route.ws <= jvae_conv2d_workspace_bytes and
    route.splits <= jvae_conv2d_stats_splits of the same geometry; the bf16 routes against the bf16 queries (the weight
    gradient there with the room of its bias gradient's sum, which the entry point adds).  A violation would be an
    out-of-bounds device write, not a wrong number.  A CK_NONE route never occurs in the fp32 layout."""
    L = lib.load()
    route = L.jvae_conv2d_route
    k, ns, ws = c_int(), c_int(), c_size_t()
    rk, rn, rw = byref(k), byref(ns), byref(ws)
    flags = list(itertools.product((0, 1), (0, 1), (0, 1, 2)))
    f32 = [(1, 0, b, st, 0, a) for (b, st, a) in flags] + [(2, 0, 0, 0, 0, 0)] + [(4, 0, 0, 0, 0, a) for a in (0, 1, 2)]
    b8 = [(1, 1, b, st, 0, a) for (b, st, a) in flags] + [(1, 1, b, st, 1, 0) for b in (0, 1) for st in (0, 1)] + \
         [(2, 1, 0, 0, 0, 0)] + [(4, 1, 0, 0, 0, a) for a in (0, 1, 2)]
    bad, calls = [], 0
    for (cin, cout, H, W, kh, kw, s, p, op, tr) in contract_geometries():
        for N in (0, 1, 2, 3, 5, 512):          # empty, one image, around the 2 and 4 images that share a tile, a training batch
            geom = (N, cin, H, W, cout, kh, kw, s, p, op, tr)
            cap_b8, spl_b8 = L.jvae_conv2d_workspace_bytes_b8(*geom), L.jvae_conv2d_stats_splits_b8(*geom)
            for split in (1, 0):
                L.jvae_conv2d_set_split_bf16(split)
                cap, spl = L.jvae_conv2d_workspace_bytes(*geom), L.jvae_conv2d_stats_splits(*geom)
                for (d, lay, b, st, yf, a) in (f32 + b8 if split else f32):          # the bf16 routes do not read the switch
                    assert route(d, lay, b, st, yf, a, *geom, rk, None, rw, rn, None) == 0, geom
                    calls += 1
                    need = ws.value + ((cout + 7) // 8 * 8 * 64 * 4 if (lay == 1 and d == 4 and k.value) else 0)
                    over = d == 1 and ns.value > (spl_b8 if lay else spl)          # only a forward writes BatchNorm sums
                    if need > (cap_b8 if lay else cap) or over or (lay == 0 and k.value == 0):
                        bad.append((geom, split, (d, lay, b, st, yf, a), L.jvae_conv2d_kernel_name(k.value).decode(),
                                    need, cap_b8 if lay else cap, ns.value, spl_b8 if lay else spl))
    print(calls, 'route queries')
    assert not bad, (len(bad), bad[:10])


def test_public_predicates_agree_with_the_route():
    """jvae_conv2d_affine_ok(_b8) is 1 exactly when the forward and the weight-gradient routes both apply the input affine;
    ops_b8.native_mask has a direction's bit exactly when that direction's bf16 route is a kernel."""
    L, bad = lib.load(), []
    rows = {(c.spec.geom(c.N, c.H, c.W)): c for c in cc.ROWS}
    geoms = list(rows) + [(3, cin, H, W, cout, kh, kw, s, p, op, tr)
                          for (cin, cout, H, W, kh, kw, s, p, op, tr) in itertools.islice(contract_geometries(), 0, None, 7)]
    for geom in geoms:
        N, cin, H, W, cout, kh, kw, s, p, op, tr = geom
        sp = cc.Spec(cin, cout, (kh, kw), s, p, op, bool(tr))
        for split in (1, 0):
            L.jvae_conv2d_set_split_bf16(split)
            for lay, query in (('f32', L.jvae_conv2d_affine_ok), ('b8', L.jvae_conv2d_affine_ok_b8)):
                both = all(ops.conv_route(sp, N, H, W, d, lay, aff=1).aff_ok for d in ('fwd', 'wgrad'))
                if query(*geom) != int(both):
                    bad.append(('affine_ok', lay, geom, split, query(*geom), both))
            mask = L.jvae_conv2d_native_b8(*geom)
            for d in DIRS:
                if bool(mask & ops.ROUTE_DIR[d]) != (ops.conv_route(sp, N, H, W, d, 'b8').kernel != 'CK_NONE'):
                    bad.append(('native_b8', geom, d, mask))
                if ops.conv_route(sp, N, H, W, d, 'f32').kernel == 'CK_NONE':
                    bad.append(('CK_NONE in fp32', geom, d))
    assert not bad, (len(bad), bad[:10])
    c = cc.CASES['conv32+@64.2 N3 b8']
    assert ops_b8.native_mask(c.spec, c.N, c.H, c.W) == 7 and ops_b8.native_mask(ops.ConvSpec(64, 200, 7, 1, 0), 3, 8, 8) == 0


def test_per_plane_measure_sees_what_the_global_one_misses():
    """The fp64 forward of a wide-dynamic-range case with only the last output row of its lowest-scale image off by a relative
    1e-3 (a halo row of the ragged image of a shared tile): the global measure of the older tests stays under the tightest bar
    (3e-6), the per-plane measure and the elementwise bound flag it."""
    c = cc.Case('measure', 1, 32, 5, 1, 2, 0, 0, 8, 37, 'FWD5 FWD5_X3~ WG5_X3~', bias=0)     # one input channel, no bias: ONE scale per image
    d = cc.make_data(c)
    ref, A, K = cc.references(c, d)
    y = ref['fwd'].clone()
    n = c.N - 1                                           # the recipe puts the smallest-scale image last: the ragged one of its tile
    assert float(d['x'][n].abs().max()) < 1e-3 * float(d['x'].abs().max())
    y[n, :, -1, :] *= 1 + 1e-3
    assert cc.global_rel(y, ref['fwd']) < 3e-6
    worst, where = cc.worst_plane(y, ref['fwd'], A['fwd'])
    assert worst > 3e-5 and where[0] == n, (worst, where)
    assert cc.elementwise_excess(y, ref['fwd'], A['fwd'], K['fwd']) > 1
    # and neither measure objects to the reference rounded to fp32
    y32 = ref['fwd'].float()
    assert cc.worst_plane(y32, ref['fwd'], A['fwd'])[0] < 1e-7 and cc.elementwise_excess(y32, ref['fwd'], A['fwd'], K['fwd']) < 1
