"""Host-only checks of the dense-product plan (gemm_plan() in csrc/gemm.hip) through jvae_gemm_route: every case of
tests/gemm_cases.py reaches the variant it names with the K slices it names, the table reaches all 16 variants and every edge
class the GPU sweep is meant to run, the K slices tile [0, K) exactly, and the inputs of the exact probe have the properties that
make equality the right assertion there.  Needs the built library, no device."""
import ctypes
import itertools

import numpy as np
import pytest

import gemm_cases as gc
from jvae_hip import lib, ops


@pytest.fixture(autouse=True)
def _switch():
    L = lib.load()
    old = L.jvae_conv2d_set_split_bf16(1)
    yield
    L.jvae_conv2d_set_split_bf16(old)


def test_variant_names_cover_the_sixteen():
    L = lib.load()
    names = [L.jvae_gemm_variant_name(v) for v in range(16)]
    assert [n.decode() for n in names] == gc.VARIANTS and len(set(names)) == 16
    assert L.jvae_gemm_variant_name(-1) is None and L.jvae_gemm_variant_name(16) is None


def test_every_case_reaches_the_variant_it_names():
    L, wrong = lib.load(), []
    for c in gc.ROWS:
        L.jvae_conv2d_set_split_bf16(c.split)
        r = c.route()
        if (r.variant, r.slices) != (c.expect, c.slices):
            wrong.append(f'{c.name}: expected {c.expect} in {c.slices} slices, routed to {r.variant} in {r.slices}')
        assert r.grid[2] == c.batch * r.slices, c.name
        assert r.kchunk % 32 == 0 and (r.slices - 1) * r.kchunk < max(c.K, 1) <= max(r.slices * r.kchunk, 1), c.name
    assert not wrong, '\n'.join(wrong)


def test_table_reaches_every_variant_and_every_edge_class():
    """Asserted, not printed: the 16 variant names, every tag of gemm_cases.TAGS, and - the GPU sweep runs ALL rows - both settings
    of the switch, both slicing forms, and a DEPTH 1 and a DEPTH 3 variant of every layout with and without atomic slices."""
    assert {c.expect for c in gc.ROWS} == set(gc.VARIANTS)
    have = {t for c in gc.ROWS for t in c.tags}
    assert have == set(gc.TAGS), (have ^ set(gc.TAGS))
    assert all(c.tags for c in gc.ROWS)
    assert {c.split for c in gc.ROWS} == {0, 1}
    assert any(c.want for c in gc.ROWS) and any(c.atomic and c.slices > 2 for c in gc.ROWS)
    for tag, n in (('deep_steps', 20), ('deep_partial', 8), ('deep_short_slice', 4), ('tile128', 4), ('switch_off', 4)):
        assert sum(tag in c.tags for c in gc.ROWS) == n, tag
    for c in gc.ROWS:          # sizes: nothing beyond about 2 M output elements
        assert c.batch * c.M * c.N * (c.slices if c.want else 1) <= 2.2e6, c.name
    # the K of the pipeline rows, and the stated neighbours
    assert {c.K for c in gc.ROWS if 'deep_steps' in c.tags} == {64, 96, 128, 160, 224}
    assert {c.K for c in gc.ROWS if 'deep_partial' in c.tags} == {68, 100}
    assert {(c.K, c.expect[:2]) for c in gc.ROWS if 'x3_boundary' in c.tags} == {(63, 'TI'), (64, 'X3')}
    assert {(c.M, c.N) for c in gc.ROWS if 'ragged' in c.tags} >= {(1, 129), (63, 65), (64, 64), (65, 63), (129, 1)}
    assert {c.expect for c in gc.ROWS if c.tags[0].startswith('nodeep')} <= {v for v in gc.VARIANTS if v.endswith('D1')}


def test_no_gpu_case_is_skipped():
    """The GPU sweep is parametrised over ALL rows of the table, in order, and its file has no skip or expected failure."""
    import inspect

    import test_24_gemm_sweep_gpu as T
    (mark,) = [m for m in T.test_sweep_against_fp64.pytestmark if m.name == 'parametrize']
    assert list(mark.args[1]) == [c.name for c in gc.ROWS]
    src = inspect.getsource(T)
    assert 'skip' not in src and 'xfail' not in src and 'importorskip' not in src
    # the probes: every layout, both depths, both roles, with and without slices; every tile variant in the one-hot probe
    marks = {m.args[0]: list(m.args[1]) for m in T.test_six_products_exactly.pytestmark if m.name == 'parametrize'}
    assert marks == {'lay': list(gc.LAYOUTS), 'depth': [1, 3], 'sparse': ['A', 'B'], 'splitk': [1, 2, 4]}
    (mark,) = [m for m in T.test_single_products_of_the_fp32_kernel.pytestmark if m.name == 'parametrize']
    assert {T._onehot_case(lay, big, sk).expect for lay, big, _, sk in mark.args[1]} == set(gc.VARIANTS[:8])
    for lay, depth, sk in itertools.product(gc.LAYOUTS, (1, 3), (1, 2, 4)):
        c = T._probe_case(lay, depth, sk)
        r = c.route()
        assert (r.variant, r.slices) == (c.expect, c.slices) and 2 * min(c.M, c.N) >= c.K, c.name


def test_tile_counts_of_the_xcd_rows():
    grids = {c.name: c.route().grid for c in gc.ROWS if 'xcd' in c.tags}
    counts = sorted(g[0] * g[1] * g[2] for g in grids.values())
    assert counts == [2, 6, 9, 13, 16], grids
    assert any(g[2] > 1 for g in grids.values())


def test_route_reports_the_plan_fields():
    c = gc.CASES['slices ragged K160 splitk4 x3']
    r = c.route()
    assert r == ops.GemmRoute('X3_AK_BK_D3', (2, 2, 3), 3, 64, True, True, r.lds) and 0 < r.lds <= 64 * 1024
    r = gc.CASES['nodeep A base+1 nn'].route()
    assert (r.vecA, r.vecB) == (False, True)
    r = gc.CASES['tile128 b128 nn'].route()
    assert r.grid == (2, 2, 128) and r.lds == 32 * (132 + 132) * 4
    r = gc.CASES['K0 bias'].route()
    assert (r.variant, r.slices, r.kchunk, r.grid) == ('TILE64_AK_BN', 1, 0, (1, 2, 1))


def test_lds_bytes_of_every_variant():
    """GemmRoute.lds per variant name, one row of the table each: the fp32 images BK * ((BM + 4) + (BN + 4)) * 4 of the tile
    kernels and three bf16 planes per operand of the split-bf16 kernels - 64 rows of 80 bytes for an operand contiguous along k,
    32 k of 192 bytes otherwise.  The figures are written out: they are what the kernels took before the variant table."""
    want = {'TILE64': 17408, 'TILE128': 33792, 'X3_AM_BK': 33792, 'X3_AM_BN': 36864, 'X3_AK_BK': 30720, 'X3_AK_BN': 33792}
    assert want['TILE64'] == 32 * 2 * 68 * 4 and want['TILE128'] == 32 * 2 * 132 * 4
    kc, kr = 3 * 64 * 80, 3 * 32 * 192
    assert [want['X3_' + n] for n in ('AM_BK', 'AM_BN', 'AK_BK', 'AK_BN')] == [kr + kc, kr + kr, kc + kc, kc + kr]
    L, seen = lib.load(), {}
    for c in gc.ROWS:
        if c.expect not in seen:
            L.jvae_conv2d_set_split_bf16(c.split)
            r = c.route()
            assert r.variant == c.expect, c.name
            seen[c.expect] = r.lds
    assert set(seen) == set(gc.VARIANTS)
    for name, lds in seen.items():
        key = name.split('_')[0] if name.startswith('TILE') else name[:-3]
        assert lds == want[key], (name, lds)


def test_route_return_codes_are_those_of_the_launch_entries():
    L = lib.load()
    base = dict(A=0x1000, sA=(8, 1, 0), B=0x2000, sB=(8, 1, 0), C=0x3000, sC=(8, 1, 0))
    for empty in (dict(M=0, N=8, K=8), dict(M=8, N=0, K=8), dict(M=8, N=8, K=8, batch=0)):
        r = ops.gemm_route(**{**base, **empty})
        assert r.variant is None and r.grid == (0, 0, 0) and r.slices == 0
    bad = [dict(M=8, N=8, K=-1), dict(M=8, N=8, K=8, A=None), dict(M=8, N=8, K=8, C=None), dict(M=8, N=8, K=8, bias_mode=1),
           dict(M=8, N=8, K=128, flags=2, splitk=2), dict(M=8, N=8, K=0, want_splits=2)]
    for kw in bad:
        with pytest.raises(lib.JvaeHipError):
            ops.gemm_route(**{**base, **kw})
    d, r = lib.GemmDesc(), lib.GemmRoute()
    assert L.jvae_gemm_route(None, ctypes.byref(r)) == -1 and L.jvae_gemm_route(ctypes.byref(d), None) == -1
    d.M = d.N = d.batch = 8
    d.K, d.A, d.B, d.C, d.sAm, d.sAk, d.sBk, d.sBn, d.sCm, d.sCn = 128, 0x1000, 0x2000, 0x3000, 128, 1, 8, 1, 8, 1
    d.want_splits = 2          # the stored form has to report its count, as in jvae_gemm_group_f32
    assert L.jvae_gemm_route(ctypes.byref(d), ctypes.byref(r)) == -1 and r.variant == -1


def test_slices_tile_k_exactly():
    """Over a grid of (M, N, K, splitk), both switch settings and both slicing forms: kchunk is a multiple of 32,
    (slices - 1) * kchunk < K <= slices * kchunk, never more slices than asked for, grid z = batch * slices."""
    L, n = lib.load(), 0
    for split in (1, 0):
        L.jvae_conv2d_set_split_bf16(split)
        for M, N, K, sk, want in itertools.product((1, 64, 65, 130), (1, 63, 200), (1, 31, 32, 33, 63, 64, 65, 96, 160, 200, 800, 7200),
                                                   (1, 2, 3, 4, 7, 16, 1000), (False, True)):
            for batch in (1, 3):
                r = ops.gemm_route(M, N, K, 0x1000, (K, 1, M * K), 0x2000, (N, 1, K * N), 0x3000, (N, 1, M * N), batch=batch,
                                   splitk=1 if want else sk, want_splits=sk if want else 0, sCsplit=batch * M * N)
                assert r.kchunk > 0 and r.kchunk % 32 == 0, (M, N, K, sk, r)
                assert (r.slices - 1) * r.kchunk < K <= r.slices * r.kchunk and 1 <= r.slices <= sk, (M, N, K, sk, r)
                assert r.grid[2] == batch * r.slices
                tile = 128 if r.variant.startswith('TILE128') else 64
                assert r.grid[:2] == ((N + tile - 1) // tile, (M + tile - 1) // tile)
                n += 1
    print(n, 'route queries')


# ---- the probes' inputs
@pytest.mark.parametrize('sparse', ['A', 'B'])
@pytest.mark.parametrize('K', [70, 160])
def test_exact_probe_inputs_make_equality_the_right_assertion(sparse, K):
    """For the probe's operands: the RNE split returns exactly the three digits as planes; the six-term sum and every partial
    sum of it are representable in fp32 (probe_expected asserts it); the sum differs from the correctly rounded full product
    in a good share of the elements (the three dropped products are seen to be dropped); dropping any one kept product, or
    doubling x1 w3 in place of x3 w1, changes most elements."""
    A, B = gc.probe_operands(132, 132, K, sparse, seed=K)
    for X in (A, B):
        h, m, l = gc.x3_split(X)
        nz = X != 0
        assert np.all(h + m + l == X.astype(np.float64))
        assert np.all(np.isin(np.abs(h[nz]), (1.0, 2.0)))
        assert np.all(np.isin(np.abs(m[nz]), (gc.EPS, 2 * gc.EPS))) and np.all(np.isin(np.abs(l[nz]), (gc.EPS ** 2, 2 * gc.EPS ** 2)))
    sp = A if sparse == 'A' else B.T
    assert np.all((sp != 0).sum(1) == 2) and np.all((sp != 0).any(0))
    y = gc.probe_expected(A, B)
    assert np.abs(y).max() <= 8.02
    full = A.astype(np.float64) @ B.astype(np.float64)
    assert np.mean(full.astype(np.float32) != y.astype(np.float32)) > 0.05
    for drop in gc.KEPT:
        assert np.mean(gc.six_products(A, B, [k for k in gc.KEPT if k != drop]) != y) > 0.7, drop
    dup = [(0, 2) if k == (2, 0) else k for k in gc.KEPT]
    assert np.mean(gc.six_products(A, B, dup) != y) > 0.7
    # what the global measure of the older tests makes of a dropped third-order product on the same operands: nothing
    lost = gc.six_products(A, B, gc.KEPT[1:])
    assert np.abs(lost - y).max() / np.abs(y).max() < 2e-5


def test_onehot_inputs_meet_every_k():
    for hot in ('A', 'B'):
        A, B = gc.onehot_operands(130, 130, 40, hot, seed=3)
        X = A if hot == 'A' else B.t()
        assert bool(((X != 0).sum(1) == 1).all()) and bool((X != 0).any(0).all())


def test_placement_leaves_nan_everywhere_else():
    import torch
    c = gc.CASES['conv generic head dgrad']
    d = gc.make_data(c)
    buf, idx = gc.place(d['A'], (c.sA[2], c.sA[0], c.sA[1]), c.offA)
    assert buf.numel() == int(idx.max()) + 1 + gc.TAIL and bool(torch.isnan(buf[:c.offA]).all()) and bool(torch.isnan(buf[-gc.TAIL:]).all())
    assert int((~torch.isnan(buf)).sum()) == d['A'].numel() and torch.equal(buf[idx], d['A'])
    ref, mag, ks = gc.reference(c, d, 96)
    assert ref.shape == (c.batch, 1, c.M, c.N) and ks == [c.K] and bool((mag >= ref.abs()).all())
