"""Host-only half of the BatchNorm sweep (tests/bn_cases.py): every row reaches the launch plan it claims, an fp32 emulation of
the kernels' summation order (numpy: per thread sequential, butterfly per wave, the four wave sums, parts from jvae_image_range,
fp64 fold) stays inside the sums bounds - so the fp64 reference alone satisfies them - and the mutants of that emulation which
the GPU sweep is there to catch breach them."""
import ctypes

import numpy as np
import pytest
import torch

import bn_cases as bc
from jvae_hip import lib

KINDS = ('d', 'd2', 'g', 'gx')
ALL = bc.ROWS + bc.MASK_ROWS
ids = lambda c: c.name.replace(' ', '_')


def plan_of(case):
    L = lib.load()
    ns, nc = ctypes.c_int(), ctypes.c_int()
    rc = (L.jvae_bn_plan_b8 if case.b8 else L.jvae_bn_plan)(case.N, case.C, case.P, ns, nc)
    assert rc == 0
    return ns.value, nc.value


def ranges(N, parts):
    L = lib.load()
    nb, ne = ctypes.c_int(), ctypes.c_int()
    out = []
    for j in range(parts):
        assert L.jvae_image_range(N, parts, j, nb, ne) == 0
        assert (nb.value, ne.value) == bc.image_range(N, parts, j)          # the mirror the references use
        out.append((nb.value, ne.value))
    return out


def index_path(case):
    """The predicate of bn_plane_walk / plane4_idx (fp32) and unit_idx (bf16)."""
    if case.b8:
        return 'shift' if case.P & (case.P - 1) == 0 else 'div'
    if case.P % 4:
        return 'scalar'
    p4 = case.P // 4
    return 'shift' if p4 & (p4 - 1) == 0 else 'div'


def features(case):
    """What of a row's plan shapes its SUMS (the apply stages are checked element by element, where every row is sharp)."""
    ns, _, es, _, path = case.plan
    per = -(-case.N // ns)
    f = {f'{case.layout} {case.mode} walk', f'{case.layout} {path} path'}
    if ns > 1:
        f.add(f'{case.layout} several parts')
        f.add(f'{case.layout} {path} path across parts')
    if ns > 1 and case.N % per:
        f.add(f'{case.layout} ragged last part')
    if es:
        f.add(f'{case.layout} empty parts')
    if case.b8 and case.C % 8:
        f.add('b8 padding channels')
    if ns == bc.MAX_SPLIT[case.layout]:
        f.add(f'{case.layout} MAX_SPLIT')
    return f


def fine(case):
    """One element of average size is more than four bounds: n (D + c) U < 1 / 4 with the largest c of the four sums."""
    return case.N * case.P * (bc.depth(case) + max(bc.C_SUM.values())) * bc.U < 0.25


@pytest.mark.parametrize('case', ALL, ids=ids)
def test_row_reaches_its_plan(case):
    ns, nc = plan_of(case)
    empty = lambda parts: sum(1 for nb, ne in ranges(case.N, parts) if nb == ne)
    assert (ns, nc, empty(ns), empty(nc), index_path(case)) == case.plan, case.name
    for parts in (ns, nc):
        r = [x for x in ranges(case.N, parts) if x[0] < x[1]]
        assert r[0][0] == 0 and r[-1][1] == case.N and all(a[1] == b[0] for a, b in zip(r, r[1:]))


def test_fine_rows_cover_every_plan_feature_but_the_caps():
    """The two MAX_SPLIT rows need n >= 2^19 elements per channel, where one element is below the resolution of an fp32 sum."""
    every = set().union(*(features(c) for c in bc.ROWS))
    caps = {'f32 MAX_SPLIT', 'b8 MAX_SPLIT'}
    assert caps <= every
    covered = set().union(*(features(c) for c in bc.ROWS if fine(c)))
    assert every - caps <= covered, sorted(every - caps - covered)
    assert not any(fine(c) for c in bc.ROWS if features(c) & caps)


# ---------------------------------------------------------------------------------------------- the emulation
def terms(case, d):
    """Rank 0 of a row: the fp32 terms as the kernels form them, (N, 4, C, P), and the exact ones in fp64 (KINDS order)."""
    N, Cn = case.N, case.C
    f = np.float32
    x, dy, p = d['x'][:N].numpy(), d['dy'][:N].numpy(), d['pivot'].numpy().reshape(1, Cn, 1)
    gam = (d['gamma'].numpy() if case.affine else np.ones(Cn, f)).reshape(1, Cn, 1)
    bet = (d['beta'].numpy() if case.affine else np.zeros(Cn, f)).reshape(1, Cn, 1)
    x64, dy64 = x.astype(np.float64), dy.astype(np.float64)
    mean64 = x64.mean((0, 2), keepdims=True)
    var64 = ((x64 - mean64) ** 2).mean((0, 2), keepdims=True)
    mu, inv = mean64.astype(f), (1. / np.sqrt(var64 + bc.EPS)).astype(f)
    sc = gam * inv                                                                   # bn_coef: fl(g * invstd)
    sh = (bet.astype(np.float64) - mu.astype(np.float64) * sc).astype(f)            # ... and fma(-mean, scale, beta)
    mask = x64 * sc + sh > 0                                                         # the sign of fmaf(x, scale, shift), exactly
    neg = f(bc.SLOPE) if case.act == 2 else f(0)
    dd = x - p
    g = dy if case.act == 0 else np.where(mask, dy, dy * neg)
    xh = (x - mu) * inv
    t32 = np.stack([dd, dd * dd, g, g * xh], 1)
    assert t32.dtype == np.float32
    d64 = x64 - p
    g64 = dy64 if case.act == 0 else np.where(mask, dy64, dy64 * float(neg))
    xh64 = (x64 - mu) * inv.astype(np.float64)
    t64 = np.stack([d64, d64 * d64, g64, g64 * xh64], 1)
    return t32, t64


def walk_sum(t, mode):
    """One 256-thread block on the flat terms t (rows, L) of its image part, in fp32: per thread sequential in ascending order,
    the xor butterfly of each wave, then the four wave sums as block_sum / block_sum8 add them."""
    rows, Ln = t.shape
    w = 4 if mode == 'vec4' else 1
    steps = -(-Ln // (256 * w))
    pad = np.zeros((rows, steps * 256 * w), np.float32)
    pad[:, :Ln] = t
    a = pad.reshape(rows, steps, 256, w)
    acc = np.zeros((rows, 256), np.float32)
    for k in range(steps):
        for e in range(w):
            acc = acc + a[:, k, :, e]
    v = acc.reshape(rows, 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o]
    r = v[:, :, 0]
    assert r.dtype == np.float32
    return (r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3]) if mode == 'b8' else (r[:, 0] + r[:, 2]) + (r[:, 1] + r[:, 3])


def emulate(case, t32, parts):
    """-> (4, C) fp32 sums: a block per image part, the parts folded in fp64 and rounded once."""
    N, K, Cn, P = t32.shape
    total = np.zeros(K * Cn, np.float64)
    for nb, ne in parts:
        if ne > nb:
            flat = t32[nb:ne].transpose(1, 2, 0, 3).reshape(K * Cn, (ne - nb) * P)
            total += walk_sum(flat, case.mode).astype(np.float64)
    return total.astype(np.float32).reshape(K, Cn)


def excess(case, sums, t64):
    """-> {kind: per-channel excess over the sums bound} against the fp64 sums of the exact terms."""
    D = bc.depth(case)
    ref, A = t64.sum((0, 3)), np.abs(t64).sum((0, 3))
    return {k: bc.channel_excess(sums[i].astype(np.float64), ref[i], A[i], D, bc.C_SUM[k]) for i, k in enumerate(KINDS)}, A


_memo = {}


def honest(case):
    if case.name not in _memo:
        _memo.clear()                    # one row at a time: the largest holds 40 MB of terms
        t32, t64 = terms(case, bc.make_data(case))
        parts = ranges(case.N, plan_of(case)[0])
        _memo[case.name] = (t32, t64, parts)
    return _memo[case.name]


@pytest.mark.parametrize('case', ALL, ids=ids)
def test_emulated_sums_are_inside_the_bounds(case):
    t32, t64, parts = honest(case)
    ex, _ = excess(case, emulate(case, t32, parts), t64)
    worst = {k: float(v.max()) for k, v in ex.items()}
    print(f'{case.name}: D = {bc.depth(case)}, emulated sums at {worst} of their bounds')
    assert all(v <= 1 for v in worst.values()), (case.name, worst)


def breaches(case, t32, t64, parts, kinds=KINDS):
    """Every sum of `kinds` that has anything to sum leaves its bound in at least one channel."""
    ex, A = excess(case, emulate(case, t32, parts), t64)
    worst = {k: float(ex[k].max()) for k in kinds if A[KINDS.index(k)].max() > 0}
    assert worst and all(v > 1 for v in worst.values()), (case.name, worst)
    return worst


@pytest.mark.parametrize('case', bc.ROWS, ids=ids)
def test_mutants_of_the_emulation_breach_the_bounds(case):
    """Dropped last image of the last non-empty part; a part boundary one image late (the image is summed twice); the P % 4
    tail of one image dropped; bf16 padding lanes read as the last channel's data (zeros against its pivot)."""
    t32, t64, parts = honest(case)
    last = max(j for j, (nb, ne) in enumerate(parts) if ne > nb)
    seen = {}
    m = list(parts)
    m[last] = (m[last][0], m[last][1] - 1)
    seen['last image'] = breaches(case, t32, t64, m)
    if last > 0:
        m = list(parts)
        m[0] = (m[0][0], m[0][1] + 1)
        seen['boundary'] = breaches(case, t32, t64, m)
    if not case.b8 and case.P % 4:
        t = t32.copy()
        t[case.N - 1, :, :, case.P - case.P % 4:] = 0
        seen['tail'] = breaches(case, t, t64, parts)
    if case.b8 and case.C % 8:
        t = t32.copy()
        p = np.float32(bc.make_data(case)['pivot'][-1])
        t[:, 0, -1], t[:, 1, -1], t[:, 2, -1], t[:, 3, -1] = -p, p * p, 0, 0
        seen['padding'] = breaches(case, t, t64, parts, ('d', 'g'))
    print(f'{case.name}: {seen}')


@pytest.mark.parametrize('case', [c for c in bc.ROWS if fine(c)], ids=ids)
def test_one_dropped_element_breaches_the_bounds_of_a_fine_row(case):
    """In every channel and every sum: the last element of at least half the average magnitude is dropped.  Its term is then
    >= A / (2 n) > 2 bounds (fine: bound < A / (4 n)), and the honest sum is inside one."""
    t32, t64, parts = honest(case)
    t = t32.copy()
    N, K, Cn, P = t64.shape
    mag = np.abs(t64).transpose(1, 2, 0, 3).reshape(K, Cn, N * P)
    big = mag >= 0.5 * mag.mean(2, keepdims=True)
    idx = N * P - 1 - np.argmax(big[:, :, ::-1], 2)
    for k in range(K):
        for c in range(Cn):
            t[idx[k, c] // P, k, c, idx[k, c] % P] = 0
    ex, A = excess(case, emulate(case, t, parts), t64)
    for i, k in enumerate(KINDS):
        live = torch.as_tensor(A[i] > 0)
        assert bool((ex[k][live] > 1).all()), (case.name, k, ex[k])
