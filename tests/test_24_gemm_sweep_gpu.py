"""GPU: every variant of the dense products (csrc/gemm.hip) against fp64, on the case table of tests/gemm_cases.py.

Each test asserts the route first (jvae_gemm_route with the device addresses of the run), so no case passes on another kernel.
Three measures:
  * dense wide-range data against the fp64 product, every element on its own scale: |y - ref| <= (K + c) U A with A = |A| |B| +
    |bias| (+ |C0|) and the derived c of gemm_cases.bound_c - printed per case, asserted <= 1; two launches give the same bits
    (atomic sums of more than two addends excepted - three slices, or two onto a C that holds values: their order is the hardware's);
  * canaries: A, B and C live inside larger NaN buffers (in front, between rows / batches / slices, behind).  A NaN that is read
    as an operand reaches the result; the elements of the C buffer outside C must come back bit for bit;
  * exact probes: operands built so that the split-bf16 kernel's six-product sum (the fp32 kernel's single product) is exactly
    representable at every partial sum - the result must EQUAL the expected bits (test_gemm_routes.py checks the inputs' properties).
The fold of stored slices (jvae_splitk_fold_f32 and its grouped form) is checked against fp64 and against the same fp32 additions
in the same order."""
import ctypes

import numpy as np
import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(autouse=True)
def _switch():
    from jvae_hip import lib
    L = lib.load()
    old = L.jvae_conv2d_set_split_bf16(1)
    yield
    L.jvae_conv2d_set_split_bf16(old)


def _launch(c, A, B, Cv, bias):
    """One launch of the case on operand views that begin at the operands' first elements.  Returns the slices reported (want)."""
    from jvae_hip import lib as L, ops
    if not c.want:
        ops.gemm(c.M, c.N, c.K, A, c.sA, B, c.sB, Cv, c.sC, bias=bias, bias_mode=c.bias, flags=c.flags, splitk=c.splitk, batch=c.batch)
        return None
    arr, made = (L.GemmDesc * 1)(), ctypes.c_int(-1)
    d = arr[0]
    d.M, d.N, d.K, d.batch = c.M, c.N, c.K, c.batch
    d.A, (d.sAm, d.sAk, d.sAb) = A.data_ptr(), c.sA
    d.B, (d.sBk, d.sBn, d.sBb) = B.data_ptr(), c.sB
    d.C, (d.sCm, d.sCn, d.sCb) = Cv.data_ptr(), c.sC
    d.bias, d.bias_mode, d.flags, d.splitk = None, 0, 0, 1
    d.want_splits, d.sCsplit, d.splits = c.want, c.sCsplit, ctypes.pointer(made)
    L.check(L.load().jvae_gemm_group_f32(arr, 1, L.stream_ptr()), 'jvae_gemm_group_f32')
    return made.value


def _sync():
    if DEV == 'cuda':
        torch.cuda.synchronize()


def _bits(t):
    return t.contiguous().view(torch.int32)


def run_case(c, d):
    """Route, launch twice, canaries.  d: A (ba, M, K), B (bb, K, N), bias, C0 (batch, M, N) on the CPU.  Returns the result as
    (batch, S, M, N) of both launches on the CPU and the route."""
    from jvae_hip import lib
    lib.load().jvae_conv2d_set_split_bf16(c.split)
    hA, _ = gc.place(d['A'], (c.sA[2], c.sA[0], c.sA[1]), c.offA)
    hB, _ = gc.place(d['B'], (c.sB[2], c.sB[0], c.sB[1]), c.offB)
    S = c.slices if c.want else 1
    base = d['C0'].unsqueeze(1) if c.onto else torch.full((c.batch, S, c.M, c.N), float('nan'))
    hC, idxC = gc.place(base.contiguous(), (c.sC[2], c.sCsplit, c.sC[0], c.sC[1]), c.offC)
    bA, bB = hA.to(DEV), hB.to(DEV)
    bias = d['bias'].to(DEV) if c.bias else None
    outs = [hC.to(DEV, copy=True), hC.to(DEV, copy=True)]
    for t in (bA, bB, *outs):
        assert t.data_ptr() % 16 == 0
    r = c.route(A=bA.data_ptr(), B=bB.data_ptr(), C=outs[0].data_ptr(), bias=bias.data_ptr() if c.bias else 0)
    assert (r.variant, r.slices) == (c.expect, c.slices), (c.name, r)          # the kernel under test is the one named
    for out in outs:
        made = _launch(c, bA[c.offA:], bB[c.offB:], out[c.offC:], bias)
        assert made is None or made == c.slices, (c.name, made)
    _sync()
    o0, o1 = (o.cpu() for o in outs)
    if c.ordered:
        assert torch.equal(_bits(o0), _bits(o1)), f'{c.name}: two launches differ'
    for o in (o0, o1):
        outside = torch.ones(o.numel(), dtype=torch.bool)
        outside[idxC.reshape(-1)] = False
        assert torch.equal(_bits(o)[outside], _bits(hC)[outside]), f'{c.name}: written outside C'
        assert not bool(torch.isnan(o[idxC]).any()), f'{c.name}: NaN inside C (an element not written, or padding read as an operand)'
    return o0[idxC], o1[idxC], r


# ---- a. dense wide-range data against fp64 on every row of the table, b. with the canaries of run_case
@pytest.mark.parametrize('name', [c.name for c in gc.ROWS])
def test_sweep_against_fp64(name):
    c = gc.CASES[name]
    d = gc.make_data(c)
    y0, y1, r = run_case(c, d)
    ref, mag, ks = gc.reference(c, d, r.kchunk)
    worst = 0.0
    for y in (y0, y1):
        for s, K in enumerate(ks):
            worst = max(worst, gc.elementwise_excess(y[:, s], ref[:, s], mag[:, s], K, c=gc.bound_c(c)))
    print(f'{name}: {r.variant} grid {r.grid} slices {r.slices}: excess of (K + {gc.bound_c(c)}) U A = {worst:.3f}')
    assert worst <= 1.0, (name, worst)


# ---- c. the exact probe of the six products: every layout, DEPTH 1 and 3, both operand roles, with and without K slices
def _probe_case(lay, depth, splitk):
    K = 160 if depth == 3 else 70          # 70: K % 4 != 0 withdraws the deep form; leading strides along k padded to 72
    ld = lambda contiguous_k, other: (72 if K == 70 else K) if contiguous_k else other
    slices = {(160, 1): 1, (160, 2): 2, (160, 4): 3, (70, 1): 1, (70, 2): 2, (70, 4): 3}[K, splitk]
    return gc.Case(f'probe {lay} D{depth} splitk{splitk}', 132, 132, K, lay, lda=ld(lay[0] == 'n', 132), ldb=ld(lay[1] == 't', 132),
                   splitk=splitk, slices=slices, expect=gc.vname('X3', lay, depth))


@pytest.mark.parametrize('splitk', [1, 2, 4])
@pytest.mark.parametrize('sparse', ['A', 'B'])
@pytest.mark.parametrize('depth', [1, 3])
@pytest.mark.parametrize('lay', gc.LAYOUTS)
def test_six_products_exactly(lay, depth, sparse, splitk):
    c = _probe_case(lay, depth, splitk)
    A, B = gc.probe_operands(c.M, c.N, c.K, sparse, seed=c.K + (sparse == 'B'))
    want = torch.from_numpy(gc.probe_expected(A, B)).float()
    d = dict(A=torch.from_numpy(A)[None], B=torch.from_numpy(B)[None], bias=None, C0=torch.zeros(1, c.M, c.N))
    y0, y1, _ = run_case(c, d)
    for y in (y0, y1):
        wrong = int((y[0, 0] != want).sum())
        assert torch.equal(y[0, 0], want), f'{c.name}: {wrong} of {want.numel()} elements are not the six-product sum'


# ---- d. the one-hot probe of the fp32 tile variants: every output is ONE product - the fp64 product rounded to fp32
ONEHOT_ULP_CAP = 0          # measured on the MI355X (profiles/NOTES.md): the matrix core's single product is correctly rounded


def _onehot_case(lay, big, splitk):
    return gc.Case(f'onehot {lay} {"128" if big else "64"} splitk{splitk}', 130, 130, 40, lay, batch=128 if big else 1, sAb=0, sBb=0,
                   splitk=splitk, slices=splitk, expect=gc.vname('TILE128' if big else 'TILE64', lay))


@pytest.mark.parametrize('lay,big,hot,splitk',
                         [(lay, False, hot, sk) for lay in gc.LAYOUTS for hot in 'AB' for sk in (1, 2)] +
                         [(lay, True, 'AB'[i % 2], 1 + i // 2 % 2) for i, lay in enumerate(gc.LAYOUTS)])
def test_single_products_of_the_fp32_kernel(lay, big, hot, splitk):
    c = _onehot_case(lay, big, splitk)
    A, B = gc.onehot_operands(c.M, c.N, c.K, hot, seed=7 + splitk)
    want = (A.double() @ B.double()).float()
    assert bool((want != 0).all())
    d = dict(A=A[None], B=B[None], bias=None, C0=torch.zeros(c.batch, c.M, c.N))
    y0, y1, _ = run_case(c, d)
    for y in (y0, y1):
        ulp = int(gc.ulp_distance(y[:, 0], want.expand(c.batch, c.M, c.N)).max())
        print(f'{c.name} hot {hot}: max deviation from the correctly rounded product {ulp} ulp')
        assert ulp <= ONEHOT_ULP_CAP, (c.name, ulp)


# ---- e. the fold of stored slices against fp64 (and against the same fp32 additions in the same order)
FOLDS = {          # S, rows, N, bias, relu, accumulate
    'S1 bias': (1, 33, 130, True, 0, 0),
    'S5 bias relu': (5, 33, 130, True, 1, 0),
    'S5 accumulate': (5, 33, 130, False, 0, 1),
    'S5 bias relu accumulate': (5, 7, 130, True, 1, 1),
    'S2 grid-stride': (2, 8100, 130, True, 0, 1),          # MN = 1 053 000 > 4096 * 256: the capped grid loops
}


def _fold_job(name):
    S, rows, N, has_bias, relu, acc = FOLDS[name]
    g = torch.Generator().manual_seed(S * 1000 + rows)
    part = torch.randn(S, rows, N, generator=g) * torch.exp(2.0 * torch.randn(1, rows, 1, generator=g))
    bias = torch.randn(N, generator=g) if has_bias else None
    y0 = torch.randn(rows, N, generator=g)
    ref = part.double().sum(0) + (bias.double() if has_bias else 0.0) + (y0.double() if acc else 0.0)
    mag = part.double().abs().sum(0) + (bias.double().abs() if has_bias else 0.0) + (y0.double().abs() if acc else 0.0)
    seq = bias.expand(rows, N).clone() if has_bias else torch.zeros(rows, N)          # the kernel's own order, in fp32
    for s in range(S):
        seq = seq + part[s]
    if acc:
        seq = seq + y0
    if relu:
        ref, seq = torch.relu(ref), torch.relu(seq)
    return dict(S=S, MN=rows * N, N=N, relu=relu, acc=acc, part=part, bias=bias, y0=y0, ref=ref, mag=mag, seq=seq)


def _fold_check(name, j, y):
    # one rounding per addition: S slices (+ 1 onto y), the first onto the bias or onto zero (exact): (S + 1) U A covers them all
    ex = gc.elementwise_excess(y, j['ref'], j['mag'], 0, c=j['S'] + 1)
    print(f'fold {name}: excess of {j["S"] + 1} U A = {ex:.3f}')
    assert ex <= 1.0, (name, ex)
    assert torch.equal(y.cpu().view(torch.int32), j['seq'].view(torch.int32)), name


def _fold_buffers(j):
    """y inside a NaN buffer (store) or holding y0 (accumulate), NaN in front and behind."""
    buf = torch.full((gc.OFF + j['MN'] + gc.TAIL,), float('nan'))
    if j['acc']:
        buf[gc.OFF:gc.OFF + j['MN']] = j['y0'].reshape(-1)
    return buf.to(DEV), j['part'].to(DEV), (j['bias'].to(DEV) if j['bias'] is not None else None)


def _fold_canaries(name, j, buf):
    out = buf.cpu()
    assert bool(torch.isnan(out[:gc.OFF]).all()) and bool(torch.isnan(out[gc.OFF + j['MN']:]).all()), f'{name}: written outside y'
    y = out[gc.OFF:gc.OFF + j['MN']].view(-1, j['N'])
    assert not bool(torch.isnan(y).any()), name
    return y


@pytest.mark.parametrize('name', sorted(FOLDS))
def test_fold_against_fp64(name):
    from jvae_hip import lib as L
    j = _fold_job(name)
    buf, part, bias = _fold_buffers(j)
    L.check(L.load().jvae_splitk_fold_f32(L.ptr(part), L.ptr(bias), buf[gc.OFF:].data_ptr(), j['S'], j['MN'], j['N'], j['relu'], j['acc'],
                                          L.stream_ptr()), 'jvae_splitk_fold_f32')
    _sync()
    _fold_check(name, j, _fold_canaries(name, j, buf))


def test_grouped_fold_with_a_capped_record_equals_the_folds_alone():
    """Three folds in one launch, the middle one with the capped grid (its record's own grid-stride loop): each equals the fold
    alone bit for bit (which test_fold_against_fp64 holds against fp64), nothing is written outside any y."""
    from jvae_hip import ops
    names = ['S5 bias relu', 'S2 grid-stride', 'S5 accumulate']
    jobs = [_fold_job(n) for n in names]
    bufs = [_fold_buffers(j) for j in jobs]
    ops.splitk_fold_group([(part, bias, buf[gc.OFF:], j['S'], j['MN'], j['N'], j['relu'], j['acc'])
                           for j, (buf, part, bias) in zip(jobs, bufs)])
    _sync()
    for n, j, (buf, _, _) in zip(names, jobs, bufs):
        _fold_check(n, j, _fold_canaries(n, j, buf))
