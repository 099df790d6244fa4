"""GPU: independent dense products as one grouped launch (jvae_gemm_group_f32, jvae_splitk_fold_group_f32, ops.linear_pair,
the grouped backward of ops.linear).  A grouped product runs the kernel, the tiles and the K slices it gets alone, so everything
here is compared with torch.equal against the single-product entry points called one by one on the same inputs: no tolerances."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _rand(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV)


class Product:
    """One product: its operands, strides and an output buffer per call."""

    def __init__(self, name, M, N, K, A, sA, B, sB, cshape, sC, batch=1, bias=None, bias_mode=0, flags=0):
        self.name, self.M, self.N, self.K = name, M, N, K
        self.A, self.sA, self.B, self.sB, self.cshape, self.sC, self.batch = A, sA, B, sB, cshape, sC, batch
        self.bias, self.bias_mode, self.flags = bias, bias_mode, flags

    def out(self):
        return torch.full(self.cshape, float('nan'), device=DEV)

    def alone(self):
        from jvae_hip import ops
        C = self.out()
        ops.gemm(self.M, self.N, self.K, self.A, self.sA, self.B, self.sB, C, self.sC, bias=self.bias, bias_mode=self.bias_mode,
                 flags=self.flags, batch=self.batch)
        return C

    def desc(self, C):
        from jvae_hip import ops
        return ops.gemm_desc(self.M, self.N, self.K, self.A, self.sA, self.B, self.sB, C, self.sC, bias=self.bias,
                             bias_mode=self.bias_mode, flags=self.flags, batch=self.batch)


def P1(seed=1):          # linear-forward strides (x row-major, W (N, K) row-major), ragged M and N, bias and ReLU in the epilogue
    M, N, K = 70, 10, 64
    return Product('P1', M, N, K, _rand(M, K, seed=seed), (K, 1, 0), _rand(N, K, seed=seed + 100), (1, K, 0), (M, N), (N, 1, 0),
                   bias=_rand(N, seed=seed + 200), bias_mode=1, flags=2)


def P2(seed=2):          # K = 33: below the split-bf16 kernel's K and no multiple of 4 - the fp32 tile kernel, scalar tail loads
    M, N, K = 64, 800, 33
    return Product('P2', M, N, K, _rand(M, K, seed=seed), (K, 1, 0), _rand(K, N, seed=seed + 100), (N, 1, 0), (M, N), (N, 1, 0))


def P3(seed=3):          # K = 512 as 4 slices stored side by side, both operands contiguous along m / n (the weight-gradient form)
    M, N, K, S = 10, 130, 512, 4
    Ks = K // S
    return Product('P3', M, N, Ks, _rand(K, M, seed=seed), (1, M, Ks * M), _rand(K, N, seed=seed + 100), (N, 1, Ks * N),
                   (S, M, N), (N, 1, M * N), batch=S)


def P4(seed=4):
    return Product('P4', 1, 1, 1, _rand(1, 1, seed=seed), (1, 1, 0), _rand(1, 1, seed=seed + 100), (1, 1, 0), (1, 1), (1, 1, 0))


def P5(seed=5):          # K = 70 >= 64 and no multiple of 4: the one-stage form of the split-bf16 kernel
    M, N, K = 64, 130, 70
    return Product('P5', M, N, K, _rand(M, K, seed=seed), (K, 1, 0), _rand(K, N, seed=seed + 100), (N, 1, 0), (M, N), (N, 1, 0))


def P6(seed=6):          # 23 x 24 = 552 tiles of 128 x 128 (>= 512) and K < 64: the large fp32 tile, ragged on both sides
    M, N, K = 2900, 2950, 9
    return Product('P6', M, N, K, _rand(M, K, seed=seed), (K, 1, 0), _rand(N, K, seed=seed + 100), (1, K, 0), (M, N), (N, 1, 0))


GROUPS = {
    'big_tiles': lambda: [P2(), P6()],
    'one': lambda: [P1()],
    'mixed': lambda: [P1(), P2(), P3(), P4()],
    'mixed_x3': lambda: [P3(), P4(), P5(), P1()],
    'same_shape_other_buffers': lambda: [P3(), P3(seed=33)],
    'eight': lambda: [P4(seed=40 + i) for i in range(8)],
    'none': lambda: [],
}


@pytest.mark.parametrize('group', sorted(GROUPS))
def test_grouped_products_equal_the_products_alone(group):
    from jvae_hip import ops
    prods = GROUPS[group]()
    want = [p.alone() for p in prods]
    got = [p.out() for p in prods]
    ops.gemm_group([p.desc(C) for p, C in zip(prods, got)])
    torch.cuda.synchronize()
    for p, a, b in zip(prods, got, want):
        assert not torch.isnan(b).any(), p.name
        assert torch.equal(a, b), (group, p.name)


def test_wanted_splits_store_the_slices_side_by_side():
    """The deterministic split-K form of a descriptor (want_splits, sCsplit) cuts K itself: the slices of P3 it makes are the
    slices of the batched launch, and their number comes back per descriptor."""
    from jvae_hip import lib as L
    p = P3()
    want = p.alone()
    M, N, K, S = p.M, p.N, 512, 4
    got = p.out()
    other = P1()
    got1 = other.out()
    arr = (L.GemmDesc * 2)()
    made = (ctypes.c_int * 2)(-1, -1)
    d = arr[0]
    d.M, d.N, d.K, d.batch = M, N, K, 1
    d.A, d.sAm, d.sAk, d.sAb = p.A.data_ptr(), 1, M, 0
    d.B, d.sBk, d.sBn, d.sBb = p.B.data_ptr(), N, 1, 0
    d.C, d.sCm, d.sCn, d.sCb = got.data_ptr(), N, 1, 0
    d.want_splits, d.sCsplit = S, M * N
    d.splits = ctypes.cast(made, ctypes.POINTER(ctypes.c_int))
    d = arr[1]
    d.M, d.N, d.K, d.batch = other.M, other.N, other.K, 1
    d.A, (d.sAm, d.sAk, d.sAb) = other.A.data_ptr(), other.sA
    d.B, (d.sBk, d.sBn, d.sBb) = other.B.data_ptr(), other.sB
    d.C, (d.sCm, d.sCn, d.sCb) = got1.data_ptr(), other.sC
    d.bias, d.bias_mode, d.flags, d.splitk = other.bias.data_ptr(), 1, 2, 1
    L.check(L.load().jvae_gemm_group_f32(arr, 2, L.stream_ptr()), 'jvae_gemm_group_f32')
    torch.cuda.synchronize()
    assert made[0] == S
    assert torch.equal(got, want)
    assert torch.equal(got1, other.alone())


def test_grouped_fold_equals_the_folds_alone():
    from jvae_hip import lib as L, ops
    lib = L.load()
    part_a = P3().alone()                                    # (4, 10, 130)
    S_b, R_b, O_b = 5, 8, 64                                 # a second sliced product with a bias and ReLU
    part_b = _rand(S_b, R_b, O_b, seed=7)
    bias_b = _rand(O_b, seed=8)
    base_a = _rand(10, 130, seed=9)                          # job a accumulates onto what y holds (the weight-gradient fold)
    jobs = [(part_a, None, None, 4, 10 * 130, 130, 0, 1), (part_b, bias_b, None, S_b, R_b * O_b, O_b, 1, 0)]
    want, got = [], []
    for part, bias, _, S, MN, N, relu, acc in jobs:
        y = base_a.clone() if acc else torch.full((MN,), float('nan'), device=DEV)
        L.check(lib.jvae_splitk_fold_f32(L.ptr(part), L.ptr(bias), L.ptr(y), S, MN, N, relu, acc, L.stream_ptr()), 'fold')
        want.append(y)
        got.append(base_a.clone() if acc else torch.full((MN,), float('nan'), device=DEV))
    ops.splitk_fold_group([(part, bias, y, S, MN, N, relu, acc) for (part, bias, _, S, MN, N, relu, acc), y in zip(jobs, got)])
    ops.splitk_fold_group([])
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert not torch.isnan(b).any()
        assert torch.equal(a, b)


def _leaves(R, I, O, bias, seed, params):
    x = _rand(R, I, seed=seed)
    ws = [_rand(O, I, seed=seed + 1 + h) / I ** 0.5 for h in range(2)]
    bs = [_rand(O, seed=seed + 11 + h) if bias else None for h in range(2)]
    gs = [_rand(R, O, seed=seed + 21 + h) for h in range(2)]
    if params:          # parameters whose .grad is in place: the backward kernels add straight into it
        ws = [torch.nn.Parameter(w) for w in ws]
        bs = [torch.nn.Parameter(b) if b is not None else None for b in bs]
        for i, t in enumerate(ws + [b for b in bs if b is not None]):
            t.grad = _rand(*t.shape, seed=seed + 31 + i)
    else:
        ws = [w.requires_grad_(True) for w in ws]
        bs = [b.requires_grad_(True) if b is not None else None for b in bs]
    return x, ws, bs, gs


@pytest.mark.parametrize('R', [8, 130, 512])                     # 512: the weight gradient runs in row slices (the bench's batch)
@pytest.mark.parametrize('I,O', [(800, 64), (20, 3)])            # (800, 64): split-K forward, the bench's own width
@pytest.mark.parametrize('bias', [True, False])
@pytest.mark.parametrize('mode', ['all', 'x_off', 'second_unused', 'slots'])
def test_linear_pair_equals_two_linear_calls(R, I, O, bias, mode):
    from jvae_hip import ops
    res = []
    for pair in (False, True):
        x, ws, bs, gs = _leaves(R, I, O, bias, seed=R + I, params=(mode == 'slots'))
        x.requires_grad_(mode != 'x_off')
        if pair:
            y0, y1 = ops.linear_pair(x, ws[0], bs[0], ws[1], bs[1])
        else:
            y0, y1 = ops.linear(x, ws[0], bs[0]), ops.linear(x, ws[1], bs[1])
        if mode == 'second_unused':
            y0.backward(gs[0])
        else:
            torch.autograd.backward((y0, y1), (gs[0], gs[1]))
        torch.cuda.synchronize()
        res.append([y0.detach(), y1.detach(), x.grad] + [w.grad for w in ws] + [b.grad if b is not None else None for b in bs])
    names = ['y0', 'y1', 'gx', 'gw0', 'gw1', 'gb0', 'gb1']
    for n, a, b in zip(names, res[1], res[0]):
        assert (a is None) == (b is None), n
        if a is not None:
            assert torch.equal(a, b), n
    assert (res[0][2] is None) == (mode == 'x_off')
    if mode == 'second_unused':
        assert res[1][4] is None and res[1][6] is None


@pytest.mark.parametrize('R,I,O,act', [(130, 800, 64, 'ident'), (512, 800, 64, 'relu'), (8, 20, 3, 'ident')])
def test_linear_backward_grouped_equals_the_products_alone(R, I, O, act):
    """ops.linear's backward (dgrad and weight gradient in one launch) against the same products through jvae_gemm_f32 and
    jvae_splitk_fold_f32 one by one, with the strides and row slices the layer has always used."""
    from jvae_hip import lib as L, ops
    x = _rand(R, I, seed=R).requires_grad_(True)
    w = (_rand(O, I, seed=R + 1) / I ** 0.5).requires_grad_(True)
    b = _rand(O, seed=R + 2).requires_grad_(True)
    g = _rand(R, O, seed=R + 3)
    y = ops.linear(x, w, b, ops.RELU if act == 'relu' else ops.IDENT)
    y.backward(g)
    gy = torch.where(y.detach() > 0, g, torch.zeros_like(g)) if act == 'relu' else g
    gx = torch.empty(R, I, device=DEV)
    ops.gemm(R, I, O, gy, (O, 1, 0), w.detach(), (I, 1, 0), gx, (I, 1, 0))
    gw = torch.zeros(O, I, device=DEV)
    S = ops._linear_split(O, I, R)
    assert (S > 1) == (R == 512)
    if S > 1:
        part = torch.empty(S, O, I, device=DEV)
        Rs = R // S
        ops.gemm(O, I, Rs, gy, (1, O, Rs * O), x.detach(), (I, 1, Rs * I), part, (I, 1, O * I), batch=S)
        L.check(L.load().jvae_splitk_fold_f32(L.ptr(part), None, L.ptr(gw), S, O * I, I, 0, 1, L.stream_ptr()), 'fold')
    else:
        ops.gemm(O, I, R, gy, (1, O, 0), x.detach(), (I, 1, 0), gw, (I, 1, 0), flags=1)
    torch.cuda.synchronize()
    assert torch.equal(x.grad, gx)
    assert torch.equal(w.grad, gw)
    assert torch.equal(b.grad, ops.channel_sum(gy, R, O, 1))


def test_linear_pair_is_capture_safe():
    """Forward and backward of linear_pair captured in one graph and replayed twice on changed inputs equal the eager result:
    the records of a grouped launch travel in the kernel arguments, nothing is uploaded at launch time."""
    from jvae_hip import ops
    R, I, O = 130, 800, 64

    def run(x, ws, bs, gs):
        y0, y1 = ops.linear_pair(x, ws[0], bs[0], ws[1], bs[1])
        grads = torch.autograd.grad((y0, y1), [x] + ws + bs, (gs[0], gs[1]))
        return [y0.detach(), y1.detach()] + list(grads)

    x, ws, bs, gs = _leaves(R, I, O, True, seed=1, params=False)
    x.requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(x, ws, bs, gs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(x, ws, bs, gs)
    for seed in (50, 60):
        nx, nws, nbs, ngs = _leaves(R, I, O, True, seed=seed, params=False)
        with torch.no_grad():
            for dst, src in zip([x] + ws + bs + gs, [nx] + nws + nbs + ngs):
                dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in outs]
        nx.requires_grad_(True)
        want = run(nx, nws, nbs, ngs)
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b)
