"""Every row of tests/bn_cases.py on the device, through the raw BatchNorm entry points of both layouts (ops.F32.bn /
ops_b8.B8.bn: one body): sums, training forward, finalize, eval forward, backward (fresh and accumulated), eval backward and the
synchronised protocol with the all-reduce done on the host, each against the fp64 references and derived bounds of bn_cases -
sums at the depth of the kernel's summation tree, moments at one ulp of the fp64 moments of the kernel's own sums, y and dx
element by element from what the kernel published - and each entry point twice, bit for bit.  Then the claim the kernels are
built on - backward re-derives the forward's ReLU mask exactly - on data that sits on the threshold, the refusals, and N = 0."""
import zlib

import pytest
import torch

import bn_cases as bc
from jvae_hip import lib, ops, ops_b8

pytestmark = pytest.mark.gpu
DEV = 'cuda'
POISON = 12288.0          # exact in bf16
NBT0 = 5
P_ = lib.ptr
ids = lambda c: c.name.replace(' ', '_')


def twice(f):
    """Two launches, bit for bit."""
    a, b = f(), f()
    for s, t in zip(a, b):
        assert (s is None and t is None) or torch.equal(s, t), 'two runs differ'
    return a


class Run:
    """The entry points of one layout on (N, C, P) operands; every call gets fresh, poisoned outputs."""

    def __init__(self, case):
        self.case, self.lay = case, (ops_b8.B8 if case.b8 else ops.F32)
        self.C, self.P, self.C8 = case.C, case.P, self.lay.coef_width(case.C)
        L = lib.load()
        self.nbytes = (L.jvae_bn_workspace_bytes_b8 if case.b8 else L.jvae_bn_workspace_bytes)(case.C)
        self.ws = torch.zeros(self.nbytes, dtype=torch.uint8, device=DEV)

    def put(self, t):
        return (bc.to_b8(t) if self.case.b8 else t).to(DEV).contiguous()

    def get(self, t):
        """-> (N, C, P) fp32 on the CPU; the padding channels of a B8 tensor must be zero."""
        if not self.case.b8:
            return t.detach().cpu()
        v, pad = bc.from_b8(t, self.C)
        assert bool((pad == 0).all()), f'{self.case.name}: padding channels of a B8 result are not zero'
        return v

    def vec(self, t=None, fill=POISON):
        return torch.full((self.C,), fill, device=DEV) if t is None else t.to(DEV)

    def partials(self, nsplit):
        return self.ws.view(torch.float32)[:self.C * nsplit * 2].view(self.C, nsplit, 2).clone().cpu()

    def _run(self, run):
        if run is None:
            return None, None, None
        return run[0].to(DEV), run[1].to(DEV), torch.full((), NBT0, dtype=torch.int64, device=DEV)

    def sums(self, x, pivot, ws=None):
        s = torch.full((self.C, 2), POISON, device=DEV)
        self.lay.bn('jvae_bn_sums', P_(x), P_(pivot), P_(s), x.shape[0], self.C, self.P, ws=self.ws if ws is None else ws)
        return (s,)

    def fwd(self, x, gamma, beta, run, training, act, ws=None, mean=True, y=None):
        rm, rv, nbt = self._run(run)
        y = torch.full_like(x, POISON) if y is None else y
        mean, invstd = (self.vec(), self.vec()) if mean else (None, None)
        self.lay.bn_fwd(P_(x), P_(gamma), P_(beta), P_(rm), P_(rv), P_(nbt), P_(y), P_(mean), P_(invstd), x.shape[0], self.C,
                        self.P, bc.MOMENTUM, bc.EPS, int(training), act, ext=(None, 0, None), ws=self.ws if ws is None else ws)
        return y, mean, invstd, rm, rv, nbt

    def finalize(self, x, gamma, beta, run, training, ws=None, mean=True):
        rm, rv, nbt = self._run(run)
        mean, invstd = (self.vec(), self.vec()) if mean else (None, None)
        coef = torch.full((2, self.C8), POISON, device=DEV)
        self.lay.bn('jvae_bn_finalize', P_(x), P_(gamma), P_(beta), P_(rm), P_(rv), P_(nbt), P_(mean), P_(invstd),
                    *self.lay.coef_args(coef), x.shape[0], self.C, self.P, bc.MOMENTUM, bc.EPS, int(training), None, 0, None,
                    ws=self.ws if ws is None else ws)
        return coef, mean, invstd, rm, rv, nbt

    def bwd(self, dy, x, gamma, beta, mean, invstd, act, grads=None, ws=None, dx=None):
        dx = torch.full_like(x, POISON) if dx is None else dx
        dg, db = (self.vec(), self.vec()) if grads is None else (grads[0].to(DEV), grads[1].to(DEV))
        self.lay.bn('jvae_bn_bwd', P_(dy), P_(x), P_(gamma), P_(beta), P_(mean), P_(invstd), P_(dx), P_(dg), P_(db),
                    int(grads is not None), x.shape[0], self.C, self.P, act, ws=self.ws if ws is None else ws)
        return dx, dg, db

    def eval_bwd(self, dy, x, gamma, beta, rm, rv, act):
        dx = torch.full_like(x, POISON)
        lib.check(lib.load().jvae_bn_eval_bwd_f32(P_(dy), P_(x), P_(gamma), P_(beta), P_(rm), P_(rv), P_(dx), x.shape[0], self.C,
                                                  self.P, bc.EPS, act, lib.stream_ptr()), 'jvae_bn_eval_bwd_f32')
        return (dx,)

    def fwd_sync(self, x, gamma, beta, run, act, gsums, pivot, world, ws=None, y=None):
        rm, rv, nbt = self._run(run)
        y = torch.full_like(x, POISON) if y is None else y
        mean, invstd = self.vec(), self.vec()
        self.lay.bn('jvae_bn_fwd_sync', P_(x), P_(gamma), P_(beta), P_(rm), P_(rv), P_(nbt), P_(y), P_(mean), P_(invstd),
                    x.shape[0], self.C, self.P, bc.MOMENTUM, bc.EPS, act, P_(gsums), P_(pivot), world,
                    ws=self.ws if ws is None else ws)
        return y, mean, invstd, rm, rv, nbt

    def bwd_sums(self, dy, x, gamma, beta, mean, invstd, act, ws=None, local=None):
        local = torch.full((self.C, 2), POISON, device=DEV) if local is None else local
        self.lay.bn('jvae_bn_bwd_sums', P_(dy), P_(x), P_(gamma), P_(beta), P_(mean), P_(invstd), P_(local), x.shape[0], self.C,
                    self.P, act, ws=self.ws if ws is None else ws)
        return (local,)

    def bwd_sync(self, dy, x, gamma, beta, mean, invstd, local, glob, world, act, grads=None, ws=None, dx=None):
        dx = torch.full_like(x, POISON) if dx is None else dx
        dg, db = (self.vec(), self.vec()) if grads is None else (grads[0].to(DEV), grads[1].to(DEV))
        self.lay.bn_bwd_sync(P_(dy), P_(x), P_(gamma), P_(beta), P_(mean), P_(invstd), P_(local), P_(glob), world, P_(dx), P_(dg),
                             P_(db), int(grads is not None), x.shape[0], self.C, self.P, act, ws=self.ws if ws is None else ws)
        return dx, dg, db


def report(case, entry, what, ex):
    print(f'BN {entry} | {case.name} | {what}: {ex:.3g}')
    assert ex <= 1, (case.name, entry, what, ex)


def check_sums(case, entry, got, ref, A, kinds):
    D = bc.depth(case)
    for i, k in enumerate(kinds):
        report(case, entry, f'sum {k} (D = {D})', bc.sum_excess(got[:, i], ref[:, i], A[:, i], D, bc.C_SUM[k]))


def check_elements(case, entry, what, got, ref, A, c):
    ex = bc.elementwise_excess(got, ref, A, 0, c, bc.UB if case.b8 else 0.0)
    worst, where = bc.worst_plane(got, ref, A)
    print(f'BN {entry} | {case.name} | {what}: worst plane {worst:.3g} at (image, channel) {where}')
    report(case, entry, what, ex)


def check_moments(case, entry, out, s64, n, pv, run0):
    """mean / invstd at one ulp of the fp64 moments of the kernel's own sums; the running statistics' blend at 3 U A."""
    _, mean, invstd, rm, rv, nbt = out
    mean64, _, invstd64, unb64 = bc.moments64(s64, n, pv)
    report(case, entry, 'mean, ulps', bc.ulp_excess(mean, mean64))
    report(case, entry, 'invstd, ulps', bc.ulp_excess(invstd, invstd64))
    if run0 is not None:
        report(case, entry, 'running mean', bc.bound_excess(rm, *bc.blend64(run0[0], mean.cpu()), 3))
        report(case, entry, 'running var', bc.bound_excess(rv, *bc.blend64(run0[1], unb64), 3))
        assert int(nbt) == NBT0 + 1


@pytest.mark.parametrize('case', bc.ROWS, ids=ids)
def test_bn_sweep(case):
    d = bc.make_data(case)
    r = Run(case)
    N, Cn, P, act, W = case.N, case.C, case.P, case.act, case.world
    ns = case.plan[0]
    cy, cdx = 4 + (act == 2), bc.C_DX
    g64, b64 = bc.ones_or(d['gamma'], Cn, 1.), bc.ones_or(d['beta'], Cn, 0.)
    gam, bet = (d['gamma'].to(DEV), d['beta'].to(DEV)) if case.affine else (None, None)
    run0 = (d['rm0'], d['rv0']) if case.running else None
    pivot = d['pivot'].to(DEV)
    xs, dys = [d['x'][k * N:(k + 1) * N] for k in range(W)], [d['dy'][k * N:(k + 1) * N] for k in range(W)]
    xd, dyd = [r.put(t) for t in xs], [r.put(t) for t in dys]
    x0, dy0 = xs[0], dys[0]
    n = N * P

    # ---- one rank on its own: training forward (own pivot x[0][c][0]), finalize, backward
    out = twice(lambda: r.fwd(xd[0], gam, bet, run0, 1, act))
    part = r.partials(ns)
    pv = x0[0, :, 0]
    ref, A = bc.fwd_sums64(x0, pv)
    check_sums(case, 'bn_fwd', part.double().sum(1), ref, A, ('d', 'd2'))
    check_moments(case, 'bn_fwd', out, part.double().sum(1), n, pv, run0)
    y, mean, invstd = r.get(out[0]), out[1].cpu(), out[2].cpu()
    check_elements(case, 'bn_fwd', 'y', y, *bc.y64(x0, g64, b64, mean, invstd, act), cy)
    if case.const:
        assert bool((y[:, 0] == (bc.CONST_BETA if case.affine else 0.)).all()), 'a constant channel must give y == beta exactly'
    fin = twice(lambda: r.finalize(xd[0], gam, bet, run0, 1))
    for a, b in zip(out[1:], fin[1:]):          # nsplit <= 64: one wave's worth of partials, the fold shapes agree to the bit
        assert (a is None and b is None) or torch.equal(a, b), 'finalize and forward publish different statistics'
    coef = fin[0].cpu()
    sc64, sh64, Ash = bc.coef64(g64, b64, mean, invstd)
    report(case, 'bn_finalize', 'scale, ulps', bc.ulp_excess(coef[0, :Cn], sc64))
    report(case, 'bn_finalize', 'shift', bc.bound_excess(coef[1, :Cn], sh64, Ash, 3))
    assert bool((coef[:, Cn:] == 0).all()), 'coefficients of padding channels must be zero'

    mask = y > 0
    g = bc.masked(dy0, mask, act)
    bw = twice(lambda: r.bwd(dyd[0], xd[0], gam, bet, out[1], out[2], act))
    dx, dgb = r.get(bw[0]), torch.stack([bw[2].cpu(), bw[1].cpu()], 1)          # (dbeta, dgamma) = (sum g, sum g xhat)
    check_sums(case, 'bn_bwd', dgb, *bc.bwd_sums64(x0, g, mean, invstd), ('g', 'gx'))
    check_elements(case, 'bn_bwd', 'dx', dx, *bc.dx64(x0, g, g64, mean, invstd, *bc.means32(dgb, n)), cdx)
    if case.accumulate:
        acc = twice(lambda: r.bwd(dyd[0], xd[0], gam, bet, out[1], out[2], act, grads=(d['dg0'], d['db0'])))
        assert torch.equal(acc[0], bw[0]), 'accumulate changes dx'
        assert torch.equal(acc[1], d['dg0'].to(DEV) + bw[1]) and torch.equal(acc[2], d['db0'].to(DEV) + bw[2])

    # ---- eval mode: the scale at the project's eval bar, the apply stage from the coefficients an eval finalize published
    rm0, rv0 = d['rm0'].to(DEV), d['rv0'].to(DEV)
    efin = twice(lambda: r.finalize(xd[0], gam, bet, (d['rm0'], d['rv0']), 0))
    ecoef = efin[0].cpu()
    esc, esh = ecoef[0, :Cn], ecoef[1, :Cn]
    sc_true = g64 / torch.sqrt(d['rv0'].double() + bc.EPS)
    rel = float(((esc.double() - sc_true).abs() / sc_true.abs()).max())
    print(f'BN bn_finalize eval | {case.name} | scale: {rel:.3g} relative (bar {bc.EVAL_SCALE_BAR})')
    assert rel < bc.EVAL_SCALE_BAR
    prod = d['rm0'].double() * esc.double()         # shift = fl(beta - fl(rm * scale)): 2 U (|beta| + |rm scale|), fused or not
    report(case, 'bn_finalize eval', 'shift', bc.bound_excess(esh, b64 - prod, b64.abs() + prod.abs(), 2))
    assert bool((ecoef[:, Cn:] == 0).all()) and torch.equal(efin[3], rm0) and torch.equal(efin[4], rv0) and int(efin[5]) == NBT0
    ev = twice(lambda: r.fwd(xd[0], gam, bet, (d['rm0'], d['rv0']), 0, act))
    assert torch.equal(ev[3], rm0) and torch.equal(ev[4], rv0) and int(ev[5]) == NBT0
    ye = r.get(ev[0])
    check_elements(case, 'bn_fwd eval', 'y', ye, *bc.y_eval64(x0, esc, esh, act), 1 + (act == 2))
    if not case.b8:
        eb = twice(lambda: r.eval_bwd(dyd[0], xd[0], gam, bet, rm0, rv0, act))
        ge = bc.masked(dy0, ye > 0, act) * esc.double().view(1, -1, 1)
        check_elements(case, 'bn_eval_bwd', 'dx', r.get(eb[0]), ge, ge.abs(), 1 + (act == 2))

    # ---- the synchronised protocol, the all-reduce done here: fp32 additions in rank order
    s = [twice(lambda k=k: r.sums(xd[k], pivot))[0] for k in range(W)]
    tot_ref, tot_A = 0., 0.
    for k in range(W):
        ref, A = bc.fwd_sums64(xs[k], d['pivot'])
        check_sums(case, 'bn_sums', s[k].cpu(), ref, A, ('d', 'd2'))
        tot_ref, tot_A = tot_ref + ref, tot_A + A
    gs = s[0].clone()
    for k in range(1, W):
        gs += s[k]
    fw = [twice(lambda k=k: r.fwd_sync(xd[k], gam, bet, run0, act, gs, pivot, W)) for k in range(W)]
    for k in range(1, W):
        for a, b in zip(fw[0][1:], fw[k][1:]):
            assert (a is None and b is None) or torch.equal(a, b), 'ranks publish different statistics'
    check_moments(case, 'bn_fwd_sync', fw[0], gs.cpu(), n * W, d['pivot'], run0)
    mean, invstd = fw[0][1].cpu(), fw[0][2].cpu()
    # ... and the mean against the whole batch in fp64: every rank's sum is inside (D + 2) U A_r, the W - 1 host additions round
    # relative to at most the total A, the moments are fp64 and rounded once
    mean_true = d['pivot'].double() + tot_ref[:, 0] / (n * W)
    slack = (bc.depth(case) + bc.C_SUM['d'] + W - 1) * bc.U * tot_A[:, 0] / (n * W) + bc.U * mean_true.abs()
    report(case, 'bn_fwd_sync', 'mean against the whole batch', bc.bound_excess(mean, mean_true, slack / bc.U, 1))
    ys = [r.get(fw[k][0]) for k in range(W)]
    gsm = []
    loc = []
    for k in range(W):
        check_elements(case, 'bn_fwd_sync', f'y, rank {k}', ys[k], *bc.y64(xs[k], g64, b64, mean, invstd, act), cy)
        gsm.append(bc.masked(dys[k], ys[k] > 0, act))
        loc.append(twice(lambda k=k: r.bwd_sums(dyd[k], xd[k], gam, bet, fw[0][1], fw[0][2], act))[0])
        check_sums(case, 'bn_bwd_sums', loc[k].cpu(), *bc.bwd_sums64(xs[k], gsm[k], mean, invstd), ('g', 'gx'))
    glob = loc[0].clone()
    for k in range(1, W):
        glob += loc[k]
    m1, m2 = bc.means32(glob.cpu(), n * W)
    for k in range(W):
        bs = twice(lambda k=k: r.bwd_sync(dyd[k], xd[k], gam, bet, fw[0][1], fw[0][2], loc[k], glob, W, act))
        assert torch.equal(bs[2], loc[k][:, 0].contiguous()) and torch.equal(bs[1], loc[k][:, 1].contiguous()), 'dgamma / dbeta are the LOCAL sums'
        check_elements(case, 'bn_bwd_sync', f'dx, rank {k}', r.get(bs[0]), *bc.dx64(xs[k], gsm[k], g64, mean, invstd, m1, m2), cdx)
        if case.accumulate:
            acc = r.bwd_sync(dyd[k], xd[k], gam, bet, fw[0][1], fw[0][2], loc[k], glob, W, act, grads=(d['dg0'], d['db0']))
            assert torch.equal(acc[0], bs[0])
            assert torch.equal(acc[1], d['dg0'].to(DEV) + bs[1]) and torch.equal(acc[2], d['db0'].to(DEV) + bs[2])


def _on_threshold(mean, scale, x0, Cn):
    """beta per channel such that the threshold -shift / scale of fmaf(x, scale, shift) > 0 lands on the grid value x0[c]:
    fl32((mean - x0) scale), moved by -2 .. +2 ulps across the channels."""
    beta = ((mean.double() - x0.double()) * scale.double()).float()
    for c in range(Cn):
        j = c % 5 - 2
        for _ in range(abs(j)):
            beta[c] = torch.nextafter(beta[c], torch.tensor(float('inf') if j > 0 else float('-inf')))
    return beta


@pytest.mark.parametrize('case', bc.MASK_ROWS, ids=ids)
def test_backward_rederives_the_forward_mask_exactly(case):
    """Data on the grid of multiples of 2^-3 around 4 (so that mean * scale is of the size of shift, and how that product is rounded
    inside bn_coef shows in shift's last bit) and, per channel, a beta that puts the ReLU threshold on a grid value to within a
    couple of ulps: the elements on that value are in or out by the last bit of bn_coef's shift.  With dy = 1, dbeta is the
    number of elements the backward kernel lets through - an integer in fp32 - and must EQUAL count(y > 0) of the forward
    (leaky ReLU: count + slope (n - count), inside the sums bound of terms that are all positive).  In eval mode (fp32) the
    forward's y > 0 and the backward's dx != 0 are compared element by element."""
    r = Run(case)
    N, Cn, P, act = case.N, case.C, case.P, case.act
    n = N * P
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    x = 4 + torch.randint(-8, 9, (N, Cn, P), generator=g).float() / 8          # 6 significant bits: exact in bf16
    x0 = x[0, :, 0].clone()          # a grid value the channel certainly holds
    gamma = torch.rand(Cn, generator=g) + 0.5
    rv = torch.rand(Cn, generator=g) + 0.5
    xd, one, gam = r.put(x), r.put(torch.ones(N, Cn, P)), gamma.to(DEV)
    on = (x == x0.view(1, -1, 1))
    assert int(on.sum((0, 2)).min()) > 0          # every channel has elements on its threshold
    fin = r.finalize(xd, gam, torch.zeros(Cn, device=DEV), None, 1)          # the statistics do not depend on beta
    beta = _on_threshold(fin[1].cpu(), fin[0][0, :Cn].cpu(), x0, Cn).to(DEV)
    out = r.fwd(xd, gam, beta, None, 1, act)
    assert torch.equal(out[1], fin[1]) and torch.equal(out[2], fin[2])
    y = r.get(out[0])
    let = (y > 0) & on
    sides = int(let.sum()), int(on.sum())
    print(f'{case.name}: {sides[0]} of the {sides[1]} elements on a threshold pass it')
    assert 0 < sides[0] < sides[1]                # the thresholds really cut through the grid value, both ways
    count = (y > 0).sum((0, 2)).double()
    for entry, db in (('bn_bwd', r.bwd(one, xd, gam, beta, out[1], out[2], act)[2]),
                      ('bn_bwd_sums', r.bwd_sums(one, xd, gam, beta, out[1], out[2], act)[0][:, 0])):
        if act == 1:
            assert torch.equal(db.cpu().double(), count), (entry, (db.cpu().double() - count).abs().max())
        else:
            ref = count + bc.SLOPE * (n - count)
            report(case, entry, 'dbeta under a leaky mask', bc.sum_excess(db.cpu(), ref, ref, bc.depth(case), bc.C_SUM['g']))
    if case.b8:
        return
    rm = fin[1]
    efin = r.finalize(xd, gam, torch.zeros(Cn, device=DEV), (rm.cpu(), rv), 0)
    esc = efin[0][0, :Cn]
    ebeta = _on_threshold(rm.cpu(), esc.cpu(), x0, Cn).to(DEV)
    ye = r.get(r.fwd(xd, gam, ebeta, (rm.cpu(), rv), 0, act)[0])
    dxe = r.get(r.eval_bwd(one, xd, gam, ebeta, rm, rv.to(DEV), act)[0])
    passed = (dxe != 0) if act == 1 else (dxe == esc.cpu().view(1, -1, 1))
    assert 0 < int(((ye > 0) & on).sum()) < int(on.sum())
    assert torch.equal(ye > 0, passed), int(((ye > 0) != passed).sum())


def refused(why, f):
    with pytest.raises(lib.JvaeHipError, match=why):
        f()


@pytest.mark.parametrize('layout', ['f32', 'b8'])
def test_refusals(layout):
    """A short workspace is JVAE_EWORKSPACE (-3), a missing save_mean in training JVAE_EINVAL (-1), leaky ReLU on a B8 entry
    point JVAE_ENOTSUP (-2) - before anything is launched: every output keeps its poison."""
    case = bc.CASES[f'{layout} 3x5x3']
    d = bc.make_data(case)
    r = Run(case)
    xd, dyd = r.put(d['x']), r.put(d['dy'])
    gam, bet, piv = d['gamma'].to(DEV), d['beta'].to(DEV), d['pivot'].to(DEV)
    run0 = (d['rm0'], d['rv0'])
    short = r.ws[:r.nbytes - 1]
    mean, invstd = r.vec(fill=0.), r.vec(fill=1.)
    sums = torch.ones(case.C, 2, device=DEV)
    small, none = 'workspace too small', 'invalid argument'
    refused(small, lambda: r.sums(xd, piv, ws=short))
    refused(small, lambda: r.fwd(xd, gam, bet, run0, 1, 1, ws=short))
    refused(small, lambda: r.finalize(xd, gam, bet, run0, 1, ws=short))
    refused(small, lambda: r.bwd(dyd, xd, gam, bet, mean, invstd, 1, ws=short))
    refused(small, lambda: r.fwd_sync(xd, gam, bet, run0, 1, sums, piv, 2, ws=short))
    refused(small, lambda: r.bwd_sums(dyd, xd, gam, bet, mean, invstd, 1, ws=short))
    if case.b8:
        refused(small, lambda: r.bwd_sync(dyd, xd, gam, bet, mean, invstd, sums, sums, 2, 1, ws=short))
    refused(none, lambda: r.fwd(xd, gam, bet, run0, 1, 1, mean=False))
    refused(none, lambda: r.finalize(xd, gam, bet, run0, 1, mean=False))
    if not case.b8:
        return
    no = 'unsupported configuration'
    y, dx, local = torch.full_like(xd, POISON), torch.full_like(xd, POISON), torch.full((case.C, 2), POISON, device=DEV)
    refused(no, lambda: r.fwd(xd, gam, bet, run0, 1, 2, y=y))
    refused(no, lambda: r.fwd(xd, gam, bet, run0, 0, 2, y=y))
    refused(no, lambda: r.fwd_sync(xd, gam, bet, run0, 2, sums, piv, 2, y=y))
    refused(no, lambda: r.bwd(dyd, xd, gam, bet, mean, invstd, 2, dx=dx))
    refused(no, lambda: r.bwd_sums(dyd, xd, gam, bet, mean, invstd, 2, local=local))
    refused(no, lambda: r.bwd_sync(dyd, xd, gam, bet, mean, invstd, sums, sums, 2, 2, dx=dx))
    torch.cuda.synchronize()
    for t in (y, dx, local):
        assert bool((t == POISON).all())
    # ... and through the op: it raises and no longer returns ReLU
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    rm, rv = d['rm0'].to(DEV), d['rv0'].to(DEV)
    refused(no, lambda: ops_b8.batchnorm_act(xd, case.C, gam, bet, rm, rv, nbt, True, 2))
    assert int(nbt) == 0 and torch.equal(rm, d['rm0'].to(DEV)) and torch.equal(rv, d['rv0'].to(DEV))


@pytest.mark.parametrize('layout', ['f32', 'b8'])
def test_an_empty_batch_as_it_is_today(layout):
    """N = 0, pinned per entry point.  fp32: the sums calls return zeros, forward / backward / the sync apply calls return 0 and
    touch nothing, finalize refuses (-1).  bf16: forward and backward return 0 and touch nothing, finalize and the four
    synchronised entry points refuse (-1)."""
    case = bc.CASES[f'{layout} 3x5x3']
    d = bc.make_data(case)
    r = Run(case)
    one = r.put(d['x'][:1])          # one image of room behind every pointer: none of it may be touched
    gam, bet, piv = d['gamma'].to(DEV), d['beta'].to(DEV), d['pivot'].to(DEV)
    mean, invstd, sums = r.vec(fill=0.), r.vec(fill=1.), torch.ones(case.C, 2, device=DEV)
    run0 = (d['rm0'], d['rv0'])
    keep = torch.full_like(one, POISON)
    L = lib.load()
    st, ws = lib.stream_ptr(), (P_(r.ws), r.nbytes)
    C, Pn = case.C, case.P
    rm, rv, nbt = r._run(run0)
    g0, b0 = r.vec(), r.vec()
    sfx = '_b8' if case.b8 else '_f32'
    call = lambda name, *a: getattr(L, name + sfx)(*a)
    ext = (None, 0, None) if case.b8 else ()
    assert call('jvae_bn_fwd', P_(one), P_(gam), P_(bet), P_(rm), P_(rv), P_(nbt), P_(keep), P_(mean), P_(invstd), 0, C, Pn,
                bc.MOMENTUM, bc.EPS, 1, 1, *ext, *ws, st) == 0
    assert call('jvae_bn_bwd', P_(one), P_(one), P_(gam), P_(bet), P_(mean), P_(invstd), P_(keep), P_(g0), P_(b0), 0, 0, C, Pn,
                1, *ws, st) == 0
    coef = torch.full((2, r.C8), POISON, device=DEV)
    assert call('jvae_bn_finalize', P_(one), P_(gam), P_(bet), P_(rm), P_(rv), P_(nbt), P_(mean), P_(invstd),
                *r.lay.coef_args(coef), 0, C, Pn, bc.MOMENTUM, bc.EPS, 1, None, 0, None, *ws, st) == -1
    s = torch.full((C, 2), POISON, device=DEV)
    loc = torch.full((C, 2), POISON, device=DEV)
    rc = {'sums': call('jvae_bn_sums', P_(one), P_(piv), P_(s), 0, C, Pn, *ws, st),
          'fwd_sync': call('jvae_bn_fwd_sync', P_(one), P_(gam), P_(bet), P_(rm), P_(rv), P_(nbt), P_(keep), P_(mean), P_(invstd),
                           0, C, Pn, bc.MOMENTUM, bc.EPS, 1, P_(sums), P_(piv), 2, *ws, st),
          'bwd_sums': call('jvae_bn_bwd_sums', P_(one), P_(one), P_(gam), P_(bet), P_(mean), P_(invstd), P_(loc), 0, C, Pn, 1,
                           *ws, st),
          'bwd_sync': call('jvae_bn_bwd_sync', P_(one), P_(one), P_(gam), P_(bet), P_(mean), P_(invstd), P_(sums), P_(sums), 2,
                           P_(keep), P_(g0), P_(b0), 0, 0, C, Pn, 1, *(ws if case.b8 else ()), st)}
    torch.cuda.synchronize()
    if case.b8:
        assert rc == {'sums': -1, 'fwd_sync': -1, 'bwd_sums': -1, 'bwd_sync': -1}, rc
        assert bool((s == POISON).all()) and bool((loc == POISON).all())
    else:
        assert rc == {'sums': 0, 'fwd_sync': 0, 'bwd_sums': 0, 'bwd_sync': 0}, rc
        assert bool((s == 0).all()) and bool((loc == 0).all())
        assert L.jvae_bn_eval_bwd_f32(P_(one), P_(one), P_(gam), P_(bet), P_(rm), P_(rv), P_(keep), 0, C, Pn, bc.EPS, 1, st) == 0
    torch.cuda.synchronize()
    assert bool((keep == POISON).all()) and bool((coef == POISON).all()) and bool((g0 == POISON).all()) and bool((b0 == POISON).all())
    assert int(nbt) == NBT0 and torch.equal(rm, d['rm0'].to(DEV)) and torch.equal(rv, d['rv0'].to(DEV))
    assert bool((mean == 0).all()) and bool((invstd == 1).all())
