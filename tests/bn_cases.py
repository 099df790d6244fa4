"""The BatchNorm case table shared by tests/test_bn_plans_host.py (CPU: the launch plan every row reaches, an fp32 emulation of
the kernels' summation order against the bounds below, and the mutants those bounds must catch) and tests/test_34_bn_sweep_gpu.py
(GPU: every entry point of csrc/bn.hip and csrc/bn_b8.hip against fp64), with the data recipe, the fp64 references and the
derived bounds both use.  A plain module, not a conftest, in the style of tests/conv_cases.py.

A row names a layout ('f32' NCHW / 'b8' channel-blocked bf16), (N, C, P) - N is the batch of ONE rank, P = H * W - the fused
activation (0 none, 1 ReLU, 2 leaky ReLU: fp32 only), its flags and the launch plan it is there for, as pick_split / pick_chunk
of the two files decide today: (nsplit, nchunk, empty parts of nsplit, empty parts of nchunk, index path).  The index path is
'scalar' (fp32, P % 4 != 0: one float at a time), 'shift' or 'div' (Plane4Idx / UnitIdx with a plane of a power of two or not).
tests/test_bn_plans_host.py asserts the plan through jvae_bn_plan / jvae_bn_plan_b8, so a changed threshold fails there and does
not quietly empty a case.  The shapes are the smallest that reach each plan; the flags are spread over the rows, not multiplied.

References are two-stage, so that every bound is local: the sums are compared with fp64 sums of the same operands at the depth
of the summation tree the kernel uses; the moments with fp64 moments OF THE KERNEL'S OWN fp32 SUMS at one ulp; y and dx with fp64
results from the mean / invstd (dbeta / M, dgamma / M) the kernel published, at a handful of roundings of the terms' magnitudes.
A wrong channel, a dropped image of a ragged part or a mis-indexed tail breaks the first link it touches, on its own scale.

No bound below is tuned: each is a formula with its derivation beside it, or a bar quoted from an existing test by name."""
import math
import zlib

import numpy as np
import torch

from conv_cases import U, UB, elementwise_excess, rbf, worst_plane  # noqa: F401  (re-exported to the two test files)

EPS = float(np.float32(1e-5))            # the kernels take eps as a float and widen it: (double)eps
MOMENTUM = float(np.float32(0.1))        # ... and momentum, which they use in fp32
SLOPE = float(np.float32(0.01))          # JVAE_LEAKY_SLOPE 0.01f
CONST_VALUE, CONST_BETA = 0.5, 0.75      # the constant channel and its beta: see Case.const
EVAL_SCALE_BAR = 1e-5                    # eval-mode scale (rsqrtf): the eval bar of test_0_ops_gpu.py::test_batchnorm_train
MAX_SPLIT = {'f32': 64, 'b8': 512}


class Case:
    """const: channel 0 is CONST_VALUE everywhere (var = 0) and its beta is CONST_BETA.  With the kernel's own pivot x[0][c][0]
    every d = x - pivot is exactly 0, so mean = CONST_VALUE and var = 0 exactly; scale = fl(gamma / sqrt(eps)) < 2^22, so
    CONST_VALUE * scale (a power of two times scale) is exact, CONST_BETA = 3 * 2^-2 is a multiple of its ulp and
    |CONST_BETA - CONST_VALUE * scale| < |CONST_VALUE * scale| (gamma > 0) stays in its binade or below: shift is exact, fused
    or not, and y = fl(CONST_VALUE * scale + shift) == CONST_BETA to the bit (0 without beta).
    offset: every channel is offset + N(0, 1) (|mean| >> std: why the statistics kernels subtract a pivot).
    affine = 0: gamma and beta are NULL.  running = 0: no running statistics (and no num_batches_tracked) in training.
    world: ranks of the synchronised protocol; the batch is world * N images."""

    def __init__(self, name, layout, N, C, P, act, plan, feature, accumulate=0, affine=1, running=1, const=0, offset=0.0, world=1):
        self.name, self.layout, self.N, self.C, self.P, self.act = name, layout, N, C, P, act
        self.plan, self.feature = plan, feature
        self.accumulate, self.affine, self.running, self.const = bool(accumulate), bool(affine), bool(running), bool(const)
        self.offset, self.world = float(offset), world
        assert layout in ('f32', 'b8') and (act in (0, 1) or layout == 'f32') and not (const and offset) and not (const and C < 2)

    @property
    def b8(self):
        return self.layout == 'b8'

    @property
    def mode(self):
        """How a thread walks its elements: 'vec4' (four consecutive floats per step), 'scalar' (one), 'b8' (one unit)."""
        return 'b8' if self.b8 else ('vec4' if self.P % 4 == 0 else 'scalar')

    def __repr__(self):
        return self.name


C_ = Case
# name, layout, N, C, P, act, (nsplit, nchunk, empty of nsplit, empty of nchunk, path), what it is there for, flags
ROWS = [
    C_('f32 1x1x1', 'f32', 1, 1, 1, 0, (1, 1, 0, 0, 'scalar'), 'n = 1: the unbiased variance is the biased one'),
    C_('f32 2x3x1', 'f32', 2, 3, 1, 1, (1, 1, 0, 0, 'scalar'), 'scalar walk, P = 1', affine=0),
    C_('f32 3x5x3', 'f32', 3, 5, 3, 2, (1, 1, 0, 0, 'scalar'), 'scalar walk, P < 4', const=1),
    C_('f32 7x1x63', 'f32', 7, 1, 63, 0, (1, 1, 0, 0, 'scalar'), 'scalar walk, C = 1', running=0, world=2),
    C_('f32 5x3x1023', 'f32', 5, 3, 1023, 1, (1, 1, 0, 0, 'scalar'), 'scalar walk, 20 steps per thread', offset=1e3),
    C_('f32 4x8x12', 'f32', 4, 8, 12, 2, (1, 1, 0, 0, 'div'), 'float4 walk, P/4 = 3: division path', accumulate=1),
    C_('f32 6x5x20', 'f32', 6, 5, 20, 1, (1, 1, 0, 0, 'div'), 'float4 walk, P/4 = 5: division path', const=1, world=3),
    C_('f32 9x16x1024', 'f32', 9, 16, 1024, 0, (1, 1, 0, 0, 'shift'), 'shift path, one part', affine=0, running=0),
    C_('f32 9x2x4096', 'f32', 9, 2, 4096, 1, (4, 2, 1, 0, 'shift'), 'nsplit 4 with 1 empty part, small enough to be a fine row'),
    C_('f32 37x32x1024', 'f32', 37, 32, 1024, 1, (4, 2, 0, 0, 'shift'), 'nsplit 4, nchunk 2, ragged last part', accumulate=1),
    C_('f32 49x8x1024', 'f32', 49, 8, 1024, 2, (6, 3, 0, 0, 'shift'), 'nsplit 6, nchunk 3', world=2),
    C_('f32 23x40x1028', 'f32', 23, 40, 1028, 1, (2, 1, 0, 0, 'div'), 'nsplit 2, nchunk 1, division path across parts', offset=1e3),
    C_('f32 300x3x256', 'f32', 300, 3, 256, 0, (9, 4, 0, 0, 'shift'), 'nsplit 9, nchunk 4', const=1, accumulate=1),
    C_('f32 130x2x4096', 'f32', 130, 2, 4096, 1, (64, 32, 20, 6, 'shift'), 'nsplit at the cap with empty parts'),
    C_('b8 1x1x1', 'b8', 1, 1, 1, 0, (1, 1, 0, 0, 'shift'), 'n = 1, seven padding channels'),
    C_('b8 2x3x1', 'b8', 2, 3, 1, 1, (1, 1, 0, 0, 'shift'), 'five padding channels, HW = 1', affine=0),
    C_('b8 3x5x3', 'b8', 3, 5, 3, 1, (1, 1, 0, 0, 'div'), 'three padding channels, HW = 3', const=1),
    C_('b8 4x13x12', 'b8', 4, 13, 12, 0, (1, 1, 0, 0, 'div'), 'second block with three padding channels', running=0, world=2),
    C_('b8 5x20x64', 'b8', 5, 20, 64, 1, (1, 1, 0, 0, 'shift'), 'third block with four padding channels', accumulate=1),
    C_('b8 37x32x256', 'b8', 37, 32, 256, 1, (4, 2, 0, 0, 'shift'), 'nsplit 4, nchunk 2', world=3),
    C_('b8 49x3x1024', 'b8', 49, 3, 1024, 0, (24, 12, 7, 2, 'shift'), 'nsplit 24 with 7 empty, nchunk 12 with 2 empty', offset=1e3),
    C_('b8 98x9x256', 'b8', 98, 9, 256, 1, (12, 6, 1, 0, 'shift'), 'nsplit 12 with 1 empty, second block with 7 padding channels',
       accumulate=1, const=1),
    C_('b8 130x40x100', 'b8', 130, 40, 100, 1, (6, 3, 0, 0, 'div'), 'HW not a power of two, across parts', affine=0),
    C_('b8 530x5x2050', 'b8', 530, 5, 2050, 1, (512, 265, 247, 0, 'div'), 'nsplit at the cap with empty parts'),
]
CASES = {c.name: c for c in ROWS}
assert len(CASES) == len(ROWS)
# the exact-mask rows: C >= 64 (every lane of a wave owns a channel of the finalize / fold kernels), data on a grid
MASK_ROWS = [C_('mask f32 relu', 'f32', 4, 64, 36, 1, (1, 1, 0, 0, 'div'), 'exact mask'),
             C_('mask f32 leaky', 'f32', 4, 64, 36, 2, (1, 1, 0, 0, 'div'), 'exact mask'),
             C_('mask b8 relu', 'b8', 4, 64, 36, 1, (1, 1, 0, 0, 'div'), 'exact mask')]


# ---------------------------------------------------------------------------------------------- plan and summation depth
def image_range(N, parts, j):
    """common.h image_range(), mirrored for the references; test_bn_plans_host.py holds it to jvae_image_range."""
    per = -(-N // parts)
    nb = min(j * per, N)
    return nb, max(min(j * per + per, N), nb)


def depth(case, parts=None):
    """Depth D of the fp32 summation tree behind one published sum: the additions one element can pass through.
    A 256-thread block owns an image part of at most per = ceil(N / nsplit) images.  fp32: thread t meets the float4 units
    t, t + 256, ... of the part's per * P / 4 and adds their four floats in sequence (4 * ceil(units / 256) additions); with
    P % 4 != 0 it meets single floats (ceil(per * P / 256)).  bf16: it meets the part's per * HW units and adds one value per
    channel and unit (ceil(per * HW / 256)).  Then the xor butterfly of the wave (6) and the four wave sums (2: (w0 + w2) + (w1 +
    w3) in block_sum, (w0 + w1) + (w2 + w3) in block_sum8).  The parts are folded in fp64 (nsplit * 2^-53, which the exact first
    addition onto 0 more than pays for) and rounded to fp32 once: that rounding is counted in c, not here."""
    per = -(-case.N // (parts or case.plan[0]))
    if case.mode == 'vec4':
        seq = 4 * -(-(per * (case.P // 4)) // 256)
    else:
        seq = -(-(per * case.P) // 256)
    return seq + 6 + 2


# roundings that form one term and publish the sum (c of the sums bound), counted on the term's own magnitude:
#   sum d       d = fl(x - pivot): 1; the fold's rounding to fp32: 1
#   sum d^2     d enters squared: 2; the product (where it is not fused): 1; the fold: 1
#   sum g       g = dy, or fl(slope * dy) under a leaky mask: 1; the fold: 1
#   sum g xhat  g: 1; xhat = fl(fl(x - mean) * invstd): 2; the product: 1; the fold: 1
C_SUM = {'d': 2, 'd2': 4, 'g': 2, 'gx': 5}


def sum_excess(got, ref, A, D, c):
    """max over channels of |got - ref| / ((D + c) U A), A = sum |term|: <= 1 is inside the bound; A = 0 must be exact.

    The bound: every summation tree of depth D has |fl(sum) - sum| <= gamma_D * sum |t_i| = D U sum |t_i| to first order
    (Higham, Accuracy and Stability, 4.2: each term carries at most D factors (1 + delta)), and a term that is itself formed
    with c roundings carries c more.  D is depth() - what the kernel does - not the element count of the part: the any-order
    bound K U A with K = elements would be a thousand times wider and hide a dropped element."""
    e = channel_excess(got, ref, A, D, c)
    return float(e.max()) if e.numel() else 0.0


def channel_excess(got, ref, A, D, c):
    """sum_excess per channel (inf where A = 0 and the sum is not exact)."""
    got, ref, A = (torch.as_tensor(t).detach().double().cpu() for t in (got, ref, A))
    bound = (D + c) * U * A
    diff = (got - ref).abs()
    return torch.where(bound > 0, diff / bound.clamp_min(1e-300), torch.where(diff > 0, torch.full_like(diff, math.inf), diff))


def ulp_excess(got, ref):
    """max |got - ref| / (2^-23 |ref|): one fp32 ulp, the bound of test_0_ops_gpu.py::test_batchnorm_folds_external_partials.
    Its argument: mean, invstd and the unbiased variance are computed in fp64 from the fp32 sums and rounded once (2^-24
    relative); scale = fl(gamma * invstd) adds one more rounding.  It does NOT hold for shift unless |beta| dominates
    |mean * scale|, nor for the blend with non-zero running statistics: those two have their own bounds below."""
    got, ref = (torch.as_tensor(t).detach().double().cpu() for t in (got, ref))
    den = 2.0 ** -23 * ref.abs()
    diff = (got - ref).abs()
    if bool(((den == 0) & (diff > 0)).any()):
        return math.inf
    return float((diff / den.clamp_min(1e-300)).max()) if diff.numel() else 0.0


def bound_excess(got, ref, A, c):
    """max |got - ref| / (c U A) over a per-channel vector."""
    return sum_excess(got, ref, A, 0, c)


# ---------------------------------------------------------------------------------------------- data
def _scales(Cn, g, spread):
    """Per-channel scale e^z as conv_cases.wide: the smallest channel comes last and is e^-4 below the rest."""
    z = spread * torch.randn(Cn, generator=g)
    if Cn > 1:
        j = int(z.argmin())
        z[[j, -1]] = z[[-1, j]]
        z[-1] -= 4.0
    return torch.exp(z)


def make_data(case):
    """fp32 operands on the CPU, x and dy as (world * N, C, P); bf16 rows already rounded to bf16."""
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    B, Cn, P = case.world * case.N, case.C, case.P
    if case.offset:
        sd = torch.ones(Cn)
        mu = case.offset + torch.randn(Cn, generator=g)
    else:
        sd = _scales(Cn, g, 1.0)
        mu = sd * torch.randn(Cn, generator=g)
    x = mu.view(1, Cn, 1) + sd.view(1, Cn, 1) * torch.randn(B, Cn, P, generator=g)
    dy = _scales(Cn, g, 1.0).view(1, Cn, 1) * torch.randn(B, Cn, P, generator=g)
    gamma = torch.rand(Cn, generator=g) + 0.5
    beta = torch.randn(Cn, generator=g)
    pivot = mu + 0.5 * sd * torch.randn(Cn, generator=g)
    d = dict(rm0=mu + sd * torch.randn(Cn, generator=g), rv0=(torch.rand(Cn, generator=g) + 0.5) * sd * sd,
             dg0=torch.randn(Cn, generator=g), db0=torch.randn(Cn, generator=g))
    if case.const:
        x[:, 0] = CONST_VALUE
        beta[0] = CONST_BETA
    if case.b8:
        x, dy = rbf(x), rbf(dy)
    d.update(x=x.contiguous(), dy=dy.contiguous(), gamma=gamma if case.affine else None, beta=beta if case.affine else None,
             pivot=pivot)
    return d


def to_b8(x):
    """(N, C, P) fp32 (bf16 values) -> B8 (N, ceil(C/8), P, 1, 8) bf16, padding channels 0."""
    N, Cn, P = x.shape
    CB = (Cn + 7) // 8
    t = torch.zeros(N, CB * 8, P, dtype=x.dtype)
    t[:, :Cn] = x
    return t.view(N, CB, 8, P).permute(0, 1, 3, 2).contiguous().view(N, CB, P, 1, 8).to(torch.bfloat16)


def from_b8(t, Cn):
    """B8 -> ((N, C, P) fp32, (N, padding channels, P) fp32)."""
    N, CB, P = t.shape[:3]
    f = t.detach().float().cpu().view(N, CB, P, 8).permute(0, 1, 3, 2).reshape(N, CB * 8, P)
    return f[:, :Cn], f[:, Cn:]


# ---------------------------------------------------------------------------------------------- fp64 references
def _v(t):
    return t.double().view(1, -1, 1)


def ones_or(t, Cn, fill):
    return torch.full((Cn,), fill, dtype=torch.float64) if t is None else t.double()


def act64(t, act):
    return t if act == 0 else (torch.relu(t) if act == 1 else torch.where(t > 0, t, SLOPE * t))


def fwd_sums64(x, pivot):
    """-> (sums (C, 2), A (C, 2)) of d = x - pivot in fp64 (the difference of two fp32 values is exact there)."""
    d = x.double() - _v(pivot)
    return torch.stack([d.sum((0, 2)), (d * d).sum((0, 2))], 1), torch.stack([d.abs().sum((0, 2)), (d * d).sum((0, 2))], 1)


def moments64(s, n, pv):
    """bn_moments() in fp64 from (C, 2) sums (the kernel's own fp32 sums, widened): -> mean, var, invstd, unbiased var."""
    s = s.double()
    dm = s[:, 0] / n
    var = (s[:, 1] / n - dm * dm).clamp_min(0.)
    return pv.double() + dm, var, 1. / torch.sqrt(var + EPS), var * n / (n - 1.) if n > 1 else var


def blend64(r0, new):
    """Running statistic after one step and the magnitude its bound is relative to.  Bound 3 U A: the kernel computes
    fl(fl(fl(1 - m) * r0) + fl(m * new)): on |(1 - m) r0| the rounding of 1 - m and of the product (2), on |m new| the rounding
    of new to fp32 and of the product (2), and the final addition rounds relative to the result <= A (1): at most 3 U A with
    A = |(1 - m) r0| + |m new|, fused or not."""
    a, b = (1. - MOMENTUM) * r0.double(), MOMENTUM * new.double()
    return a + b, a.abs() + b.abs()


def coef64(gamma, beta, mean, invstd):
    """scale, shift from PUBLISHED fp32 mean / invstd and the magnitude of shift's bound.  scale = fl(gamma * invstd): one
    rounding (ulp_excess).  shift = fl(beta - fl(mean * scale)): the rounding of scale and of the product on |mean scale| (2),
    the subtraction on |shift| <= A (1): 3 U A with A = |beta| + |mean scale|."""
    sc = gamma * invstd.double()
    return sc, beta - mean.double() * sc, beta.abs() + (mean.double() * sc).abs()


def y64(x, gamma, beta, mean, invstd, act):
    """y from published mean / invstd, and A = |x sc| + |mean sc| + |beta|.  Bound c U A with c = 4 (5 under leaky ReLU): the
    kernel computes fl(x sc' + sh') with sc' = sc (1 + d1), sh' = fl(beta - mean sc' (1 + d2)): d1 on |x sc| and |mean sc|, d2 on
    |mean sc|, the rounding of sh' on |beta| + |mean sc|, the final rounding on all three - |x sc| 2, |mean sc| 4, |beta| 2.
    The activation is 1-Lipschitz, so it passes the error on; the leaky product adds one rounding."""
    sc = _v(gamma) * _v(invstd)
    ms = _v(mean) * sc
    t = x.double() * sc + (_v(beta) - ms)
    return act64(t, act), (x.double() * sc).abs() + ms.abs() + _v(beta).abs()


def y_eval64(x, scale, shift, act):
    """Eval-mode y from the fp32 scale / shift an eval-mode finalize PUBLISHED (rsqrtf has no accuracy to derive from; the
    apply stage is fl(fma(x, scale, shift))): c = 1 (2 under leaky ReLU) on A = |x scale| + |shift|."""
    t = x.double() * _v(scale) + _v(shift)
    return act64(t, act), (x.double() * _v(scale)).abs() + _v(shift).abs()


def masked(dy, mask, act):
    """g = dy where the forward's pre-activation was > 0 (mask: the KERNEL'S y > 0), slope * dy (leaky) or 0 (ReLU) elsewhere."""
    if act == 0:
        return dy.double()
    return torch.where(mask, dy.double(), (SLOPE if act == 2 else 0.) * dy.double())


def bwd_sums64(x, g, mean, invstd):
    """-> (sums (C, 2), A (C, 2)) of (g, g xhat), xhat = (x - mean) invstd in fp64 from the fp32 mean / invstd handed in."""
    xh = (x.double() - _v(mean)) * _v(invstd)
    return torch.stack([g.sum((0, 2)), (g * xh).sum((0, 2))], 1), torch.stack([g.abs().sum((0, 2)), (g * xh).abs().sum((0, 2))], 1)


C_DX = 8


def dx64(x, g, gamma, mean, invstd, m1, m2):
    """dx = k (g - m1 - xhat m2), k = gamma invstd, with m1 = fl32(dbeta / M), m2 = fl32(dgamma / M) from the sums the kernel
    published (or was handed), and A = |k| (|g| + |m1| + |xhat m2|).  Bound C_DX U A, C_DX = 8: the kernel's m is the fp64 sum
    over M rounded once, ours the published fp32 sum over M rounded again, so they differ by 2 U; per term -
      |g|:       k 1, leaky product 1, g - m1 1, the second subtraction 1, the product with k 1                       = 5
      |m1|:      k 1, m1 2, g - m1 1, the second subtraction 1, the product with k 1                                  = 6
      |xhat m2|: k 1, x - mean 1, times invstd 1, m2 2, the product 1, the subtraction 1, the product with k 1       = 8."""
    k = _v(gamma) * _v(invstd)
    xh = (x.double() - _v(mean)) * _v(invstd)
    a, b = _v(m1), xh * _v(m2)
    return k * (g - a - b), k.abs() * (g.abs() + a.abs() + b.abs())


def means32(sums, M):
    """(fl32(s1 / M), fl32(s2 / M)) from (C, 2) fp32 sums, as the apply kernels form them."""
    m = (sums.double() / M).float()
    return m[:, 0], m[:, 1]
