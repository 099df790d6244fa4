"""The dense-product case table shared by tests/test_gemm_routes.py (CPU: which variant of csrc/gemm.hip every case reaches, how
its K is sliced) and tests/test_24_gemm_sweep_gpu.py (GPU: every case against fp64, with canaries around every operand), with the
data recipes, the fp64 reference and the two exact probes both use.  A plain module, not a conftest.

A case names the extents, the element strides of A, B and C written out, the offset of each operand inside its buffer, the
epilogue (bias mode, flags), the K slicing asked for (splitk: atomics; want: slices stored side by side), the split-bf16 switch -
and the variant gemm_plan() is EXPECTED to choose with the number of K slices it makes, as jvae_gemm_route reports them today.  The
rows were written from gemm_plan() as it stands: a change of the plan that moves a case to another variant fails
test_gemm_routes.py on a CPU instead of passing on another kernel.

Variant names (jvae_gemm_variant_name): TILE64 / TILE128 the fp32 MFMA tile kernel, X3 the split-bf16 kernel with D1 / D3 K steps
in flight; AK: sAk == 1, else AM; BN: sBn == 1, else BK.  Layout letters below: A 'n' = (M, K) row-major (AK), 't' = (K, M)
row-major (AM); B 'n' = (K, N) row-major (BN), 't' = (N, K) row-major (BK).

Every operand lives inside a larger buffer whose other elements are NaN: OFF elements in front (4 keeps the 16-byte alignment,
5 breaks it), the gaps a leading or batch stride leaves, TAIL elements behind."""
import math
import zlib

import numpy as np
import torch

from conv_cases import U, elementwise_excess          # noqa: F401  (the measure of the sweep)

OFF, TAIL = 4, 7
VARIANTS = [f'TILE{t}_{a}_{b}' for t in (64, 128) for a in ('AM', 'AK') for b in ('BK', 'BN')] + \
           [f'X3_{a}_{b}_D{d}' for a in ('AM', 'AK') for b in ('BK', 'BN') for d in (1, 3)]          # index = variant number
LAYOUTS = ('nn', 'nt', 'tn', 'tt')


def vname(kind, lay, depth=None):
    a, b = ('AK' if lay[0] == 'n' else 'AM'), ('BN' if lay[1] == 'n' else 'BK')
    return f'{kind}_{a}_{b}' + (f'_D{depth}' if depth else '')


def up4(v):
    return (v + 3) // 4 * 4


class Case:
    def __init__(self, name, M, N, K, lay='nn', batch=1, expect=None, slices=1, tags=(), lda=None, ldb=None, ldc=None, sA=None,
                 sB=None, sC=None, sAb=None, sBb=None, sCb=None, offA=OFF, offB=OFF, offC=OFF, ct=False, bias=0, flags=0, splitk=1,
                 want=0, split=1):
        self.name, self.M, self.N, self.K, self.batch, self.lay = name, M, N, K, batch, lay
        # strides not written out (sA / sB / sC) come from the layout letter: the leading stride defaults to the extent, the batch
        # stride to the matrix rounded up to a multiple of 4 (one batch: 0, as the callers pass it)
        def batch_stride(given, matrix):
            if given is not None:
                return given
            return up4(matrix) if batch > 1 else 0
        if sA is None:
            lda = lda or (K if lay[0] == 'n' else M)
            sA = (lda, 1, batch_stride(sAb, M * lda)) if lay[0] == 'n' else (1, lda, batch_stride(sAb, K * lda))
        if sB is None:
            ldb = ldb or (N if lay[1] == 'n' else K)
            sB = (ldb, 1, batch_stride(sBb, K * ldb)) if lay[1] == 'n' else (1, ldb, batch_stride(sBb, N * ldb))
        if sC is None:          # ct: C stored transposed (sCm = 1)
            ldc = ldc or (M if ct else N)
            sC = (1, ldc, batch_stride(sCb, N * ldc)) if ct else (ldc, 1, batch_stride(sCb, M * ldc))
        self.sA, self.sB, self.sC = tuple(sA), tuple(sB), tuple(sC)
        self.offA, self.offB, self.offC = offA, offB, offC
        self.bias, self.flags, self.splitk, self.want, self.split = bias, flags, splitk, want, split
        self.expect, self.slices, self.tags = expect, slices, tuple(tags)

    # the stored-slices form puts slice s at C + s * sCsplit: behind the last batch of the slice before
    @property
    def sCsplit(self):
        if not self.want:
            return 0
        span = max(self.sC[0] * (self.M - 1) + self.sC[1] * (self.N - 1) + self.sC[2] * (self.batch - 1) + 1, 1)
        return span + 3

    @property
    def x3(self):
        return self.expect.startswith('X3')

    @property
    def atomic(self):
        return not self.want and (self.slices > 1 or bool(self.flags & 4))

    @property
    def onto(self):          # the product is added to what C holds
        return not self.want and (bool(self.flags & 1) or self.atomic)

    @property
    def c0(self):            # ... and C holds values: an accumulating call, or the rows tagged for it; else a slicing caller's zeros
        return self.onto and (bool(self.flags & 1) or 'atomic_c0' in self.tags)

    @property
    def ordered(self):
        """Two launches give the same bits: always without atomics; with them while there are at most two addends per element
        (fp32 addition commutes, it does not associate) - two slices onto zeros, or one onto the values C holds."""
        return not self.atomic or self.slices + (1 if self.c0 else 0) <= 2

    def route(self, A=0x10000000, B=0x20000000, C=0x30000000, bias=0x40000000):
        """The plan of the case for operands at these (16-byte aligned) buffer addresses; the operands begin off* elements in."""
        from jvae_hip import ops
        return ops.gemm_route(self.M, self.N, self.K, A + 4 * self.offA, self.sA, B + 4 * self.offB, self.sB, C + 4 * self.offC,
                              self.sC, bias=bias if self.bias else None, bias_mode=self.bias, flags=self.flags, splitk=self.splitk,
                              batch=self.batch, want_splits=self.want, sCsplit=self.sCsplit)

    def __repr__(self):
        return self.name


C = Case
ROWS = []

# ---- all 16 variants.  128 x 128 tiles: tiles128 >= 512 with M, N > 64 - M = N = 130, batch 128 gives 2 * 2 * 128 = 512; batch 127 not
for lay in LAYOUTS:
    ROWS.append(C(f'tile128 b128 {lay}', 130, 130, 40, lay, batch=128, expect=vname('TILE128', lay), tags=('tile128',)))
ROWS.append(C('tile128 neighbour b127 nn', 130, 130, 40, 'nn', batch=127, expect='TILE64_AK_BN', tags=('tile128_neighbour',)))
# switch off: K >= 64 stays on the fp32 tile kernel, one per layout
for lay in LAYOUTS:
    ROWS.append(C(f'switch off K96 {lay}', 70, 66, 96, lay, split=0, expect=vname('TILE64', lay), tags=('switch_off',)))

# ---- the K pipeline of the DEPTH 3 variants (K step 32): K = 64, 96, 128, 160, 224 are 2, 3, 4, 5, 7 steps (remainders 2, 0, 1, 2, 1
# of the three-stage loop; 64: a slice shorter than the pipeline); 68 and 100 end in a partial step that is a multiple of 4; K = 64 as two
# slices: one step per slice under a three-step prologue.  M = 68, N = 72: 2 x 2 tiles, both ragged, both multiples of 4.
for lay in LAYOUTS:
    for K in (64, 96, 128, 160, 224):
        ROWS.append(C(f'deep K{K} {lay}', 68, 72, K, lay, expect=vname('X3', lay, 3), tags=('deep_steps',)))
    for K in (68, 100):
        ROWS.append(C(f'deep K{K} {lay}', 68, 72, K, lay, expect=vname('X3', lay, 3), tags=('deep_partial',)))
    ROWS.append(C(f'deep K64 splitk2 {lay}', 68, 72, 64, lay, splitk=2, slices=2, expect=vname('X3', lay, 3), tags=('deep_short_slice',)))

# ---- each condition that withdraws `deep` or the 16-byte loads, ONE at a time (the leading strides stay multiples of 4 where the
# condition under test is another one)
ROWS += [
    C('nodeep K70 nn', 68, 72, 70, 'nn', lda=72, expect='X3_AK_BN_D1', tags=('nodeep_k',)),
    C('nodeep K70 tt', 68, 72, 70, 'tt', ldb=72, expect='X3_AM_BK_D1', tags=('nodeep_k',)),
    C('nodeep A base+1 nn', 68, 72, 96, 'nn', offA=OFF + 1, expect='X3_AK_BN_D1', tags=('nodeep_base',)),
    C('nodeep B base+1 tt', 68, 72, 96, 'tt', offB=OFF + 1, expect='X3_AM_BK_D1', tags=('nodeep_base',)),
    C('nodeep A base+1 tn', 68, 72, 96, 'tn', offA=OFF + 1, expect='X3_AM_BN_D1', tags=('nodeep_base',)),
    C('nodeep lda K+1 nn', 68, 72, 96, 'nn', lda=97, expect='X3_AK_BN_D1', tags=('nodeep_ld',)),
    C('nodeep ldb K+1 nt', 68, 72, 96, 'nt', ldb=97, expect='X3_AK_BK_D1', tags=('nodeep_ld',)),
    C('nodeep M70 A along m tn', 70, 72, 96, 'tn', lda=72, expect='X3_AM_BN_D1', tags=('nodeep_m',)),
    C('nodeep N70 B along n nn', 68, 70, 96, 'nn', ldb=72, expect='X3_AK_BN_D1', tags=('nodeep_n',)),
    C('nodeep sAb%4 nn', 68, 72, 96, 'nn', batch=2, sAb=68 * 96 + 2, expect='X3_AK_BN_D1', tags=('nodeep_batch',)),
    C('nodeep sBb%4 tt', 68, 72, 96, 'tt', batch=2, sBb=72 * 96 + 1, expect='X3_AM_BK_D1', tags=('nodeep_batch',)),
    C('x3 boundary K63 nn', 68, 72, 63, 'nn', expect='TILE64_AK_BN', tags=('x3_boundary',)),
    C('x3 boundary K64 nn', 68, 72, 64, 'nn', expect='X3_AK_BN_D3', tags=('x3_boundary',)),
    C('x3 boundary K63 tn', 68, 72, 63, 'tn', expect='TILE64_AM_BN', tags=('x3_boundary',)),
]

# ---- K slicing
ROWS += [
    C('slices clamped K33 splitk4', 37, 75, 33, 'nn', splitk=4, slices=2, expect='TILE64_AK_BN', tags=('slice_clamp', 'atomic_c0')),
    C('slices ragged K160 splitk4 x3', 68, 72, 160, 'nt', splitk=4, slices=3, expect='X3_AK_BK_D3', tags=('slice_ragged', 'atomic_c0')),
    C('slices ragged K160 splitk4 tile', 68, 72, 160, 'tn', splitk=4, slices=3, split=0, expect='TILE64_AM_BN',
      tags=('slice_ragged', 'atomic_c0')),
    C('slices ragged K70 splitk2 D1', 65, 63, 70, 'nn', splitk=2, slices=2, expect='X3_AK_BN_D1', tags=('slice_ragged',)),
    C('flag4 one slice', 65, 63, 40, 'nt', flags=4, expect='TILE64_AK_BK', tags=('atomic_c0',)),
    C('stored K160 want4 x3', 68, 72, 160, 'nn', want=4, slices=3, expect='X3_AK_BN_D3', tags=('stored',)),
    C('stored K512 want4 wgrad form', 10, 130, 512, 'tn', want=4, slices=4, expect='X3_AM_BN_D1', tags=('stored',)),
    C('stored K40 want2 tile', 65, 63, 40, 'tt', want=2, slices=2, expect='TILE64_AM_BK', tags=('stored',)),
    C('stored K40 want1 tile b3', 65, 63, 40, 'nn', want=1, batch=3, slices=1, expect='TILE64_AK_BN', tags=('stored',)),
    C('stored tile128 shape stays 64', 130, 130, 40, 'nn', batch=128, want=1, slices=1, expect='TILE64_AK_BN', tags=('stored',)),
]

# ---- ragged and degenerate extents: M, N in {1, 63, 64, 65, 129} on both kernel families, K = 1, K = 0
# (an extent of 1 along the contiguous direction makes BOTH strides 1: the plan then reads the operand as AK / BN)
ROWS += [
    C('ragged 1x129 K40 nn', 1, 129, 40, 'nn', bias=1, expect='TILE64_AK_BN', tags=('ragged',)),
    C('ragged 63x65 K40 nt', 63, 65, 40, 'nt', bias=1, expect='TILE64_AK_BK', tags=('ragged',)),
    C('ragged 64x64 K40 tn', 64, 64, 40, 'tn', bias=1, expect='TILE64_AM_BN', tags=('ragged',)),
    C('ragged 65x63 K40 tt', 65, 63, 40, 'tt', bias=1, expect='TILE64_AM_BK', tags=('ragged',)),
    C('ragged 129x1 K40 nn', 129, 1, 40, 'nn', bias=1, expect='TILE64_AK_BN', tags=('ragged',)),
    C('ragged 1x129 K96 tn', 1, 129, 96, 'tn', bias=2, expect='X3_AK_BN_D1', tags=('ragged',)),          # lda = M = 1; ldb = 129
    C('ragged 63x65 K96 tt', 63, 65, 96, 'tt', bias=2, expect='X3_AM_BK_D1', tags=('ragged',)),
    C('ragged 64x64 K96 nn', 64, 64, 96, 'nn', bias=2, expect='X3_AK_BN_D3', tags=('ragged',)),
    C('ragged 65x63 K96 nt', 65, 63, 96, 'nt', bias=2, expect='X3_AK_BK_D3', tags=('ragged',)),
    C('ragged 129x1 K96 tn', 129, 1, 96, 'tn', bias=2, expect='X3_AM_BN_D1', tags=('ragged',)),
    C('ragged 129x129 K96 tn', 129, 129, 96, 'tn', lda=132, ldb=132, bias=1, expect='X3_AM_BN_D1', tags=('ragged',)),
]
ROWS += [
    C('K1 nn', 65, 63, 1, 'nn', bias=1, expect='TILE64_AK_BN', tags=('k1',)),
    C('K1 tt', 65, 63, 1, 'tt', bias=2, expect='TILE64_AM_BN', tags=('k1',)),          # ldb = K = 1: sBn = 1 too
    C('K1 tt ld4', 65, 63, 1, 'tt', lda=68, ldb=4, bias=2, expect='TILE64_AM_BK', tags=('k1',)),
    C('K0 bias', 65, 63, 0, 'nn', bias=1, expect='TILE64_AK_BN', tags=('k0',)),
    C('K0 bias relu', 65, 63, 0, 'nt', bias=2, flags=2, expect='TILE64_AK_BK', tags=('k0',)),
    C('K0 bias accumulate', 65, 63, 0, 'tn', bias=1, flags=1, expect='TILE64_AM_BN', tags=('k0',)),
]

# ---- tile counts of the XCD remap (x3 variants): fewer than 8, not multiples of 8, and gz > 1
ROWS += [
    C('xcd 2 tiles', 64, 128, 64, 'nn', expect='X3_AK_BN_D3', tags=('xcd',)),
    C('xcd 9 tiles', 192, 132, 64, 'nt', expect='X3_AK_BK_D3', tags=('xcd',)),
    C('xcd 13 tiles', 60, 13 * 64, 96, 'tn', expect='X3_AM_BN_D3', tags=('xcd',)),
    C('xcd 2x1x3 tiles', 68, 40, 64, 'tt', batch=3, expect='X3_AM_BK_D3', tags=('xcd', 'xcd_gz')),
    C('xcd 2x2x2x2 tiles sliced', 68, 72, 128, 'nn', batch=2, splitk=2, slices=2, expect='X3_AK_BN_D3', tags=('xcd', 'xcd_gz')),
]

# ---- epilogues, on both kernel families (K = 40: tile, K = 64: x3)
for K, kind, dp in ((40, 'TILE64', None), (64, 'X3', 3)):
    f = lambda lay: vname(kind, lay, dp)
    ROWS += [
        C(f'epi bias n K{K}', 68, 72, K, 'nt', bias=1, expect=f('nt'), tags=('bias_n',)),
        C(f'epi bias m K{K}', 68, 72, K, 'tn', bias=2, expect=f('tn'), tags=('bias_m',)),
        C(f'epi accumulate K{K}', 68, 72, K, 'nn', flags=1, expect=f('nn'), tags=('acc',)),
        C(f'epi relu K{K}', 68, 72, K, 'nt', bias=1, flags=2, expect=f('nt'), tags=('relu',)),
        C(f'epi accumulate relu K{K}', 68, 72, K, 'tt', bias=2, flags=3, expect=f('tt'), tags=('acc_relu',)),
        C(f'epi C transposed K{K}', 68, 72, K, 'nn', ct=True, bias=1, expect=f('nn'), tags=('c_transposed',)),
        C(f'epi ldc padded K{K}', 68, 72, K, 'nn', ldc=77, flags=1, expect=f('nn'), tags=('ldc',)),
        C(f'epi C batch stride K{K}', 68, 72, K, 'nt', batch=3, sCb=68 * 72 + 5, bias=2, expect=f('nt'), tags=('c_batch',)),
    ]

# ---- the callers' stride patterns at small sizes
R, I, O, S = 70, 800, 10, 4          # ops.linear forward, K slices as the batch (the model's K = 800 -> 4 slices of 200)
ROWS.append(C('linear sliced forward', R, O, I // S, batch=S, sA=(I, 1, I // S), sB=(1, I, I // S), sC=(O, 1, R * O),
              expect='X3_AK_BK_D3', tags=('linear_sliced',)))
R, I, O, S = 512, 20, 12, 4          # ops.linear weight gradient, row slices as the batch: A = gy (R, O) as (1, O, Rs * O)
ROWS.append(C('linear weight gradient row-sliced', O, I, R // S, batch=S, sA=(1, O, R // S * O), sB=(I, 1, R // S * I), sC=(I, 1, O * I),
              expect='X3_AM_BN_D3', tags=('wgrad_rows',)))
Ni, Cs, Ps, Kd = 5, 72, 4, 96        # csrc/conv_generic.hip: images, small-side channels, folded positions, unfolded K
ROWS += [
    # head forward: shared weights (batch stride 0), output (n, cs, q) written with sCn = Ps, batch (q) stride 1
    C('conv generic head forward', Ni, Cs, Kd, batch=Ps, sA=(Kd, 1, Ni * Kd), sB=(1, Kd, 0), sC=(Cs * Ps, Ps, 1), bias=1,
      expect='X3_AK_BK_D3', tags=('conv_shared', 'conv_scn')),
    # forward over images: the weights are the shared A, bias per m
    C('conv generic forward', Cs, Ps, Kd, batch=Ni, sA=(Kd, 1, 0), sB=(Ps, 1, Kd * Ps), sC=(Ps, 1, Cs * Ps), bias=2,
      expect='X3_AK_BN_D3', tags=('conv_shared',)),
    # head dgrad: A = ys (n, cs, q) read as (m = n, k = cs, batch = q): NEITHER stride is 1
    C('conv generic head dgrad', Ni, Kd, Cs, batch=Ps, sA=(Cs * Ps, Ps, 1), sB=(Kd, 1, 0), sC=(Kd, 1, Ni * Kd),
      expect='X3_AM_BN_D1', tags=('conv_nostride1', 'conv_shared')),
    C('conv generic head dgrad tile', Ni, Kd, 40, batch=Ps, sA=(40 * Ps, Ps, 1), sB=(Kd, 1, 0), sC=(Kd, 1, Ni * Kd),
      expect='TILE64_AM_BN', tags=('conv_nostride1', 'conv_shared')),
    # per-position weight gradient: A = ys + q as (m = cs, k = n), accumulating
    C('conv generic wgrad per position', Cs, Kd, 70, sA=(Ps, Cs * Ps, 0), sB=(Kd, 1, 0), sC=(Kd, 1, 0), flags=1,
      expect='X3_AM_BN_D1', tags=('conv_nostride1',)),
]

CASES = {c.name: c for c in ROWS}
assert len(CASES) == len(ROWS)
TAGS = ('tile128', 'tile128_neighbour', 'switch_off', 'deep_steps', 'deep_partial', 'deep_short_slice', 'nodeep_k', 'nodeep_base',
        'nodeep_ld', 'nodeep_m', 'nodeep_n', 'nodeep_batch', 'x3_boundary', 'slice_clamp', 'slice_ragged', 'stored', 'atomic_c0',
        'ragged', 'k1', 'k0', 'xcd', 'xcd_gz', 'bias_n', 'bias_m', 'acc', 'relu', 'acc_relu', 'c_transposed', 'ldc', 'c_batch',
        'linear_sliced', 'wgrad_rows', 'conv_shared', 'conv_nostride1', 'conv_scn')


# ---------------------------------------------------------------------------------------------- placement
def index(shape, strides, off):
    """Element index inside the buffer of every entry of a logical tensor with these strides (int64, shape `shape`)."""
    idx = torch.full(tuple(shape), off, dtype=torch.int64)
    for d, (n, s) in enumerate(zip(shape, strides)):
        view = [1] * len(shape)
        view[d] = n
        idx = idx + (torch.arange(n, dtype=torch.int64) * s).view(view)
    return idx


def place(vals, strides, off):
    """A NaN buffer with vals at off + sum(index * stride), TAIL NaN elements behind the last one.  A stride-0 axis holds one
    entry (vals has extent 1 there).  The placement must not fold two entries onto one element."""
    idx = index(vals.shape, strides, off)
    n = (int(idx.max()) + 1 if idx.numel() else off) + TAIL
    assert idx.unique().numel() == idx.numel(), 'strides fold two entries onto one element'
    buf = torch.full((n,), math.nan, dtype=vals.dtype)
    buf[idx.reshape(-1)] = vals.reshape(-1)
    return buf, idx


def operand_shapes(c):
    """Logical shapes (batch, rows, cols) of A (M, K) and B (K, N): batch extent 1 for a shared operand."""
    ba = 1 if c.sA[2] == 0 else c.batch
    bb = 1 if c.sB[2] == 0 else c.batch
    return (ba, c.M, c.K), (bb, c.K, c.N)


def slice_bounds(c, kchunk):
    return [(s * kchunk, min(c.K, (s + 1) * kchunk)) for s in range(c.slices)]


def make_data(c):
    """fp32 operands: the rows of A and the columns of B scaled by exp(2 randn) (the wide-range recipe of the conv accuracy
    tests), a bias and a base value C0 on the scale of the element they are added to."""
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    sa, sb = operand_shapes(c)
    ra, cb = torch.exp(2.0 * torch.randn(sa[0], c.M, 1, generator=g)), torch.exp(2.0 * torch.randn(sb[0], 1, c.N, generator=g))
    A = torch.randn(sa, generator=g) * ra
    B = torch.randn(sb, generator=g) * cb
    scale = (ra * cb).expand(c.batch, c.M, c.N) * math.sqrt(c.K + 1)          # of an output element
    bias = None
    if c.bias == 1:
        bias = torch.randn(c.N, generator=g) * scale[0, 0, :]
    elif c.bias == 2:
        bias = torch.randn(c.M, generator=g) * scale[0, :, 0]
    C0 = torch.randn(c.batch, c.M, c.N, generator=g) * scale
    if not c.c0:
        C0 = torch.zeros_like(C0)
    return dict(A=A, B=B, bias=bias, C0=C0)


def reference(c, d, kchunk):
    """fp64 result and the absolute-value sum A it is measured against, as (batch, S, M, N): S = the stored slices (want), else 1."""
    A, B = d['A'].double(), d['B'].double()
    parts = slice_bounds(c, kchunk) if c.want else [(0, c.K)]
    ref = torch.stack([torch.matmul(A[:, :, lo:hi], B[:, lo:hi, :]).expand(c.batch, c.M, c.N) for lo, hi in parts], 1)
    mag = torch.stack([torch.matmul(A[:, :, lo:hi].abs(), B[:, lo:hi, :].abs()).expand(c.batch, c.M, c.N) for lo, hi in parts], 1)
    if c.bias and not c.want:
        b = d['bias'].double().view((1, 1, 1, c.N) if c.bias == 1 else (1, 1, c.M, 1))
        ref, mag = ref + b, mag + b.abs()
    if c.onto:
        ref, mag = ref + d['C0'].double().unsqueeze(1), mag + d['C0'].double().abs().unsqueeze(1)
    if c.flags & 2 and not c.want:
        ref = torch.relu(ref)
    return ref, mag, [hi - lo for lo, hi in parts]


def bound_c(c):
    """The constant of elementwise_excess's (K + c) U A, derived: 1 the bias add, 3 the three dropped cross products of a
    split-bf16 variant, 1 the add onto an existing C, one rounding per atomic add of a slice."""
    return (1 if c.bias and not c.want else 0) + (3 if c.x3 else 0) + (1 if c.flags & 1 and not c.want else 0) + \
        (c.slices if c.atomic else 0)


# ---------------------------------------------------------------------------------------------- the exact probe of the six products
KEPT = ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0))          # (plane of A, plane of B) of the six products gemm_x3_body keeps
EPS = 2.0 ** -10


def x3_split(x):
    """numpy restatement of x3_split (csrc/conv_x3.h): h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), round to nearest even;
    the planes as fp64."""
    bf = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()
    x = np.asarray(x, dtype=np.float32)
    h = bf(x)
    r = (x - h).astype(np.float32)
    m = bf(r)
    r = (r - m).astype(np.float32)
    return [p.astype(np.float64) for p in (h, m, bf(r))]


def six_products(A, B, kept=KEPT):
    """sum of the kept cross products of the planes of A (..., M, K) and B (..., K, N) in fp64."""
    a, b = x3_split(A), x3_split(B)
    return sum(np.matmul(a[i], b[j]) for i, j in kept)


def digit_values(shape, rng):
    """+-(d1 + d2 2^-10 + d3 2^-20), d in {1, 2}: three bf16 digits 10 bits apart, so that the RNE split returns exactly them."""
    d = rng.integers(1, 3, size=(3,) + tuple(shape)).astype(np.float64)
    v = rng.choice([-1.0, 1.0], size=shape) * (d[0] + d[1] * EPS + d[2] * EPS * EPS)
    assert np.all(v.astype(np.float32) == v)
    return v, d


def probe_operands(M, N, K, sparse, seed):
    """(A (M, K), B (K, N)) fp32 for the exact probe: the `sparse` operand ('A' / 'B') has exactly two non-zeros per row of A /
    per column of B and every k is the non-zero of some row (column); the other operand is dense."""
    rng = np.random.default_rng(seed)
    rows = M if sparse == 'A' else N
    assert 2 * rows >= K and K >= 2
    # two non-zeros per row: the k of permutations of [0, K) dealt out in order, so that every k is met before any repeats
    ks = np.concatenate([rng.permutation(K) for _ in range((2 * rows + K - 1) // K)])[:2 * rows].reshape(rows, 2)
    for r in np.nonzero(ks[:, 0] == ks[:, 1])[0]:          # (a pair that straddles two permutations can repeat a k)
        ks[r, 1] = (ks[r, 1] + 1) % K
    mask = np.zeros((rows, K), bool)
    mask[np.arange(rows)[:, None], ks] = True
    assert np.all(mask.sum(1) == 2) and mask.any(0).all(), 'a k no row of the sparse operand meets'
    A, _ = digit_values((M, K), rng)
    B, _ = digit_values((K, N), rng)
    if sparse == 'A':
        A = np.where(mask, A, 0.0)
    else:
        B = np.where(mask.T, B, 0.0)
    return A.astype(np.float32), B.astype(np.float32)


def probe_expected(A, B):
    """The six-term sum of the probe operands, asserted exactly representable in fp32 at every partial sum: all terms are
    multiples of 2^-20 and the sum of their magnitudes stays below 2^4, so any partial sum in any order has at most 24 bits."""
    a, b = x3_split(A), x3_split(B)
    y = sum(np.matmul(a[i], b[j]) for i, j in KEPT)
    tot = sum(np.matmul(np.abs(a[i]), np.abs(b[j])) for i, j in KEPT)
    for i, j in KEPT:
        t = np.matmul(a[i], b[j]) * 2.0 ** 20
        assert np.all(t == np.round(t))
    assert tot.max() < 16.0 and np.all(y.astype(np.float32).astype(np.float64) == y)
    return y


# ---------------------------------------------------------------------------------------------- the one-hot probe of the fp32 kernel
def onehot_operands(M, N, K, hot, seed):
    """`hot` = 'A': one non-zero per row of A at k = m % K (M >= K: every k, the first and last of every slice included), B dense;
    'B': one per column of B at k = n % K, A dense.  All values random with full 24-bit significands."""
    g = torch.Generator().manual_seed(seed)
    A, B = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g)
    if hot == 'A':
        assert M >= K
        keep = torch.zeros(M, K, dtype=torch.bool)
        keep[torch.arange(M), torch.arange(M) % K] = True
        A = torch.where(keep, A, torch.zeros(()))
    else:
        assert N >= K
        keep = torch.zeros(K, N, dtype=torch.bool)
        keep[torch.arange(N) % K, torch.arange(N)] = True
        B = torch.where(keep, B, torch.zeros(()))
    return A, B


def ulp_distance(a, b):
    """Distance of two finite fp32 tensors in units in the last place (the integer order of the fp32 encoding)."""
    def key(t):
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7fffffff), i)
    return (key(a) - key(b)).abs()
