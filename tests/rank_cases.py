"""The case table of the rank kernels - csrc/roc_sort.h (the padded bitonic sort and the order-preserving key) under csrc/roc.hip,
csrc/prc.hip, csrc/scod.hip and the split / confusion of csrc/misclass.hip - shared by tests/test_rank_cases_host.py (CPU: the
table covers the regimes it names, every discriminating row discriminates, the restatements agree with a second, naive
definition, the closed forms of the long rows are the restatements) and tests/test_40_rank_sweep_gpu.py (GPU: every row through
every user it feeds).  A plain module without a GPU import, in the style of tests/conv_cases.py and tests/tail_cases.py.

The references are the restatements the other tests pin to the reference's goldens, imported, not copied: roc_restatement,
roc_restatement_quantile, pr_restatement, scod_restatement, mdr_restatement, with their bounds auc_bound, pr_bounds, area_bound.

A row names a value kind, its sizes, a seed and the users it feeds:
    roc0 one-sided ROC    roc1 around-mean ROC    rocq quantile ROC at FACTORS    pr PR figures (mode 0, and mode 1 with roc1)
    scod SCOD curves of the `ins` vector under the label pattern of its length    mdr split / confusion / rates of the same
    vector under the mask of its length

Sizes.  A row is padded to max(2048, next power of two) keys; the network runs log2(padded / 2048) merge stages above the tile.
The tie-free rows 2, 3, 2047, 2048, 2049, 4096, 4097, 8193, 16385 give no stage, then one (2049, 4096), two, three and four, on
either side of each power of two; the pairs (2049, 1), (1, 8193), (4097, 2047) pad their two sides differently.

Value kinds (fp32).  tiefree / sorted_asc / sorted_desc / organ_pipe: distinct multiples of 2^-10 below 16.  signed_zeros:
draws from {-1, -0., +0., 1}.  denormals: +- the first eight denormals, both zeros, +-FLT_MIN.  extremes: +-FLT_MAX and +-inf
among normal draws.  adjacent_bits: the 3000 bit patterns around +0. (1500 on either side: the key's sign change) and the 3000
around 1., shuffled.  all_equal: one value.  straddle: two values, the lower one `arg` times, so that its group ends at that
sorted position.

Around-mean rows stay on the project's grid, multiples of 2^-10 below 16: the fp64 sum of such scores is exact in any order, so
the centre does not depend on how the device sums.  tiefree, the sorted kinds, signed_zeros, all_equal and straddle are on it;
denormals, extremes and adjacent_bits are not and feed no roc1 (ON_GRID below; the host test asserts it).  extremes feeds only
the one-sided ROC, the PR figures and SCOD; its around-mean behaviour is a status word, asserted by the device test."""
import math
from collections import namedtuple

import numpy as np

from test_mdr_restatement import mdr_restatement
from test_pr_restatement import PR_FIGURES, pr_bounds, pr_restatement     # noqa: F401  (the bounds travel with the references)
from test_roc_restatement import auc_bound, roc_restatement               # noqa: F401
from test_rocq_restatement import roc_restatement_quantile
from test_scod_restatement import FIGURES as SCOD_FIGURES, area_bound, scod_restatement      # noqa: F401

F32 = np.float32
TILE = 2048                    # ROC_TILE of csrc/roc_sort.h
SCAN = 1024                    # MISC_SCAN of csrc/misclass.hip, and the threads of scod_offsets_kernel
KEPT = [pc / 100 for pc in range(90, 100)]
FACTORS = [(1, 1), (4, 1), (3, 7), (255, 255)]
FLT_MAX, FLT_MIN = float(np.finfo(F32).max), float(np.finfo(F32).tiny)
ALL = ('roc0', 'roc1', 'rocq', 'pr', 'scod', 'mdr')
NO_MEAN = ('roc0', 'rocq', 'pr', 'scod', 'mdr')
ON_GRID = ('tiefree', 'sorted_asc', 'sorted_desc', 'organ_pipe', 'signed_zeros', 'all_equal', 'straddle')
TIEFREE_SIZES = (2, 3, 2047, 2048, 2049, 4096, 4097, 8193, 16385)
PAIRS = ((2049, 1), (1, 8193), (4097, 2047))
STRADDLE_ENDS = (2047, 2048, 2049, 4095, 4096, 4097)

Row = namedtuple('Row', 'name kind n_in n_out seed users arg')


def _rows():
    rows, seed = [], [100]

    def add(name, kind, n_in, n_out, users, arg=None):
        seed[0] += 1
        rows.append(Row(name, kind, n_in, n_out, seed[0], users, arg))
    for n in TIEFREE_SIZES:
        add(f'tiefree_{n}', 'tiefree', n, n, ALL)
    for a, b in PAIRS:
        add(f'pair_{a}_{b}', 'tiefree', a, b, ('roc0', 'roc1', 'rocq', 'pr'))
    for n in (64, 4097):
        add(f'signed_zeros_{n}', 'signed_zeros', n, n, ALL)
    add('denormals_2049', 'denormals', 2049, 2049, NO_MEAN)
    add('extremes_2049', 'extremes', 2049, 2049, ('roc0', 'pr', 'scod'))
    add('adjacent_bits_6000', 'adjacent_bits', 6000, 6000, NO_MEAN)
    for n in (4097, 8193):
        add(f'all_equal_{n}', 'all_equal', n, n, ALL)
    for b in STRADDLE_ENDS:
        add(f'straddle_{b}', 'straddle', 6000, 6000, ALL, b)
    for kind in ('sorted_asc', 'sorted_desc', 'organ_pipe'):
        for n in (4097, 8193):
            add(f'{kind}_{n}', kind, n, n, ALL)
    return rows


ROWS = _rows()
BY_NAME = {r.name: r for r in ROWS}


def ids(r):
    return r.name


def padded(n):
    p = TILE
    while p < n:
        p <<= 1
    return p


def stages(n):
    """merge stages of the bitonic network above the tile"""
    return (padded(n) // TILE).bit_length() - 1


def bits_f32(b):
    return np.asarray(b, np.uint32).view(F32)


def _pool(kind):
    if kind == 'signed_zeros':
        return np.array([-1., -0., 0., 1.], F32)
    if kind == 'denormals':
        k = np.arange(1, 9, dtype=np.uint32)
        return np.concatenate([bits_f32(k), bits_f32(k | 0x80000000), np.array([0., -0., FLT_MIN, -FLT_MIN], F32)])
    if kind == 'adjacent_bits':
        k = np.arange(1500, dtype=np.uint32)                   # +0. and the 1499 patterns above it; -0. and the 1499 below it
        one = np.uint32(0x3F800000)
        return np.concatenate([bits_f32(k), bits_f32(k | 0x80000000), bits_f32(one + k), bits_f32(one - 1 - k)])
    raise ValueError(kind)


def values(row, side):
    """The fp32 vector of one side of a row (0: ins - also the SCOD / misclassification score row -, 1: outs)."""
    n = (row.n_in, row.n_out)[side]
    rng = np.random.default_rng([row.seed, side])
    kind = row.kind
    if kind in ('tiefree', 'sorted_asc', 'sorted_desc', 'organ_pipe'):
        v = ((rng.choice(32767, n, replace=False) - 16383) / 1024).astype(F32)
        if kind == 'tiefree':
            return v
        s = np.sort(v)
        return {'sorted_asc': s, 'sorted_desc': s[::-1].copy(), 'organ_pipe': np.concatenate([s[::2], s[1::2][::-1]])}[kind]
    if kind in ('signed_zeros', 'denormals'):
        return rng.choice(_pool(kind), n)
    if kind == 'adjacent_bits':
        pool = _pool(kind)
        assert n == len(pool)
        return rng.permutation(pool) if side == 0 else rng.choice(pool, n)
    if kind == 'extremes':
        v = rng.standard_normal(n).astype(F32)
        where = rng.permutation(n)[:4 * (n // 16)].reshape(4, -1)
        for w, x in zip(where, (FLT_MAX, -FLT_MAX, np.inf, -np.inf)):
            v[w] = x
        return v
    if kind == 'all_equal':
        return np.full(n, 0.5, F32)
    if kind == 'straddle':
        return rng.permutation(np.concatenate([np.full(row.arg, 0.25, F32), np.full(n - row.arg, 0.75, F32)]))
    raise ValueError(kind)


def flush(v):
    """The vector as a kernel that flushed denormals to zero would see it"""
    v = np.asarray(v, F32)
    return np.where(np.abs(v) < F32(FLT_MIN), np.copysign(F32(0), v), v).astype(F32)


def raw_key_image(v):
    """Scores whose STABLE order is the order of the raw sortable bits, which put -0. strictly in front of +0.: every -0. becomes
    the negative denormal next to it.  For vectors that hold no other value in (-FLT_MIN, 0)."""
    v = np.asarray(v, F32)
    assert not ((v < 0) & (v > -F32(FLT_MIN))).any()
    return np.where((v == 0) & np.signbit(v), bits_f32(0x80000001), v).astype(F32)


def labels(n):
    """(y_true, y_est) of the SCOD rows of length n: about 40 % OOD (y_true = -1), about 30 % of the rest wrong; position 0 is
    in-distribution and position 1 OOD, so neither side is empty from n = 2 on."""
    rng = np.random.default_rng([7, n])
    y_true = rng.integers(0, 10, n)
    y_est = np.where(rng.random(n) < 0.3, (y_true + 1) % 10, y_true)
    y_true = np.where(rng.random(n) < 0.4, -1, y_true)
    y_true[0], y_true[1] = abs(y_true[0]), -1
    return y_true.astype(np.int64), y_est.astype(np.int64)


def mask(n):
    """The correctly-classified mask of the misclassification rows of length n: about 60 % correct, position 0 correct and
    position 1 not."""
    m = np.random.default_rng([11, n]).random(n) < 0.6
    m[0], m[1] = True, False
    return m


def roc_modes(row):
    """The mode values `ops.roc_curve` takes, for the modes this row runs in"""
    out = [False] if 'roc0' in row.users else []
    if 'roc1' in row.users:
        out.append('around-mean')
    if 'rocq' in row.users:
        out += [('quantile', a, b) for a, b in FACTORS]
    return out


def pr_modes(row):
    return ([False] if 'pr' in row.users else []) + (['around-mean'] if 'pr' in row.users and 'roc1' in row.users else [])


def roc_ref(ins, outs, mode):
    """-> auc, fpr, tpr, low, up of one row in one mode (a value of roc_modes)"""
    if isinstance(mode, tuple):
        return roc_restatement_quantile(ins, outs, KEPT, mode[1:])
    return roc_restatement(ins, outs, KEPT, around_mean=mode == 'around-mean')


def pr_ref(ins, outs, mode):
    return pr_restatement(ins, outs, 1 if mode == 'around-mean' else 0)


def scod_ref(scores):
    return scod_restatement(scores, *labels(len(scores)))


def mdr_ref(scores):
    return mdr_restatement(scores, mask(len(scores)), KEPT)


def permuted(v, j):
    """Row j of a batched call: the vector in an order of its own (row 0 as it is)"""
    return v if j == 0 else v[np.random.default_rng([13, j]).permutation(len(v))]


# ------------------------------------------------------------------------------------------------------------ the long rows
# Scores are the integers below n in the order i -> i * LONG_A mod n (exact in fp32 below 2^24), labels a function of the
# position: the sorted order is the inverse permutation, known in closed form, and every expected count is one cumsum over it.
LONG_A = 1000003
SCOD_LONG_N = (1 << 21) + 1            # 2048 tiles of the padded row: scod_offsets_kernel scans two tile totals per thread
MDR_LONG_N = (1 << 20) + 1025          # 1026 scan blocks: misclass_offsets_kernel runs a second chunk with a carry
MDR_LONG_THR = [-1., 0.5, 1023.5, 262144.25, 524288., 786432., 1049599.5, 1049600., 1049601.]


def long_scores(n):
    assert math.gcd(LONG_A, n) == 1 and n < 1 << 24
    return ((np.arange(n, dtype=np.int64) * LONG_A) % n).astype(F32)


def long_order(n):
    """position of the sample whose score is r, for every r below n"""
    return (np.arange(n, dtype=np.int64) * pow(LONG_A, -1, n)) % n


def scod_long_labels(n=SCOD_LONG_N):
    i = np.arange(n, dtype=np.int64)
    y_true = np.where(i % 4 == 3, -1, i % 10)
    y_est = np.where(i % 5 == 0, (i + 1) % 10, i % 10)
    return y_true, y_est


def scod_long_closed_form(n=SCOD_LONG_N):
    """-> (tpr, selective_risk, fpr) fp32 and [fpr95, sr95, auroc, aust, auscodt] of the long SCOD row, without a sort"""
    y_true, y_est = scod_long_labels(n)
    order = long_order(n)
    inside, wrong = (y_true >= 0)[order], ((y_true >= 0) & (y_true != y_est))[order]
    inn, bad = np.cumsum(inside), np.cumsum(wrong)
    ood = np.arange(1, n + 1) - inn
    tpr, fpr = inn.astype(F32) / F32(inn[-1]), ood.astype(F32) / F32(ood[-1])
    sr = np.where(inn > 0, bad.astype(F32) / np.maximum(inn, 1).astype(F32), F32(0)).astype(F32)
    half = F32(0.5) * sr + F32(0.5) * fpr
    kept = tpr >= F32(0.95)
    t, s, f, h = (v.astype(np.float64) for v in (tpr, sr, fpr, half))
    trapezoid = getattr(np, 'trapezoid', None) or np.trapz
    return (tpr, sr, fpr), [float(fpr[kept].min()), float(sr[kept].min()), float(trapezoid(t, f)), float(trapezoid(s, t)),
                            float(trapezoid(h, t))]


def mdr_long_mask(n=MDR_LONG_N):
    return np.arange(n) % 3 != 0


def mdr_long_counts(thr, n=MDR_LONG_N):
    """-> tp, fp int32 (K,): the correct / missed samples of the long misclassification row whose score is >= thr[k]"""
    correct = mdr_long_mask(n)[long_order(n)]                  # by score
    below = np.concatenate([[0], np.cumsum(correct)])          # below[r] = correct samples with a score < r
    first = np.clip(np.ceil(np.asarray(thr, np.float64)), 0, n).astype(np.int64)     # the smallest integer score >= thr
    tp = below[n] - below[first]
    return tp.astype(np.int32), ((n - first) - tp).astype(np.int32)
