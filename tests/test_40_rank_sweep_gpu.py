"""Every row of tests/rank_cases.py on the device, through every user it feeds: ops.roc_curve, ops.pr_metrics, ops.scod_curve,
ops.misclass_split, ops.misclass_confusion, ops.misclass_rates - the padded bitonic sort and the order-preserving key of
csrc/roc_sort.h under the scans and searches of csrc/roc.hip, csrc/prc.hip, csrc/scod.hip and csrc/misclass.hip.

Rates, kept values, the SCOD curves with fpr95 / sr95, split rows, confusion counts and status words are compared bit for bit
with the restatements; thresholds by value (the restatement sorts with numpy, which leaves the order - so the sign - of a -0.
and a +0. threshold open; every other value has one bit pattern); the fp64 sums under auc_bound, pr_bounds and area_bound,
printed against their bound before they are held.  All rows of one size go into ONE call, each in an order of its own, and each
must equal its own single-row call byte for byte; every call runs twice and must repeat its bytes.  The raw entry points run with
a workspace of exactly *_workspace_bytes and outputs that are carved out of sentinel-filled byte buffers with a 256-byte guard on
either side: the guards stay intact and every output element is written.  (`Guarded` of tests/test_35_loss_tail_sweep_gpu.py
reroutes the fp32 allocations of jvae_hip.ops; these calls take int32, fp64 and byte buffers by pointer, hence `Carved` here.)"""
import time

import numpy as np
import pytest
import torch

import rank_cases as rc
from rank_cases import F32

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CURVES = ('tpr', 'selective_risk', 'fpr')
_refs = {}


def ref(what, row, *key):
    """One reference per (user, row, mode), computed once and shared"""
    k = (what, row.name) + key
    if k not in _refs:
        ins, outs = rc.values(row, 0), rc.values(row, 1)
        _refs[k] = {'roc': lambda: rc.roc_ref(ins, outs, *key), 'pr': lambda: rc.pr_ref(ins, outs, *key)}[what]()
    return _refs[k]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def host(r):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}


def twice(f):
    a, b = host(f()), host(f())
    assert set(a) == set(b)
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), f'two runs differ in {k}'
    return a


def sizes(user_test):
    out = []
    for r in rc.ROWS:
        if user_test(r) and (r.n_in, r.n_out) not in out:
            out.append((r.n_in, r.n_out))
    return out


def size_id(s):
    return f'{s[0]}_{s[1]}'


def hold_roc(got, want, n_in, what):
    auc, fpr, tpr, low, up = want
    print(what, 'auc', float(got['auc']), 'ref', auc, 'diff', abs(float(got['auc']) - auc), 'bound', rc.auc_bound(n_in))
    assert int(got['status']) == 0, what
    for k, w in (('fpr', fpr), ('tpr', tpr)):
        assert got[k].dtype == np.float64 and got[k].tobytes() == np.asarray(w, np.float64).tobytes(), (what, k, got[k], w)
    for k, w in (('low', low), ('up', up)):
        assert got[k].dtype == np.float64 and np.array_equal(got[k], w), (what, k, got[k], w)
    assert abs(float(got['auc']) - auc) <= rc.auc_bound(n_in), what


# ------------------------------------------------------------------------------------------------------------ ROC
ROC_SIZES = sizes(lambda r: bool(rc.roc_modes(r)))


@pytest.mark.parametrize('size', ROC_SIZES, ids=size_id)
def test_roc_curve(size):
    from jvae_hip import ops
    entries = [(r, m) for r in rc.ROWS if (r.n_in, r.n_out) == size for m in rc.roc_modes(r)]
    assert len(entries) > 1
    ins = np.stack([rc.permuted(rc.values(r, 0), j) for j, (r, _) in enumerate(entries)])
    outs = np.stack([rc.permuted(rc.values(r, 1), j) for j, (r, _) in enumerate(entries)])
    modes = [m for _, m in entries]
    d_ins, d_outs = dev(ins), dev(outs)
    batch = twice(lambda: ops.roc_curve(d_ins, d_outs, rc.KEPT, modes))
    for j, (r, m) in enumerate(entries):
        one = twice(lambda: ops.roc_curve(d_ins[j], d_outs[j], rc.KEPT, m))
        for k in batch:
            assert one[k].tobytes() == batch[k][j].tobytes(), (r.name, m, k)
        hold_roc({k: v[j] for k, v in batch.items()}, ref('roc', r, m), r.n_in, (r.name, m))


# ------------------------------------------------------------------------------------------------------------ PR
PR_SIZES = sizes(lambda r: 'pr' in r.users)


@pytest.mark.parametrize('size', PR_SIZES, ids=size_id)
def test_pr_metrics(size):
    from jvae_hip import ops
    entries = [(r, m) for r in rc.ROWS if (r.n_in, r.n_out) == size for m in rc.pr_modes(r)]
    entries.append((entries[0][0], ('quantile', 3, 7)))        # a quantile row has no scalar score: five NaNs, no status
    ins = np.stack([rc.permuted(rc.values(r, 0), j) for j, (r, _) in enumerate(entries)])
    outs = np.stack([rc.permuted(rc.values(r, 1), j) for j, (r, _) in enumerate(entries)])
    modes = [m for _, m in entries]
    d_ins, d_outs = dev(ins), dev(outs)
    batch = twice(lambda: ops.pr_metrics(d_ins, d_outs, modes))
    assert batch['status'].tolist() == [0] * len(entries)
    for j, (r, m) in enumerate(entries):
        one = twice(lambda: ops.pr_metrics(d_ins[j], d_outs[j], m))
        for k in batch:
            assert one[k].tobytes() == batch[k][j].tobytes(), (r.name, m, k)
        if isinstance(m, tuple):
            assert all(np.isnan(batch[k][j]) for k in rc.PR_FIGURES)
            continue
        for k, w, b in zip(rc.PR_FIGURES, ref('pr', r, m), rc.pr_bounds(*size)):
            print(r.name, m, k, float(batch[k][j]), 'ref', w, 'diff', abs(float(batch[k][j]) - w), 'bound', b)
            assert abs(float(batch[k][j]) - w) <= b, (r.name, m, k)


# ------------------------------------------------------------------------------------------------------------ SCOD
SCOD_SIZES = sizes(lambda r: 'scod' in r.users)


def hold_scod(got, want, n, what):
    curves, figures = want
    assert int(got['status']) == 0, what
    for k, w in zip(CURVES, curves):
        differ = int((got[k].view(np.uint32) != w.view(np.uint32)).sum())
        if differ:
            print(what, k, 'differs at', differ, 'of', n, 'positions; device', got[k][:16], 'stable order', w[:16])
        assert got[k].dtype == F32 and got[k].tobytes() == w.tobytes(), (what, k, f'{differ} of {n} positions differ')
    assert got['figures'][0] == figures[0] and got['figures'][1] == figures[1], (what, got['figures'][:2], figures[:2])
    for k in range(2, 5):
        g, w = float(got['figures'][k]), figures[k]
        print(what, rc.SCOD_FIGURES[k], g, 'ref', w, 'diff', abs(g - w), 'bound', rc.area_bound(n, w))
        assert abs(g - w) <= rc.area_bound(n, w), (what, k)


@pytest.mark.parametrize('size', SCOD_SIZES, ids=size_id)
def test_scod_curve(size):
    from jvae_hip import ops
    n = size[0]
    rows = [r for r in rc.ROWS if 'scod' in r.users and r.n_in == n]
    y_true, y_est = rc.labels(n)
    # every row as it is and once more in another order under the SAME labels: a score row of its own, with its own reference
    scores = np.stack([rc.values(r, 0) for r in rows] + [rc.permuted(rc.values(r, 0), j + 1) for j, r in enumerate(rows)])
    names = [r.name for r in rows] + [r.name + '/permuted' for r in rows]
    d_s, d_t, d_e = dev(scores), dev(y_true), dev(y_est)
    batch = twice(lambda: ops.scod_curve(d_s, d_t, d_e, n_in=int((y_true >= 0).sum())))
    failed = []
    for j, name in enumerate(names):
        one = twice(lambda: ops.scod_curve(d_s[j], d_t, d_e))                  # n_in counted by the call
        for k in batch:
            assert one[k].tobytes() == batch[k][j].tobytes(), (name, k)
        try:
            hold_scod({k: v[j] for k, v in batch.items()}, rc.scod_restatement(scores[j], y_true, y_est), n, name)
        except AssertionError as e:                            # name every failing row of the call, not the first alone
            failed.append((name, str(e)[:200]))
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------------ misclassification
MDR_SIZES = sizes(lambda r: 'mdr' in r.users)


@pytest.mark.parametrize('size', MDR_SIZES, ids=size_id)
def test_misclass_split_confusion_and_rates(size):
    from jvae_hip import ops
    n = size[0]
    rows = [r for r in rc.ROWS if 'mdr' in r.users and r.n_in == n]
    m = rc.mask(n)
    scores = np.stack([rc.values(r, 0) for r in rows] + [rc.permuted(rc.values(r, 0), j + 1) for j, r in enumerate(rows)])
    names = [r.name for r in rows] + [r.name + '/permuted' for r in rows]
    d_s, d_m = dev(scores), dev(m)

    def split():
        ins, outs, nc = ops.misclass_split(d_s, d_m)
        return dict(ins=ins, outs=outs, nc=np.int64(nc))
    s = twice(split)
    assert s['nc'] == m.sum() and s['ins'].tobytes() == scores[:, m].tobytes() and s['outs'].tobytes() == scores[:, ~m].tobytes()
    batch = twice(lambda: ops.misclass_rates(d_s, d_m, rc.KEPT))
    assert batch['n_correct'] == m.sum()
    for j, name in enumerate(names):
        one = twice(lambda: ops.misclass_rates(d_s[j], d_m, rc.KEPT))
        want = rc.mdr_restatement(scores[j], m, rc.KEPT)
        for k in batch:
            assert np.asarray(one[k]).tobytes() == np.asarray(batch[k] if k == 'n_correct' else batch[k][j]).tobytes(), (name, k)
        hold_roc({k: v[j] for k, v in batch.items() if k != 'n_correct'},
                 (want['auc'], want['fpr'], want['tpr'], want['low'], np.full(len(rc.KEPT), np.inf)), int(m.sum()), name)
        for k in ('tp', 'fp'):
            assert batch[k].dtype == np.int32 and batch[k][j].tobytes() == want[k].astype(np.int32).tobytes(), (name, k)
    # the confusion counts on their own, at thresholds the host names
    lows = np.stack([rc.mdr_restatement(row, m, rc.KEPT)['low'] for row in scores])
    c = twice(lambda: dict(zip(('tp', 'fp'), ops.misclass_confusion(d_s, d_m, dev(lows)))))
    assert c['tp'].tobytes() == batch['tp'].tobytes() and c['fp'].tobytes() == batch['fp'].tobytes()


# ------------------------------------------------------------------------------------------------------------ raw entry points
GUARD, SENTINEL = 256, 0xA5


class Carved:
    """Device buffers for one raw call, each carved out of a sentinel-filled byte buffer with a guard band on either side"""

    def __init__(self):
        self.bufs = []

    def take(self, nbytes, dtype=None, output=True):
        """nbytes from a 256-byte boundary -> the uint8 view (dtype None: a workspace, whose contents are not looked at) or the
        view as `dtype`"""
        buf = torch.full((nbytes + 3 * GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
        off = GUARD + (-(buf.data_ptr() + GUARD)) % GUARD
        view = buf[off:off + nbytes]
        assert view.data_ptr() % GUARD == 0
        self.bufs.append((buf, off, nbytes, dtype if output else None))
        return view if dtype is None else view.view(dtype)

    def out(self, shape, dtype):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        return self.take(n, dtype).view(shape)

    def check(self):
        torch.cuda.synchronize()
        for buf, off, nbytes, dtype in self.bufs:
            assert bool((buf[:off] == SENTINEL).all()) and bool((buf[off + nbytes:] == SENTINEL).all()), 'a guard band was written'
            if dtype is not None:                              # no element is left as the sentinel pattern
                size = torch.empty(0, dtype=dtype).element_size()
                assert bool((buf[off:off + nbytes].view(-1, size) != SENTINEL).any(1).all()), 'an output element was not written'


RAW_N = (2048, 2049, 4097, 16385)      # one row per regime of the padded length: one tile, then one, two and four stages above it


def raw_rows(n):
    r = rc.BY_NAME[f'tiefree_{n}']
    return r, rc.values(r, 0), rc.values(r, 1)


@pytest.mark.parametrize('n', RAW_N)
def test_raw_roc_entry_point_inside_guards(n):
    from jvae_hip import lib, ops
    L = lib.load()
    r, ins, outs = raw_rows(n)
    modes = [False, 'around-mean', ('quantile', 3, 7)]
    M, K = len(modes), len(rc.KEPT)
    d_ins, d_outs = dev(np.stack([ins] * M)), dev(np.stack([outs] * M))
    kept, words = dev(np.array(rc.KEPT)), dev(np.array([ops.roc_mode_word(m) for m in modes], np.int32))
    c = Carved()
    nbytes = L.jvae_roc_workspace_bytes(M, n, n)
    ws = c.take(nbytes)
    auc, status = c.out((M,), torch.float64), c.out((M,), torch.int32)
    fpr, tpr, low, up = (c.out((M, K), torch.float64) for _ in range(4))
    rcode = L.jvae_roc_curve_f32(d_ins.data_ptr(), d_outs.data_ptr(), kept.data_ptr(), words.data_ptr(), auc.data_ptr(), fpr.data_ptr(),
                                 tpr.data_ptr(), low.data_ptr(), up.data_ptr(), status.data_ptr(), M, n, n, K, ws.data_ptr(), nbytes,
                                 lib.stream_ptr())
    assert rcode == 0
    c.check()
    assert L.jvae_roc_curve_f32(d_ins.data_ptr(), d_outs.data_ptr(), kept.data_ptr(), words.data_ptr(), auc.data_ptr(), fpr.data_ptr(),
                                tpr.data_ptr(), low.data_ptr(), up.data_ptr(), status.data_ptr(), M, n, n, K, ws.data_ptr(), nbytes - 1,
                                lib.stream_ptr()) != 0          # one byte short is refused
    got = host(dict(auc=auc, fpr=fpr, tpr=tpr, low=low, up=up, status=status))
    for j, m in enumerate(modes):
        hold_roc({k: v[j] for k, v in got.items()}, ref('roc', r, m), n, (r.name, m, 'raw'))


@pytest.mark.parametrize('n', RAW_N)
def test_raw_pr_entry_point_inside_guards(n):
    from jvae_hip import lib
    L = lib.load()
    r, ins, outs = raw_rows(n)
    modes = [False, 'around-mean']
    M = len(modes)
    d_ins, d_outs, words = dev(np.stack([ins] * M)), dev(np.stack([outs] * M)), dev(np.array([0, 1], np.int32))
    c = Carved()
    nbytes = L.jvae_pr_workspace_bytes(M, n, n)
    ws, figures, status = c.take(nbytes), c.out((M, 5), torch.float64), c.out((M,), torch.int32)
    args = (d_ins.data_ptr(), d_outs.data_ptr(), words.data_ptr(), figures.data_ptr(), status.data_ptr(), M, n, n, ws.data_ptr())
    assert L.jvae_pr_metrics_f32(*args, nbytes, lib.stream_ptr()) == 0
    c.check()
    assert L.jvae_pr_metrics_f32(*args, nbytes - 1, lib.stream_ptr()) != 0
    assert status.tolist() == [0, 0]
    for j, m in enumerate(modes):
        for k, g, w, b in zip(rc.PR_FIGURES, figures[j].tolist(), ref('pr', r, m), rc.pr_bounds(n, n)):
            print(r.name, m, 'raw', k, g, 'ref', w, 'diff', abs(g - w), 'bound', b)
            assert abs(g - w) <= b, (r.name, m, k)


@pytest.mark.parametrize('n', RAW_N)
def test_raw_scod_entry_point_inside_guards(n):
    from jvae_hip import lib
    L = lib.load()
    r, s, s2 = raw_rows(n)
    y_true, y_est = rc.labels(n)
    scores = np.stack([s, s2])
    M = 2
    d_s, d_t, d_e = dev(scores), dev(y_true), dev(y_est)
    c = Carved()
    nbytes = L.jvae_scod_workspace_bytes(M, n)
    ws, curves = c.take(nbytes), c.out((3, M, n), torch.float32)
    figures, status = c.out((M, 5), torch.float64), c.out((M,), torch.int32)
    args = (d_s.data_ptr(), d_t.data_ptr(), d_e.data_ptr(), curves.data_ptr(), figures.data_ptr(), status.data_ptr(), M, n,
            int((y_true >= 0).sum()), ws.data_ptr())
    assert L.jvae_scod_curve_f32(*args, nbytes, lib.stream_ptr()) == 0
    c.check()
    assert L.jvae_scod_curve_f32(*args, nbytes - 1, lib.stream_ptr()) != 0
    got = host(dict(zip(CURVES, curves), figures=figures, status=status))
    for j in range(M):
        hold_scod({k: v[j] for k, v in got.items()}, rc.scod_restatement(scores[j], y_true, y_est), n, (r.name, j, 'raw'))


@pytest.mark.parametrize('n', RAW_N)
def test_raw_split_entry_point_inside_guards(n):
    from jvae_hip import lib
    L = lib.load()
    r, s, s2 = raw_rows(n)
    scores, m = np.stack([s, s2]), rc.mask(n)
    d_s, d_m = dev(scores), dev(m.astype(np.uint8))
    c = Carved()
    nbytes = L.jvae_misclass_split_workspace_bytes(n)
    ws, out, count = c.take(nbytes), c.out((2 * n,), torch.float32), c.out((1,), torch.int32)
    args = (d_s.data_ptr(), d_m.data_ptr(), out.data_ptr(), count.data_ptr(), 2, n, ws.data_ptr())
    assert L.jvae_misclass_split_f32(*args, nbytes, lib.stream_ptr()) == 0
    c.check()
    assert L.jvae_misclass_split_f32(*args, nbytes - 1, lib.stream_ptr()) != 0
    nc = int(count.item())
    assert nc == m.sum()
    assert out.cpu().numpy().tobytes() == np.concatenate([scores[:, m].ravel(), scores[:, ~m].ravel()]).tobytes()


# ------------------------------------------------------------------------------------------------------------ status words
def test_refused_inputs_are_reported_in_the_status_word_and_a_healthy_call_follows():
    """NaN scores (a negative-sign NaN sorts in FRONT of every score under the key, a positive one behind), a non-finite in-score
    of an around-mean row, a malformed mode word and a wrong n_in: each is a status bit, none disturbs the next call."""
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    r = rc.BY_NAME['tiefree_2049']
    ins, outs = rc.values(r, 0), rc.values(r, 1)
    neg_nan, pos_nan = rc.bits_f32(0xFFC00000), rc.bits_f32(0x7FC00000)
    assert np.isnan(neg_nan) and np.signbit(neg_nan) and np.isnan(pos_nan) and not np.signbit(pos_nan)

    def put(v, i, x):
        v = v.copy()
        v[i] = x
        return v
    extreme = rc.values(rc.BY_NAME['extremes_2049'], 0)
    rows_in = np.stack([ins, put(ins, 5, neg_nan), put(ins, 2048, pos_nan), ins, put(ins, 7, np.inf), extreme, extreme, ins, ins])
    rows_out = np.stack([outs, outs, outs, put(outs, 0, neg_nan), outs, outs, outs, put(outs, 9, -np.inf), outs])
    words = [0, 0, 1, 1, 1, 1, 0, 1, 3]
    want = [0, 1, 3, 1, 2, 2, 0, 0, 4]     # a NaN in-score of an around-mean row is non-finite too; out-scores may be infinite
    d_in, d_out, d_words = dev(rows_in), dev(rows_out), dev(np.array(words, np.int32))
    roc = twice(lambda: ops.roc_curve(d_in, d_out, rc.KEPT, d_words))
    assert roc['status'].tolist() == want
    pr = twice(lambda: ops.pr_metrics(d_in, d_out, d_words))
    assert pr['status'].tolist() == want
    for bad in (2 | 0 << 8 | 1 << 16, 2 | 1 << 8, 2 | 1 << 8 | 1 << 16 | 1 << 24, -1):
        w = dev(np.array([bad], np.int32))
        assert ops.roc_curve(d_in[:1], d_out[:1], rc.KEPT, w)['status'].tolist() == [4], bad
        assert ops.pr_metrics(d_in[:1], d_out[:1], w)['status'].tolist() == [4], bad
    with pytest.raises(JvaeHipError):
        ops.roc_check_status(roc['status'][8:])
    with pytest.raises(ValueError):
        ops.roc_check_status(roc['status'][1:2])
    # a malformed word runs as a one-sided row, and the healthy rows of the same call are untouched by their neighbours
    for j in (0, 6, 8):
        hold_roc({k: (v[j] if k != 'status' else np.int32(0)) for k, v in roc.items()}, rc.roc_ref(rows_in[j], rows_out[j], False),
                 r.n_in, ('status', j))
    y_true, y_est = rc.labels(r.n_in)
    d_t, d_e, n_in = dev(y_true), dev(y_est), int((y_true >= 0).sum())
    s = twice(lambda: ops.scod_curve(dev(np.stack([ins, put(ins, 5, neg_nan), put(ins, 2048, pos_nan)])), d_t, d_e, n_in=n_in))
    assert s['status'].tolist() == [0, 1, 1]
    s = twice(lambda: ops.scod_curve(dev(np.stack([ins, put(ins, 5, neg_nan)])), d_t, d_e, n_in=n_in - 1))
    assert s['status'].tolist() == [2, 3]
    with pytest.raises(JvaeHipError):
        ops.scod_check_status(s['status'][:1])
    torch.cuda.synchronize()
    # the follow-up healthy calls
    hold_roc(host(ops.roc_curve(d_in[0], d_out[0], rc.KEPT, 'around-mean')), ref('roc', r, 'around-mean'), r.n_in, 'healthy')
    assert int(ops.pr_metrics(d_in[0], d_out[0])['status']) == 0
    hold_scod(host(ops.scod_curve(d_in[0], d_t, d_e)), rc.scod_restatement(ins, y_true, y_est), r.n_in, 'healthy')


# ------------------------------------------------------------------------------------------------------------ the long rows
def test_long_scod_row_scans_two_tile_totals_per_thread():
    """n = 2^21 + 1: 2048 tiles, so scod_offsets_kernel runs per = 2 and scod_figures_kernel strides twice
    (test_rank_cases_host.py asserts the sizes).  The expected curves need no sort on the host: one cumsum."""
    from jvae_hip import ops
    n = rc.SCOD_LONG_N
    y_true, y_est = rc.scod_long_labels()
    d_s, d_t, d_e = dev(rc.long_scores(n)), dev(y_true), dev(y_est)
    n_in = int((y_true >= 0).sum())
    want = rc.scod_long_closed_form()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = ops.scod_curve(d_s, d_t, d_e, n_in=n_in)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    again = ops.scod_curve(d_s, d_t, d_e, n_in=n_in)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(f'long SCOD row, n = {n}: first call {1e3 * (t1 - t0):.3f} ms, second call {1e3 * (t2 - t1):.3f} ms (wall, synchronised)')
    for k in got:
        assert torch.equal(got[k], again[k]), f'two runs differ in {k}'
    hold_scod(host(got), want, n, 'scod_long')


def test_long_misclass_row_scans_a_second_chunk_of_block_counts():
    """N = 2^20 + 1025: 1026 scan blocks, so misclass_offsets_kernel carries the first chunk's total into a second one."""
    from jvae_hip import ops
    N = rc.MDR_LONG_N
    s, m = rc.long_scores(N), rc.mdr_long_mask()
    scores = np.stack([s, F32(N - 1) - s])
    d_s, d_m = dev(scores), dev(m)
    thr = np.array(rc.MDR_LONG_THR)
    tp, fp = rc.mdr_long_counts(thr)
    lows = dev(np.stack([thr, thr]))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ins, outs, nc = ops.misclass_split(d_s, d_m)
    ctp, cfp = ops.misclass_confusion(d_s, d_m, lows)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ins2, outs2, nc2 = ops.misclass_split(d_s, d_m)
    ctp2, cfp2 = ops.misclass_confusion(d_s, d_m, lows)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(f'long misclassification row, N = {N}: split + confusion {1e3 * (t1 - t0):.3f} ms, again {1e3 * (t2 - t1):.3f} ms '
          '(wall, synchronised; the split reads one count back)')
    assert nc == nc2 == int(m.sum())
    for a, b in ((ins, ins2), (outs, outs2), (ctp, ctp2), (cfp, cfp2)):
        assert torch.equal(a, b)
    assert ins.cpu().numpy().tobytes() == scores[:, m].tobytes() and outs.cpu().numpy().tobytes() == scores[:, ~m].tobytes()
    assert ctp.cpu().numpy()[0].tolist() == tp.tolist() and cfp.cpu().numpy()[0].tolist() == fp.tolist()
    wide = (N - 1) - np.arange(N)                              # the mirrored row N - 1 - s, by the rank of s
    correct = m[rc.long_order(N)]
    assert ctp.cpu().numpy()[1].tolist() == [int(correct[wide >= t].sum()) for t in thr]
    assert cfp.cpu().numpy()[1].tolist() == [int((~correct)[wide >= t].sum()) for t in thr]
