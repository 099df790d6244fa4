"""Numpy restatement of the reference's misclassification_detection_rates (cvae.py:1975-2079) - split by correctness, ROC,
confusion counts at the kept thresholds - against the goldens the reference wrote (tools/gen_mdr_golden.py ->
tests/golden/mdr/*.npz), and fp64 restatements of the score formulas (batch_dist_measures, cvae.py:1013-1063) against the golden's
fp32 score rows.  No GPU.  `mdr_restatement` and `fp64_rows` are also the checkers of tests/test_7_mdr_gpu.py."""
import glob
import os

import numpy as np

from test_roc_restatement import auc_bound, roc_restatement

CASES = ('cvae_1500', 'cvae_257', 'one_correct_300', 'ties_2000', 'vib_1200')


def mdr_restatement(row, correct, kept):
    """-> dict(auc, fpr, tpr, low, tp, fp, precision) of one fp32 score row: ROC of row[correct] against row[~correct], then the
    counts of correct / missed samples at or above each kept low threshold, on the scores widened to fp64."""
    row, correct = np.asarray(row, np.float32), np.asarray(correct, bool)
    auc, fpr, tpr, low, _ = roc_restatement(row[correct], row[~correct], kept)
    wide = row.astype(np.float64)
    tp = np.array([(wide[correct] >= t).sum() for t in low], np.int32)
    fp = np.array([(wide[~correct] >= t).sum() for t in low], np.int32)
    with np.errstate(invalid='ignore', divide='ignore'):
        precision = tp / (tp + fp).astype(np.float64)
    return dict(auc=auc, fpr=fpr, tpr=tpr, low=low, tp=tp, fp=fp, precision=precision)


def fp64_rows(tensors, methods):
    """{method: fp64 score row} from the fp32 recorder tensors ({name: (C, N) or (N,) array}, `logits` as (C, N))."""
    def soft(v):
        e = np.exp(v - v.max(0))
        return (e / e.sum(0)).max(0)
    f = {k: np.asarray(v).astype(np.float64) for k, v in tensors.items() if k != 'y_true'}
    out = {}
    for m in methods:
        T = float(m.split('-')[-1]) if '-' in m else 1.
        if m.startswith('odin'):
            out[m] = f[m]
        elif m == 'iws':
            out[m] = np.log(np.exp(f['iws'] - f['iws'].max(0)).sum(0)) + f['iws'].max(0) + np.log(f['iws'].shape[0])
        elif m == 'softiws':
            out[m] = soft(f['iws'])                                      # cvae.py:1024-1028: +iws, but -iws / T with a temperature
        elif m.startswith('soft'):
            out[m] = soft(-f[m.split('-')[0][4:] or 'kl'] / T)
        elif m in ('kl', 'zdist'):
            out[m] = (-f[m]).max(0)
        elif m == 'max':
            out[m] = (-f['total']).max(0)
        elif m == 'logits':
            out[m] = f['logits'].max(0)
        elif m.startswith('baseline'):
            out[m] = soft(f['logits'] / T)
        elif m == 'hyz':
            z = f['logits'] - f['logits'].max(0)
            p = np.exp(z) / np.exp(z).sum(0)
            out[m] = (p * np.log(p)).sum(0)
        else:
            raise ValueError(m)
    return out


def family(m):
    return 'odin' if m.startswith('odin') else m.split('-')[0]


EXACT_FAMILIES = ('kl', 'zdist', 'max', 'logits', 'odin')               # pure max / negation / recorded rows


def load_case(golden_dir, name):
    g = np.load(os.path.join(golden_dir, 'mdr', name + '.npz'))
    case = {k: g[k] for k in g.files}
    case['methods'], case['predict'] = [str(m) for m in case['methods']], [str(p) for p in case['predict']]
    case['recorder'] = {k[4:]: v for k, v in case.items() if k.startswith('rec_')}
    case['referr'] = dict(zip((str(n) for n in case.get('referr_names', [])), (float(v) for v in case.get('referr_values', []))))
    return case


def test_goldens_cover_the_cases(golden_dir):
    files = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(golden_dir, 'mdr', '*.npz')))
    assert tuple(files) == CASES
    biggest = max(os.path.getsize(f) for f in glob.glob(os.path.join(golden_dir, '*.npz')))
    for f in glob.glob(os.path.join(golden_dir, 'mdr', '*.npz')):
        assert os.path.getsize(f) <= biggest
    c = load_case(golden_dir, 'cvae_1500')
    assert c['predict'] == ['iws', 'closest'] and len(c['methods']) == 35 and c['scores'].shape == (35, 1500)
    assert c['recorder']['kl'].shape == (10, 1500) and c['recorder']['kl'].dtype == np.float32
    for k in ('softkl-1', 'softzdist-1000', 'baseline-50', 'iws', 'kl', 'max', 'zdist', 'hyz'):
        assert k in c['methods']
    assert not [m for m in c['methods'] if m.startswith('softiws')]      # softiws* expands to nothing (no such methods_params key)
    assert load_case(golden_dir, 'cvae_257')['scores'].shape == (35, 257)
    v = load_case(golden_dir, 'vib_1200')
    assert v['predict'] == ['esty'] and v['methods'][:3] == ['baseline', 'logits', 'hyz']
    assert len(v['methods']) == 8 and all(m.startswith('odin-') for m in v['methods'][3:])
    t = load_case(golden_dir, 'ties_2000')
    assert all(len(np.unique(row)) <= 64 for row in t['scores'])
    o = load_case(golden_dir, 'one_correct_300')
    assert int(o['mask_given'].sum()) == 1
    for name in CASES:
        assert np.array_equal(load_case(golden_dir, name)['kept'], [pc / 100 for pc in range(90, 100)])


def test_input_conditions(golden_dir):
    for name in ('cvae_1500', 'cvae_257', 'vib_1200'):
        c = load_case(golden_dir, name)
        rec = c['recorder']
        assert (rec['logits'].max(0) - rec['logits'].min(0)).max() < 80
        for pm, (key, best) in {'iws': ('iws', np.max), 'closest': ('zdist', np.min), 'esty': ('logits', np.max)}.items():
            if pm in c['predict']:
                assert ((rec[key] == best(rec[key], 0)).sum(0) == 1).all(), (name, pm)
                pred = (np.argmax if best is np.max else np.argmin)(rec[key], 0)
                assert np.array_equal(pred == rec['y_true'], c[f'mask_{pm}'])
        assert np.isfinite(c['scores']).all()


def test_restatement_reproduces_every_golden(golden_dir):
    for name in CASES:
        c = load_case(golden_dir, name)
        for pm in c['predict']:
            mask = c[f'mask_{pm}']
            assert float(c[f'accuracy_{pm}']) == mask.sum() / len(mask), (name, pm)
            for i, m in enumerate(c['methods']):
                r = mdr_restatement(c['scores'][i], mask, c['kept'])
                for k in ('tpr', 'fpr', 'low', 'tp', 'fp'):
                    assert np.array_equal(r[k], c[f'{k}_{pm}'][i]), (name, pm, m, k)
                assert np.array_equal(r['precision'], c[f'precision_{pm}'][i], equal_nan=True), (name, pm, m)
                assert abs(r['auc'] - float(c[f'auc_{pm}'][i])) <= auc_bound(int(mask.sum())), (name, pm, m)


def test_fp64_score_formulas_agree_with_the_golden_rows(golden_dir):
    for name in ('cvae_1500', 'cvae_257', 'vib_1200'):
        c = load_case(golden_dir, name)
        exact = fp64_rows(c['recorder'], c['methods'])
        assert set(c['referr']) == {family(m) for m in c['methods']}
        for i, m in enumerate(c['methods']):
            err = float(np.abs(c['scores'][i].astype(np.float64) - exact[m]).max())
            assert err <= c['referr'][family(m)], (name, m, err)
            if family(m) in EXACT_FAMILIES:
                assert err == 0 and c['referr'][family(m)] == 0, (name, m)
        for fam, e in c['referr'].items():
            assert e < 1e-5, (name, fam, e)                              # fp32 rounding of values of magnitude <= 100, nothing more
