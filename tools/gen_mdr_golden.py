#!/usr/bin/env python3
"""Write tests/golden/mdr/*.npz: recorded losses, score rows and what the REFERENCE's misclassification_detection_rates gives.

    python tools/gen_mdr_golden.py --reference <checkout of moxime/joint-vae> [--timing]

Route: the PREFERRED one of the two the feature's issue names.  The model-level cases (cvae_1500, cvae_257, vib_1200) drive the
reference's own `ClassificationVariationalNetwork.misclassification_detection_rates` (cvae.py:1913-2079) on a small reference
model: a synthetic `record-<set>.pth` is written through the reference's `LossRecorder` into a temporary job directory and only
`available_results` in the reference's `cvae` namespace is replaced, by a stub that reports the recorder present (the import stubs
for torchvision / setproctitle are those of oracle/gen_golden.py).  What the method stores - accuracy, auc, tpr, fpr, precision -
is taken from `net.testing`.  It stores neither the thresholds nor the confusion counts, so every row is ALSO computed by the loop
of cvae.py:2003-2015 written out below over the reference's `roc_curve`, `batch_dist_measures` and `predict_after_evaluate`; the
two are asserted equal.  The ops-level cases (ties_2000, one_correct_300) have score rows only and use that loop alone.

Only data is written: the recorder tensors (fp32 (C, N) losses, `logits`, `y_true`), the reference's fp32 score rows, the
correctness masks and, per (prediction method, method), auc / tpr / fpr / thr_low / tp / fp / precision / accuracy; and per
method family the maximum error of the reference's own fp32 score rows against an fp64 evaluation of the same formulas on the
same fp32 inputs (`referr_*`: the yardstick of the device score kernel).

Input conditions (asserted here and again in tests/test_mdr_restatement.py): logit spread below 80 (no softmax term is 0 in fp32,
`hyz` has no NaN); no exact tie in the arg-max / arg-min a prediction method takes.  The ROC is one-sided (correct against
missed), so no case needs the order-free mean of the 2^-10 grid explained in tools/gen_roc_golden.py; the ties case uses that grid
quantised to 64 levels all the same.

--timing also times the reference method on the 70-row cvae case (2 prediction methods x 35 methods) at N = 10 000 on this CPU and
stores the figure in tests/golden/mdr/timing.json (the figure tools/mdr_bench.py prints beside the device time).
"""
import argparse
import collections
import json
import os
import platform
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, 'tests', 'golden', 'mdr')
KEPT = [pc / 100 for pc in range(90, 100)]                    # cvae.py:1970
SET = 'synth'
EPOCH = 7                                                     # not 0: a new model's `testing` already has an (empty) epoch 0
sys.path.insert(0, REPO)


def synth_cvae(rng, C, N, acc=.85):
    """All-class losses of a cvae-like model: the true class is (mostly) the closest / the most likely one."""
    y = rng.integers(0, C, N)
    hit = rng.random((3, N)) < acc
    onehot = np.eye(C, dtype=bool)[y].T                        # (C, N)
    zdist = rng.gamma(4., 2., (C, N)) + 6.
    zdist = np.where(onehot & hit[0], zdist - 6. * rng.random(N), zdist)
    kl = .5 * zdist + rng.gamma(2., .5, (C, N))
    cross_x = rng.gamma(9., 3., N) + 40.
    total = kl + cross_x
    iws = -total + rng.normal(0, 1., (C, N))
    iws = np.where(onehot & hit[1], iws + 5. * rng.random(N), iws)
    logits = rng.normal(0, 2., (C, N))
    logits = np.where(onehot & hit[2], logits + 4. * rng.random(N) + 1., logits)
    t = {'total': total, 'kl': kl, 'zdist': zdist, 'iws': iws, 'cross_x': np.broadcast_to(cross_x, (C, N)).copy(), 'logits': logits}
    t = {k: torch.tensor(v.astype(np.float32)) for k, v in t.items()}
    t['y_true'] = torch.tensor(y)
    return t


def synth_vib(rng, C, N, odin, acc=.9):
    y = rng.integers(0, C, N)
    onehot = np.eye(C, dtype=bool)[y].T
    hit = rng.random(N) < acc
    logits = rng.normal(0, 3., (C, N))
    logits = np.where(onehot & hit, logits + 6. * rng.random(N) + 1., logits)
    kl, cross_y = rng.gamma(3., 2., N), rng.gamma(1., 1., N)
    t = {'total': kl + cross_y, 'kl': kl, 'cross_y': cross_y, 'logits': logits}
    for name in odin:                                          # synthetic rows shaped like the real ones: a tempered max softmax
        T, eps = float(name.split('-')[1]), float(name.split('-')[2])
        z = logits / T + 50. * eps * rng.normal(0, 1., (C, N))
        e = np.exp(z - z.max(0))
        t[name] = (e / e.sum(0)).max(0)
    t = {k: torch.tensor(np.asarray(v).astype(np.float32)) for k, v in t.items()}
    t['y_true'] = torch.tensor(y)
    return t


def check_inputs(t, predict):
    """The input conditions of the module docstring."""
    logits = t['logits'].numpy()
    assert (logits.max(0) - logits.min(0)).max() < 80
    for pm, (key, best) in {'iws': ('iws', np.max), 'closest': ('zdist', np.min), 'esty': ('logits', np.max)}.items():
        if pm in predict:
            v = t[key].numpy()
            assert ((v == best(v, 0)).sum(0) == 1).all(), f'tie in {pm}'


def rows_by_the_loop(ref_roc, measures, correct, missed):
    """cvae.py:2003-2015 for one method, with the reference's roc_curve."""
    auc, fpr, tpr, thr = ref_roc(measures[correct], measures[missed], *KEPT, debug=False)
    low = np.asarray(thr['low'], np.float64)
    tp = np.array([((measures >= t) * correct).sum() for t in low], np.int32)
    fp = np.array([((measures >= t) * missed).sum() for t in low], np.int32)
    with np.errstate(invalid='ignore', divide='ignore'):
        precision = np.array([(t / (t + f)) for t, f in zip(tp, fp)], np.float64)
    return dict(auc=np.float64(auc), fpr=np.asarray(fpr, np.float64), tpr=np.asarray(tpr, np.float64), low=low, tp=tp, fp=fp,
                precision=precision)


def pack(data, pm, rows, accuracy, mask):
    for k in ('auc', 'fpr', 'tpr', 'low', 'tp', 'fp', 'precision'):
        data[f'{k}_{pm}'] = np.stack([r[k] for r in rows])
    data[f'accuracy_{pm}'] = np.float64(accuracy)
    data[f'mask_{pm}'] = np.asarray(mask, bool)


def fp64_rows(t, methods):
    """The score formulas of batch_dist_measures (cvae.py:1013-1063) in fp64 numpy on the fp32 recorder tensors."""
    def soft(v):                                              # max_c softmax_c(v), v (C, N)
        e = np.exp(v - v.max(0))
        return (e / e.sum(0)).max(0)
    f = {k: v.numpy().astype(np.float64) for k, v in t.items() if k != 'y_true'}
    out = {}
    for m in methods:
        T = float(m.split('-')[-1]) if '-' in m else 1.
        if m.startswith('odin'):
            out[m] = f[m]
        elif m == 'iws':
            out[m] = np.log(np.exp(f['iws'] - f['iws'].max(0)).sum(0)) + f['iws'].max(0) + np.log(f['iws'].shape[0])
        elif m == 'softiws':
            out[m] = soft(f['iws'])
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
    return m.split('-')[0] if not m.startswith('odin') else 'odin'


def run_reference(ref, kw, tensors, predict_methods, misclass_methods, batch=100):
    """The reference method on a reference model over a record file written by the reference's LossRecorder."""
    net = ref.ClassificationVariationalNetwork(**kw)
    N = tensors['y_true'].shape[0]
    with tempfile.TemporaryDirectory() as job:
        sdir = os.path.join(job, 'samples', '{:04d}'.format(EPOCH))
        os.makedirs(sdir)
        rec = ref.LossRecorder(batch)
        for i in range(0, N, batch):
            rec.append_batch(**{k: v[..., i:i + batch] for k, v in tensors.items()})
        rec.save(os.path.join(sdir, f'record-{SET}.pth'))
        net.saved_dir, net.training_parameters['set'] = job, SET
        present = {SET: {'where': {'recorders': True}, 'recorders': collections.defaultdict(lambda: True)}}
        real = ref.available_results
        ref.available_results = lambda *a, **k: {EPOCH: present}
        try:
            t0 = time.perf_counter()
            net.misclassification_detection_rates(predict_methods=predict_methods, misclass_methods=misclass_methods)
            dt = time.perf_counter() - t0
        finally:
            ref.available_results = real
    return net, dt


def model_case(ref, kw, tensors, predict_methods, misclass_methods):
    net, _ = run_reference(ref, kw, tensors, predict_methods, misclass_methods)
    predict = list(net.predict_methods) if predict_methods == 'all' else list(predict_methods)
    stored = net.testing[EPOCH]
    methods = [m for m in stored[predict[0]] if isinstance(stored[predict[0]][m], dict)]
    check_inputs(tensors, predict)
    losses = {k: v for k, v in tensors.items() if k not in ('logits', 'y_true')}
    logits, y = tensors['logits'].T, tensors['y_true']
    scores = net.batch_dist_measures(logits, losses, methods, to_cpu=True)
    data = {f'rec_{k}': v.numpy() for k, v in tensors.items()}
    data.update(methods=np.array(methods), predict=np.array(predict), kept=np.asarray(KEPT),
                scores=np.stack([scores[m].numpy() for m in methods]), type=np.array(kw['type']))
    assert data['scores'].dtype == np.float32
    for pm in predict:
        y_ = net.predict_after_evaluate(logits, losses, method=pm)
        correct, missed = np.asarray(y_ == y), np.asarray(y_ != y)
        rows = [rows_by_the_loop(ref.roc_curve, np.asarray(scores[m]), correct, missed) for m in methods]
        for m, r in zip(methods, rows):                        # the method's own results are the loop's
            s = stored[pm][m]
            assert s['n'] == len(y) and s['auc'] == r['auc'] and s['tpr'] == list(r['tpr']) and s['fpr'] == list(r['fpr'])
            assert np.array_equal(np.asarray(s['precision'], np.float64), r['precision'], equal_nan=True)
        assert stored[pm]['accuracy'] == correct.sum() / len(y)
        pack(data, pm, rows, stored[pm]['accuracy'], correct)
    exact = fp64_rows(tensors, methods)
    err = collections.defaultdict(float)
    for m, row in zip(methods, data['scores']):
        err[family(m)] = max(err[family(m)], float(np.abs(row.astype(np.float64) - exact[m]).max()))
    data.update(referr_names=np.array(sorted(err)), referr_values=np.array([err[k] for k in sorted(err)]))
    return data


def ops_case(ref, scores, correct):
    scores, correct = np.asarray(scores, np.float32), np.asarray(correct, bool)
    data = dict(methods=np.array([f'row{i}' for i in range(len(scores))]), predict=np.array(['given']), kept=np.asarray(KEPT),
                scores=scores, type=np.array('ops'))
    pack(data, 'given', [rows_by_the_loop(ref.roc_curve, row, correct, ~correct) for row in scores], correct.mean(), correct)
    return data


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='checkout of the reference (the directory that holds cvae.py)')
    ap.add_argument('--timing', action='store_true')
    a = ap.parse_args()
    from oracle import gen_golden
    from oracle.cases import get_case
    from tools.gen_roc_golden import grid_scores
    gen_golden.REF = os.path.abspath(a.reference)
    gen_golden.import_reference()
    ref = sys.modules['cvae']
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20241016)
    cvae_kw, vib_kw = dict(get_case('c1_n16_mlp')['net'], gamma=0.), dict(get_case('eb2_n8_vib_L2')['net'])
    # gamma = 0: no classifier head, the prediction methods are the table's ('iws', 'closest')
    odin = ['odin-1-0.0000', 'odin-1-0.0040', 'odin-10-0.0012', 'odin-100-0.0020', 'odin-1000-0.0040']
    cases = {
        'cvae_1500': model_case(ref, cvae_kw, synth_cvae(rng, 10, 1500), 'all', 'all'),
        'cvae_257': model_case(ref, cvae_kw, synth_cvae(rng, 10, 257, acc=.7), 'all', 'all'),
        'vib_1200': model_case(ref, vib_kw, synth_vib(rng, 10, 1200, odin), 'all', ['baseline', 'logits', 'hyz'] + odin),
    }
    ties = np.stack([grid_scores(rng, 2000, .3 * i, 1., levels=64) for i in range(3)])
    cases['ties_2000'] = ops_case(ref, ties, rng.random(2000) < .5 + .1 * ties[0])
    one = np.zeros(300, bool)
    one[137] = True
    cases['one_correct_300'] = ops_case(ref, rng.standard_normal((2, 300)), one)
    for name, data in cases.items():
        np.savez_compressed(os.path.join(OUT, name + '.npz'), **data)
        pm = str(data['predict'][0])
        print(f'{name:18s} {len(data["methods"]):3d} rows x {len(data["predict"])} prediction methods, accuracy[{pm}] '
              f'{float(data[f"accuracy_{pm}"]):.4f}, auc[0] {data[f"auc_{pm}"][0]:.4f}, '
              f'{os.path.getsize(os.path.join(OUT, name + ".npz"))} bytes')
        if 'referr_names' in data:
            print('    reference fp32 error:', dict(zip(data['referr_names'].tolist(), data['referr_values'].tolist())))
    if a.timing:
        tensors = synth_cvae(np.random.default_rng(7), 10, 10000)
        net, dt = run_reference(ref, cvae_kw, tensors, 'all', 'all')
        rows = sum(len([m for m in v if isinstance(v[m], dict)]) for v in net.testing[EPOCH].values())
        json.dump({'what': 'reference misclassification_detection_rates (cvae.py:1913-2079) record file included, one CPU '
                           'process', 'rows': rows, 'n': 10000, 'seconds': dt, 'machine': platform.machine(),
                   'python': platform.python_version(), 'numpy': np.__version__, 'torch': torch.__version__},
                  open(os.path.join(OUT, 'timing.json'), 'w'), indent=1)
        print(f'reference, {rows} rows of 10000: {dt:.3f} s')


if __name__ == '__main__':
    main()
