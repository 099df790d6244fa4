#!/usr/bin/env python3
"""Write tests/golden/wim/*.npz: inputs and the REFERENCE's WIM score rows, and one both-prior evaluation of a small model.

    python tools/gen_wim_golden.py --reference <checkout of moxime/joint-vae>

Score cases `scores_C<C>_N<N>` for (C, N) in CASES: synthetic all-class losses kl, zdist, iws, total (C, N) fp32, their (N,)
values under the alternate prior, estimated labels y_est, and the 16 rows {kl, zdist, iws, elbo} x {~, @, ~@} + soft*~ that the
reference's `WIMJob.batch_dist_measures` (ft/wim.py:132-201) makes of them.
Route (stored in every file as `route`): 'reference' - the reference's own `WIMJob`, instantiated on a tiny model with the import
placeholders of oracle/gen_golden.py, and its method called on the tensors; 'formulas' - only when the reference's `ft` package
cannot be imported: the table of the method's docstring evaluated in numpy fp32.

`referr_*`: per family the maximum error of those fp32 rows against an fp64 evaluation of the same formulas on the same fp32
inputs - the yardstick the device kernel is held to (4 x, as tests/test_7_mdr_gpu.py does).  The families are the KINDS of row,
pooled over the four losses: '~' and '~@' (a gather, one fp32 subtraction: exact in any order, the error is that of the final
rounding alone and the rows are compared bit for bit), 'soft~' (the four softmax gathers) and '@' (the four log-sum-exp
differences).  Pooled, because the smallest case has ONE sample: a single fp32 result lies within a small fraction of an ulp
of its fp64 value too often for its own error to be a yardstick.

The one case above 512 samples, (128, 1500), tiles 300 distinct columns of class-axis losses (sample n has those of sample
n % 300; the labels and the alternate losses are drawn per sample): a sample is scored on its own, the tiling only lets the file
compress below the size limit for committed files while N keeps its six workgroups and its ragged last one.

Input conditions (asserted here and again in tests/test_wim_restatement.py): per sample the spread over the classes of every
f * loss is below 80, so no softmax term underflows in fp32; y_est in [0, C).

Model case `model_e2_n8_L3`: geometry `e2_n8_L3` of oracle/cases.py, deterministic weights (oracle/det_init.py; the prior's
tensors by their `encoder.prior.*` keys), alternate prior of WIM_CASES['w2_n8'], N = 8, L = 3, eval mode: the reference's
all-class evaluate(x) under each prior with the SAME injected epsilon; every loss of both runs (`orig.*`, `alt.*`),
y_est (argmin_c kl for even samples, n mod C for odd ones) and the 16 rows.  Only data is written.
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, 'tests', 'golden', 'wim')
sys.path.insert(0, REPO)

CASES = [(1, 65), (2, 64), (10, 257), (100, 63), (128, 1500), (10, 1)]
FACTORS = {'kl': -1., 'zdist': -.5, 'iws': 1., 'elbo': 1.}
METHODS = [k + s for k in FACTORS for s in ('~', '@', '~@')] + ['soft' + k + '~' for k in FACTORS]
MAX_SPREAD = 80.


def family(m):
    if m.endswith('~@'):
        return '~@'
    if m.endswith('@'):
        return '@'
    return 'soft~' if m.startswith('soft') else '~'


PERIOD = 300            # N > 512: sample n shares its (C,) class-axis losses with sample n % PERIOD (see the module docstring)


def synth(rng, C, N):
    """All-class losses of a cvae-like model and their values under a single alternate prior; y_est mostly the closest class."""
    M = N if N <= 512 else PERIOD
    zdist = rng.gamma(4., 2., (C, M)) + 6.
    kl = .5 * zdist + rng.gamma(2., .5, (C, M))
    cross_x = rng.gamma(9., 3., M) + 40.
    total = kl + cross_x
    iws = -total + rng.normal(0, 1., (C, M))
    if M < N:
        col = np.arange(N) % M
        zdist, kl, total, iws, cross_x = zdist[:, col], kl[:, col], total[:, col], iws[:, col], cross_x[col]
    zdist_a = rng.gamma(4., 2., N) + 10.
    kl_a = .5 * zdist_a + rng.gamma(2., .5, N)
    total_a = kl_a + cross_x
    iws_a = -total_a + rng.normal(0, 1., N)
    y = np.where(rng.random(N) < .8, kl.argmin(0), rng.integers(0, C, N))
    t = {'kl': kl, 'zdist': zdist, 'iws': iws, 'total': total, 'kl@': kl_a, 'zdist@': zdist_a, 'iws@': iws_a, 'total@': total_a}
    t = {k: torch.tensor(np.ascontiguousarray(v, np.float32)) for k, v in t.items()}
    t['y_est_already'] = torch.tensor(y.astype(np.int64))
    return t


def check_inputs(t):
    """The input conditions of the module docstring, on numpy or torch values."""
    C = np.asarray(t['kl']).shape[0]
    y = np.asarray(t['y_est_already'])
    assert ((0 <= y) & (y < C)).all()
    for k, f in FACTORS.items():
        v = f * np.asarray(t['total' if k == 'elbo' else k], np.float64) * (-1. if k == 'elbo' else 1.)
        assert (v.max(0) - v.min(0)).max() < MAX_SPREAD, k


def formula_rows(t, dtype):
    """The table of ft/wim.py:171-192 in numpy at `dtype` on the given (fp32) tensors -> {method: (N,)}."""
    y = np.asarray(t['y_est_already'])
    n = np.arange(y.shape[0])
    out = {}
    for k, f in FACTORS.items():
        v = np.asarray(t['total' if k == 'elbo' else k]).astype(dtype)
        a = np.asarray(t[('total' if k == 'elbo' else k) + '@']).astype(dtype)
        if k == 'elbo':
            v, a = -v, -a
        x, fa = dtype(f) * v, dtype(f) * a
        top = x.max(0)
        e = np.exp(x - top)
        out[k + '~'] = x[y, n]
        out['soft' + k + '~'] = (e / e.sum(0))[y, n]
        out[k + '@'] = (np.log(e.sum(0)) + top) - fa
        out[k + '~@'] = x[y, n] - fa
    return {m: np.asarray(r, dtype) for m, r in out.items()}


def referr(rows, t):
    exact = formula_rows(t, np.float64)
    err = {}
    for m in METHODS:
        e = float(np.abs(np.asarray(rows[m], np.float64) - exact[m]).max())
        err[family(m)] = max(err.get(family(m), 0.), e)
    return err


def pack(t, rows, route):
    assert all(np.asarray(rows[m]).dtype == np.float32 for m in METHODS)
    data = {'in.' + k: np.asarray(v) for k, v in t.items()}
    data.update({'row.' + m: np.asarray(rows[m]) for m in METHODS})
    err = referr(rows, t)
    data.update(methods=np.array(METHODS), route=np.array(route), referr_names=np.array(sorted(err)),
                referr_values=np.array([err[k] for k in sorted(err)]))
    return data


def det_wim_state(job, load_det_state, det_tensor):
    """Deterministic weights of a WIM job: every tensor by its state_dict key; the original prior by its `encoder.prior.*` keys
    (the job lists the same tensors a second time as `_original_prior.*`)."""
    load_det_state(job, seed=0)
    with torch.no_grad():
        for k in ('mean', '_var_parameter'):
            t = getattr(job.encoder.prior, k)
            t.copy_(det_tensor('encoder.prior.' + k, t.shape, 0))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='checkout of the reference (the directory that holds cvae.py)')
    a = ap.parse_args()
    from oracle import gen_golden
    from oracle.cases import WIM_CASES, get_case
    from oracle.det_init import det_inputs, det_tensor, load_det_state
    gen_golden.REF = os.path.abspath(a.reference)
    gen_golden.import_reference()
    try:
        from ft.wim import WIMJob
        route = 'reference'
    except Exception as err:                                   # noqa: BLE001 - whatever the placeholders cannot satisfy
        print('the reference ft package does not import here (%r): rows from the formulas' % (err,))
        WIMJob, route = None, 'formulas'
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20261018)
    tiny = dict(get_case('c1_n16_mlp')['net'], gamma=0.)
    alt = dict(WIM_CASES['w2_n8']['alternate_prior'], num_priors=1)
    job = WIMJob(**tiny, alternate_prior=dict(alt, dim=tiny['latent_dim'])) if WIMJob else None
    for C, N in CASES:
        t = synth(rng, C, N)
        check_inputs(t)
        if job is not None:
            losses = dict(t)
            rows = {m: v.numpy() for m, v in job.batch_dist_measures(None, losses, list(METHODS)).items()}
            assert set(losses) == set(t)
        else:
            rows = formula_rows(t, np.float32)
        data = pack(t, rows, route)
        path = os.path.join(OUT, f'scores_C{C}_N{N}.npz')
        np.savez_compressed(path, **data)
        print(f'scores_C{C}_N{N}: {os.path.getsize(path)} bytes, reference fp32 error',
              dict(zip(data['referr_names'].tolist(), data['referr_values'].tolist())))
    if job is None:
        print('model case skipped: it needs the reference WIMJob')
        return
    case = get_case('e2_n8_L3')
    kw, N = case['net'], case['N']
    torch.manual_seed(0)
    job = WIMJob(**kw)
    det_wim_state(job, load_det_state, det_tensor)
    job.set_alternate_prior(**dict(alt, dim=kw['latent_dim']))
    job.eval()
    L = job.latent_sampling
    x, _, eps = det_inputs(N, kw['input_shape'], kw['num_labels'], L, kw['latent_dim'])
    runs = {}
    with torch.no_grad(), job.no_estimated_labels():
        for name in ('alt', 'orig'):
            with (job.alternate_prior if name == 'alt' else job.original_prior), gen_golden.inject_eps(eps):
                runs[name] = job.evaluate(x, batch=0)[2]
    data = {'L': np.int64(L)}
    for name, losses in runs.items():
        data.update({f'{name}.{k}': v.numpy() for k, v in losses.items()})
    n = torch.arange(N)
    y_est = torch.where(n % 2 == 0, runs['orig']['kl'].argmin(0), n % kw['num_labels'])
    t = {k: runs['orig'][k] for k in ('kl', 'zdist', 'iws', 'total')}
    t.update({k + '@': runs['alt'][k] for k in ('kl', 'zdist', 'iws', 'total')})
    t['y_est_already'] = y_est
    check_inputs(t)
    losses = dict(t)
    rows = {m: v.numpy() for m, v in job.batch_dist_measures(None, losses, list(METHODS)).items()}
    data.update(pack(t, rows, route))
    path = os.path.join(OUT, 'model_e2_n8_L3.npz')
    np.savez_compressed(path, **data)
    print(f'model_e2_n8_L3: L={L} y_est={y_est.tolist()} {os.path.getsize(path)} bytes, reference fp32 error',
          dict(zip(data['referr_names'].tolist(), data['referr_values'].tolist())))


if __name__ == '__main__':
    main()
