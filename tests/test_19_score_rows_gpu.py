"""score_rows.write_rows on the device against the frozen restatement (tests/score_rows_cases.py), under each of the three policies
its callers pass: a row left on torch is, bit for bit, the `if` chain on the device; a row given to a kernel is, bit for bit, a
direct ops.misclass_scores / ops.wim_scores call with the frozen (source, kind, const); one launch per source tensor.  C = 10 and
N = 70 (one full 64-lane tile and a ragged one), written at column 3 of a buffer with a 128-column stride."""
import pytest
import torch

import score_rows_cases as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
C, N, COL, STRIDE = 10, 70, 3, 128
POLICIES = {'score_set': ('iws', 'elbo', 'soft', 'baseline', 'hyz'), 'misclass': ('iws', 'odin'), 'out': ()}


def bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def job_and_names(type_):
    """The model, and the names of the table it has a row for: all of them but, of the 210-point ODIN grid, three points."""
    from jvae_compat.wim import WIMJob
    from oracle.cases import get_case
    if type_ == 'wim':
        return WIMJob(**dict(get_case('c1_n16_mlp')['net'], gamma=0.)).to(DEV), S.WIM_NAMES + ['elbo', 'zdist-2s', 'softkl-10', 'mse', 'iws']
    odin = ('odin-1-0.0000', 'odin-10-0.0020', 'odin-1000-0.0040')
    names = [m for m, per_type in S.table().items() if not isinstance(per_type[type_], dict) and m[-1] not in '~@'
             and (not m.startswith('odin') or (m.startswith(odin) and '-a-' not in m))]
    return S.build_model(type_).to(DEV), names


def test_policy_table():
    from cvae import ClassificationVariationalNetwork as Net
    assert Net.SCORE_SET_TORCH_ROWS == POLICIES['score_set'] and Net.MISCLASS_TORCH_ROWS == POLICIES['misclass']


@pytest.mark.filterwarnings('ignore:std')
@pytest.mark.parametrize('policy', list(POLICIES))
@pytest.mark.parametrize('type_', ('cvae', 'vae', 'vib', 'wim'))
def test_rows_under_each_policy(type_, policy, monkeypatch):
    from jvae_hip import ops
    from module import score_rows
    job, names = job_and_names(type_)
    traits = score_rows.traits_of(job)
    per_class = traits.losses_might_be_computed_for_each_class
    logits, losses = S.inputs(C, N, 3000. if policy == 'out' else 1., 7, names, per_class=per_class)
    logits, losses = logits.to(DEV), {k: v.to(DEV) for k, v in losses.items()}
    frozen = {m: S.table()[m]['cvae' if type_ == 'wim' else type_] for m in names}
    want, by_kernel = {}, {}
    for m in names:
        source, kind, const, _ = frozen[m]
        src = logits.T if source == 'logits' else losses[source]
        if m[-1] in '~@':
            continue
        by_kernel[m] = kind is not None and not S.frozen_base(m).startswith(POLICIES[policy]) \
            and src.dim() == (1 if kind in ('neg', 'id') else 2)
        if by_kernel[m]:
            want[m] = ops.misclass_scores(src[None] if src.dim() == 1 else src, [(kind, const)])[0]
            continue
        try:
            want[m] = S.frozen_plain(m, logits, losses, traits)
        except (IndexError, RuntimeError):                  # a class-axis row of an (N,) loss
            continue
    # a class-axis maximum of an (N,) loss is one number, not a row: no caller asks a model without per-class losses for it
    names = [m for m in names if m[-1] in '~@' or (m in want and want[m].shape == (N,))]
    wim = [m for m in names if m[-1] in '~@']
    if wim:
        keys = list(dict.fromkeys(frozen[m][0] for m in wim))
        factor = {frozen[m][0]: frozen[m][2] for m in wim}
        direct = ops.wim_scores([(losses[k], -factor[k] if k == 'total' else factor[k], losses[k + '@']) for k in keys],
                                losses['y_est_already'], [(keys.index(frozen[m][0]), frozen[m][1]) for m in wim])
        want.update(zip(wim, direct))
    assert any(by_kernel.values()) and (policy == 'out' or not all(by_kernel.values()))      # both routes are exercised

    launches = {'misclass': 0, 'wim': 0}
    real_m, real_w = ops.misclass_scores, ops.wim_scores
    monkeypatch.setattr(ops, 'misclass_scores', lambda *a, **k: launches.__setitem__('misclass', launches['misclass'] + 1) or real_m(*a, **k))
    monkeypatch.setattr(ops, 'wim_scores', lambda *a, **k: launches.__setitem__('wim', launches['wim'] + 1) or real_w(*a, **k))
    records = [score_rows.parse(m, traits) for m in names]
    rows = list(range(len(names), 0, -1))
    buf = torch.full((len(names) + 1, STRIDE), -7., device=DEV)
    got = score_rows.write_rows(records, rows, logits, losses, buf, COL, POLICIES[policy], job._wim_status_word)
    assert launches == {'misclass': len({frozen[m][0] for m in names if by_kernel.get(m)}), 'wim': 1 if wim else 0}
    for m, r, view in zip(names, rows, got):
        assert view.data_ptr() == buf[r, COL:].data_ptr() and view.shape == (N,), m
        assert bits(view) == bits(want[m]), (m, 'kernel' if by_kernel.get(m, True) else 'torch')
    assert bool((buf[0] == -7.).all() and (buf[:, :COL] == -7.).all() and (buf[:, COL + N:] == -7.).all())
    if wim:
        ops.wim_check_status(job._wim_status)


def test_callers_pass_their_policy(monkeypatch):
    """batch_dist_measures: nothing on torch that has a kernel row with `out`, everything without; the same rows either way as
    write_rows gives."""
    from module import score_rows
    job, names = job_and_names('cvae')
    logits, losses = S.inputs(C, N, 1., 7, names)
    logits, losses = logits.to(DEV), {k: v.to(DEV) for k, v in losses.items()}
    seen = []
    real = score_rows.write_rows
    monkeypatch.setattr(score_rows, 'write_rows', lambda *a, **k: seen.append((a, k)) or real(*a, **k))
    buf = torch.zeros((len(names), STRIDE), device=DEV)
    into = job.batch_dist_measures(logits, losses, names, out=buf, col=COL)
    plain = job.batch_dist_measures(logits, losses, names)
    assert seen[0][1].get('torch_rows', ()) == () and seen[1][1]['torch_rows'] == ('',)
    traits = score_rows.traits_of(job)
    for m in names:
        assert bits(plain[m]) == bits(S.frozen_plain(m, logits, losses, traits)), m
        assert into[m].data_ptr() == buf[names.index(m), COL:].data_ptr()
