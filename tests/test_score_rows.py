"""module/score_rows.py against the frozen restatement of tests/score_rows_cases.py, without a GPU: `parse()` gives every name the
(source, kind, const, roc_mode) it had in the five places that used to encode it, and the plain call through the catalogue is,
bit for bit, the `if` chain it replaced."""
import pytest
import torch

import score_rows_cases as S

N = 70
_models = {}


def model(type_):
    if type_ not in _models:
        _models[type_] = S.build_model(type_)
    return _models[type_]


@pytest.mark.parametrize('type_', list(S.MODEL_CASES))
def test_parse_gives_the_frozen_table(type_):
    from module import score_rows
    traits = score_rows.traits_of(model(type_))
    table = S.table()
    assert set(table) == set(S.all_names()) | set(S.MALFORMED)
    for name, per_type in table.items():
        want = per_type[type_]
        if isinstance(want, dict):
            with pytest.raises({'ValueError': ValueError, 'NotImplementedError': NotImplementedError}[want['raises']]):
                score_rows.parse(name, traits)
            continue
        row = score_rows.parse(name, traits)
        mode = list(row.roc_mode) if isinstance(row.roc_mode, tuple) else row.roc_mode
        assert [row.source, row.kind, row.const, mode] == want, (name, type_)
        assert type(row.const) is type(want[2])


def test_malformed_names_raise_what_they_raised():
    from module import score_rows
    traits = score_rows.traits_of(model('cvae'))
    for name, exc in S.MALFORMED.items():
        with pytest.raises(exc):
            score_rows.parse(name, traits)
    with pytest.raises(ValueError, match='x and y in 1 .. 255'):
        score_rows.parse('iws-a-0-1', traits)
    with pytest.raises(NotImplementedError, match='mse~: WIM score outside this build'):
        score_rows.parse('mse~', traits)
    with pytest.raises(NotImplementedError, match='fisher_rao: OOD method outside this build'):
        model('cvae').batch_dist_measures(None, {}, ['fisher_rao'])
    with pytest.raises(ValueError, match='softmax: unknown misclassification method'):
        score_rows.parse('softmax', traits, misclass=True)
    with pytest.raises(NotImplementedError, match='zdist~: OOD method outside this build'):      # only a WIMJob has these rows
        model('cvae').batch_dist_measures(None, S.inputs(10, N, 1., 0, [])[1], ['zdist~'])


@pytest.mark.filterwarnings('ignore:std')                   # C = 1: the deviation of one class is NaN, as in the chain
@pytest.mark.parametrize('spread', (1., 3000.))
@pytest.mark.parametrize('C', (1, 2, 10))
@pytest.mark.parametrize('type_', list(S.MODEL_CASES))
def test_plain_call_is_the_frozen_chain_bit_for_bit(type_, C, spread):
    from module import score_rows
    net = model(type_)
    traits = score_rows.traits_of(net)
    names = [m for m, per_type in S.table().items() if not isinstance(per_type[type_], dict)]
    logits, losses = S.inputs(C, N, spread, C, names, per_class=traits.losses_might_be_computed_for_each_class)
    want, fails = {}, {}
    for m in names:
        if m[-1] not in '~@':
            try:
                want[m] = S.frozen_plain(m, logits, losses, traits)
            except (IndexError, RuntimeError, KeyError) as err:
                fails[m] = type(err)      # a class-axis row of an (N,) loss; `odin-T-eps-a-x-y`, whose base is cut to `odin`
    got = net.batch_dist_measures(logits, losses, list(want))
    assert list(got) == list(want) and len(want) > 100
    for m in want:
        assert got[m].dtype == want[m].dtype and got[m].numpy().tobytes() == want[m].numpy().tobytes(), (m, type_)
    for m, err in fails.items():                            # the catalogue fails the way the chain did
        with pytest.raises(err):
            net.batch_dist_measures(logits, losses, [m])
    if type_ == 'cvae' and 'total' in losses:
        assert str(float(got['elbo'][5])) == '-0.0' and str(float(got['sum'][5])) == str(float(S.frozen_plain('sum', logits, losses, traits)[5]))


@pytest.mark.parametrize('C', (1, 2, 10))
def test_wim_rows_are_the_frozen_expressions_bit_for_bit(C):
    from jvae_compat.wim import WIMJob
    from oracle.cases import get_case
    job = WIMJob(**dict(get_case('c1_n16_mlp')['net'], gamma=0.))
    for spread in (1., 3000.):
        logits, losses = S.inputs(C, N, spread, C, [])
        got = job.batch_dist_measures(logits, losses, S.WIM_NAMES + ['elbo', 'zdist-2s'])
        for m in S.WIM_NAMES + ['elbo', 'zdist-2s']:
            want = S.frozen_row(m, logits, losses, job)
            assert got[m].numpy().tobytes() == want.numpy().tobytes(), m
    vae = WIMJob(**dict(get_case('ea2_n8_vae_L3')['net']))
    with pytest.raises(NotImplementedError, match='class-conditional'):
        vae.batch_dist_measures(None, losses, ['zdist~'])
