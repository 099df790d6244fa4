"""The device status words of the flagging ops, one mechanism for six families (ops._status_word, ops._read_status): per family
the smallest input the op is documented to flag and survive - one or two launches on a handful of elements."""
import pytest
import torch

from jvae_hip import ops
from jvae_hip.lib import JvaeHipError

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')


def dev(values, dtype=torch.float32):
    return torch.tensor(values, dtype=dtype, device=DEV)


def run_knn(status):
    bank, sq = ops.knn_bank(dev([[1.]]))
    ops.knn(dev([[NAN]]), bank, sq, 1, status=status)


def run_maha(status):
    clean = torch.zeros(1, dtype=torch.int32, device=DEV)
    moments = ops.maha_moments(dev([[0.], [1.], [3.], [5.]]), dev([0, 0, 1, 1], torch.int64), 2, status=clean)
    assert int(clean) == 0
    ops.maha_scores(dev([[NAN]]), ops.maha_fit(moments), status=status)


def run_ic(status):
    ops.image_code_length(dev([[[[NAN]]]]), status=status)


def run_ssim(status):
    x = torch.full((1, 1, 11, 11), .5, device=DEV)
    x[0, 0, 5, 5] = NAN
    ops.ssim(x, torch.full((1, 1, 1, 11, 11), .5, device=DEV), status=status)


def run_kde(status):
    ops.kde_logdensity(dev([[NAN]]), ops.kde_fit(dev([[0., 1.]])), status=status)


def run_wim(status):
    ops.wim_scores([(dev([[0.]]), 1., None)], dev([1], torch.int64), [(0, 'Y')], status=status)


# family -> (the op on its flagging input, the default word, the reader, the bit, the reader's exception, its message)
FAMILIES = {'knn': (run_knn, ops.knn_status, ops.knn_check_status, ops.KNN_STATUS_QUERY, ValueError, 'knn: a query row with a non-finite'),
            'maha': (run_maha, ops.maha_status, ops.maha_check_status, ops.MAHA_STATUS_QUERY, ValueError,
                     'maha: a query row with a non-finite'),
            'ic': (run_ic, ops.ic_status, ops.ic_check_status, ops.IC_STATUS_NONFINITE, ValueError,
                   'image_code_length: an image with a non-finite pixel'),
            'ssim': (run_ssim, ops.ssim_status, ops.ssim_check_status, ops.SSIM_STATUS_X, ValueError,
                     'ssim: an image with a non-finite pixel'),
            'kde': (run_kde, ops.kde_status, ops.kde_check_status, ops.DOSE_STATUS_QUERY, JvaeHipError,
                    'kde_logdensity: a query with a non-finite statistic'),
            'wim': (run_wim, ops.wim_status, ops.wim_check_status, 1, JvaeHipError, r'a label outside \[0, C\) was met by wim_scores')}
# what each op says of a word that is no int32 tensor with an element on its device
REFUSALS = {'knn': 'knn: an int32 status word on the device of the rows expected',
            'maha': 'maha_scores: an int32 status word on the device of the rows expected',
            'ic': 'image_code_length: an int32 status word on the device of the images expected',
            'ssim': 'ssim: an int32 status word on the device of the images expected',
            'kde': 'kde_logdensity: an int32 status word on the device of the statistics expected',
            'wim': 'wim_scores: an int32 status word on the device of the sources expected'}


def bad_words():
    return [torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.float32, device=DEV),
            torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32), 0, [0]]


@pytest.mark.parametrize('family', list(FAMILIES))
def test_default_word_and_own_word(family):
    run, default_word, check, bit, exc, message = FAMILIES[family]
    device = torch.device(DEV)
    default = default_word(device)
    assert default_word(device) is default and default.dtype == torch.int32 and default.numel() == 1 and default.device == device
    others = [FAMILIES[f][1](device) for f in FAMILIES if f != family]
    assert all(o is not default and o.data_ptr() != default.data_ptr() for o in others)       # a word per family
    default.zero_()                                            # whatever an earlier test left unread
    run(None)                                                  # without status=: the default word takes the flag
    assert int(default) & bit
    with pytest.raises(exc, match=message):
        check()
    assert int(default) == 0
    check()                                                    # read and cleared: a second read is silent
    own = torch.zeros(1, dtype=torch.int32, device=DEV)
    run(own)                                                   # a caller's word takes the flag, the default word stays clear
    assert int(own) & bit and int(default) == 0
    check()
    with pytest.raises(exc, match=message):
        check(own)
    assert int(own) == 0
    for word in bad_words():
        with pytest.raises(JvaeHipError, match=REFUSALS[family]):
            run(word)
    assert int(default) == 0


def test_the_other_ops_of_the_wim_family_refuse_a_bad_word():
    calls = {'scod_scores': (lambda s: ops.scod_scores([('zero', None, None, 'zero', None, None, 1.)], None, 1, 1, status=s), 'sources'),
             'prior_sample': (lambda s: ops.prior_sample(dev([[0.]]), None, dev([[0.]]), None, status=s), 'noise'),
             'aggregate_scores': (lambda s: ops.aggregate_scores([dev([[0.]])], 'mean', temps=(1.,), status=s), 'sources'),
             'maha_moments': (lambda s: ops.maha_moments(dev([[0.], [1.]]), dev([0, 0], torch.int64), 1, status=s), 'rows')}
    for what, (call, noun) in calls.items():
        for word in bad_words():
            with pytest.raises(JvaeHipError, match=f'{what}: an int32 status word on the device of the {noun} expected'):
                call(word)
