"""The readers of the device status words (ops.wim_check_status, knn_check_status, maha_check_status, ic_check_status,
ssim_check_status, kde_check_status) on host integers and CPU tensors.  No GPU, nothing is launched.

READERS pins, per reader, the exception type and message of every bit it knows, in the order in which they win when several are
set, as the readers raised them while each family had a copy of its own of the reading loop."""
import itertools
import re

import pytest
import torch

from jvae_hip import ops
from jvae_hip.lib import JvaeHipError

# reader -> ([(bit, exception, message) in winning order], bits it ignores, whether it returns the word)
READERS = {
    'wim_check_status': ([(1, JvaeHipError, r'a label outside \[0, C\) was met by wim_scores, prior_sample or aggregate_scores \(the rows '
                                            r'of that sample are NaN\)')], (2, 4, 1 << 16), False),
    'knn_check_status': ([(2, ValueError, r'knn: a query row with a non-finite element was met \(its distances are NaN, its indices -1\)'),
                          (1, ValueError, r'knn: a bank row at a non-finite distance was met \(it is in no list\)')], (4, 1 << 16), False),
    'maha_check_status': ([(4, ValueError, r'maha: a query row with a non-finite element was met \(its scores are NaN, its class -1\)'),
                           (1, ValueError, r'maha: a bank row with a label outside \[0, num_classes\) was met \(it is in no sum\)'),
                           (2, ValueError, r'maha: a bank row with a non-finite element was met \(it is in no sum\)')], (8, 1 << 16), False),
    'ic_check_status': ([(2, ValueError, r'image_code_length: an image with a non-finite pixel was met \(its bits are NaN, its choice '
                                         r'-1\)')], (1, 4, 1 << 16), True),
    'ssim_check_status': ([(1, ValueError, r'ssim: an image with a non-finite pixel was met \(the scores of all its draws are NaN\)'),
                           (2, ValueError, r'ssim: a reconstruction with a non-finite pixel was met \(its scores are NaN\)')],
                          (4, 1 << 16), True),
    'kde_check_status': ([(1 << 16, JvaeHipError, r'kde_logdensity: a query with a non-finite statistic, or one so far from the bank that '
                                                  r'its square overflows fp32, was met \(its rows hold -inf / NaN\)')],
                         (1, 2, 1 << 8, 1 << 15, 1 << 17), False),
}


def test_the_bits_are_the_constants():
    assert (ops.KNN_STATUS_BANK, ops.KNN_STATUS_QUERY) == (1, 2)
    assert (ops.MAHA_STATUS_LABEL, ops.MAHA_STATUS_BANK, ops.MAHA_STATUS_QUERY) == (1, 2, 4)
    assert (ops.IC_STATUS_INEXACT, ops.IC_STATUS_NONFINITE) == (1, 2)
    assert (ops.SSIM_STATUS_X, ops.SSIM_STATUS_Y, ops.DOSE_STATUS_QUERY) == (1, 2, 1 << 16)


@pytest.mark.parametrize('reader', list(READERS))
def test_every_bit_and_every_pair(reader):
    check = getattr(ops, reader)
    known, ignored, _ = READERS[reader]
    for bit, exc, message in known:
        for word in (bit, bit | ignored[0], bit | ignored[-1]):
            with pytest.raises(exc, match=message) as err:
                check(word)
            assert type(err.value) is exc
    for (bit, exc, message), (later, _, loses) in itertools.combinations(known, 2):        # the earlier one of the table wins
        with pytest.raises(exc, match=message) as err:
            check(bit | later)
        assert not re.search(loses, str(err.value))
    with pytest.raises(known[0][1], match=known[0][2]):
        check(sum(bit for bit, _, _ in known) | sum(ignored))


@pytest.mark.parametrize('reader', list(READERS))
def test_zero_and_ignored_bits_are_silent(reader):
    check = getattr(ops, reader)
    _, ignored, returns_word = READERS[reader]
    for word in (0,) + tuple(ignored) + (sum(ignored),):
        got = check(word)
        assert got == word if returns_word else got is None
    assert check() == 0 if returns_word else check() is None          # no default word exists in a process without a device
    assert ops.ic_check_status(ops.IC_STATUS_INEXACT) == 1


@pytest.mark.parametrize('reader', list(READERS))
@pytest.mark.parametrize('shape', [(1,), (3,), (1, 2)])
def test_a_tensor_word_is_cleared_by_the_read(reader, shape):
    check = getattr(ops, reader)
    known, ignored, returns_word = READERS[reader]
    for bit, exc, message in known:
        word = torch.zeros(shape, dtype=torch.int32)
        word.reshape(-1)[0] = bit | ignored[0]
        with pytest.raises(exc, match=message):
            check(word)
        assert int(word.reshape(-1)[0]) == 0                          # read and cleared ...
        got = check(word)                                             # ... so a second read is silent
        assert got == 0 if returns_word else got is None
    word = torch.tensor([ignored[0]], dtype=torch.int32)              # a word that raises nothing is cleared as well
    got = check(word)
    assert (got == ignored[0] if returns_word else got is None) and int(word) == 0
