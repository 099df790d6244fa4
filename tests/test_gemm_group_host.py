"""No GPU: the argument checks of the grouped dense entry points (jvae_gemm_group_f32, jvae_splitk_fold_group_f32).  Every call
here is refused (or has nothing to do) before a launch, so the operand addresses are never read."""
import ctypes

import pytest

from jvae_hip import lib as L

EINVAL, ENOTSUP = -1, -2
BASE = 0x10000000            # stand-in device addresses, 16-byte aligned; outputs 1 MiB apart


def _desc(d, i, M=8, N=8, K=8, out=None):
    d.M, d.N, d.K, d.batch = M, N, K, 1
    d.A, d.sAm, d.sAk, d.sAb = BASE, K, 1, 0
    d.B, d.sBk, d.sBn, d.sBb = BASE + (1 << 20), N, 1, 0
    d.C, d.sCm, d.sCn, d.sCb = (BASE + ((2 + i) << 20)) if out is None else out, N, 1, 0
    d.bias, d.bias_mode, d.flags, d.splitk = None, 0, 0, 1


def _group(n, **kw):
    arr = (L.GemmDesc * max(n, 1))()
    for i in range(n):
        _desc(arr[i], i, **kw)
    return arr


def test_struct_layout_matches_the_header():
    """The C struct: 4 ints, 3 x (pointer + 3 longs), pointer + 3 ints, int, long, pointer with natural alignment."""
    assert ctypes.sizeof(L.GemmDesc) == 16 + 3 * 32 + 8 + 12 + 4 + 8 + 8
    assert L.GemmDesc.sCsplit.offset == 136 and L.GemmDesc.splits.offset == 144
    assert ctypes.sizeof(L.FoldDesc) == 24 + 8 + 8 + 16
    assert L.FoldDesc.MN.offset == 32


def test_an_empty_group_is_a_no_op():
    lib = L.load()
    assert lib.jvae_gemm_group_f32(None, 0, None) == 0
    assert lib.jvae_splitk_fold_group_f32(None, 0, None) == 0
    arr = _group(2, M=0)                     # empty products are dropped, as jvae_gemm_f32 does
    assert lib.jvae_gemm_group_f32(arr, 2, None) == 0


def test_more_than_eight_products_are_refused():
    lib = L.load()
    assert lib.jvae_gemm_group_f32(_group(9), 9, None) == ENOTSUP
    assert lib.jvae_splitk_fold_group_f32((L.FoldDesc * 9)(), 9, None) == ENOTSUP
    assert lib.jvae_gemm_group_f32(None, 2, None) == EINVAL
    assert lib.jvae_gemm_group_f32(_group(1), -1, None) == EINVAL


@pytest.mark.parametrize('field', ['A', 'B', 'C'])
def test_a_null_operand_is_refused(field):
    arr = _group(3)
    setattr(arr[1], field, None)
    assert L.load().jvae_gemm_group_f32(arr, 3, None) == EINVAL


def test_descriptors_that_the_single_entry_refuses_are_refused():
    lib = L.load()
    arr = _group(2)
    arr[1].bias_mode = 1                     # a bias mode without a bias
    assert lib.jvae_gemm_group_f32(arr, 2, None) == EINVAL
    arr = _group(2, K=128)
    arr[0].flags, arr[0].splitk = 2, 2       # ReLU cannot follow a partial sum
    assert lib.jvae_gemm_group_f32(arr, 2, None) == EINVAL
    arr = _group(2, K=128)
    arr[0].want_splits, arr[0].sCsplit = 2, 64          # the split form has to report its number of pieces
    assert lib.jvae_gemm_group_f32(arr, 2, None) == EINVAL


def test_overlapping_outputs_are_refused():
    lib = L.load()
    arr = _group(3)
    arr[2].C = arr[0].C                      # the same output twice
    assert lib.jvae_gemm_group_f32(arr, 3, None) == EINVAL
    arr = _group(2)
    arr[1].C = arr[0].C + 4 * 63             # the last element of the first output
    assert lib.jvae_gemm_group_f32(arr, 2, None) == EINVAL
    made = (ctypes.c_int * 1)(-1)
    arr = _group(2, K=128)
    arr[0].want_splits, arr[0].sCsplit = 4, 1 << 18     # slices 1 MiB apart: the fourth reaches into the second product's output
    arr[0].splits = ctypes.cast(made, ctypes.POINTER(ctypes.c_int))
    assert lib.jvae_gemm_group_f32(arr, 2, None) == EINVAL
    assert made[0] == 0                      # nothing was launched, nothing is reported


def test_fold_group_checks():
    lib = L.load()
    arr = (L.FoldDesc * 2)()
    for i, d in enumerate(arr):
        d.part, d.bias, d.y = BASE, None, BASE + ((1 + i) << 20)
        d.S, d.MN, d.N, d.relu, d.accumulate = 2, 64, 8, 0, 0
    arr[1].part = None
    assert lib.jvae_splitk_fold_group_f32(arr, 2, None) == EINVAL
    arr[1].part = BASE
    arr[1].S = 0
    assert lib.jvae_splitk_fold_group_f32(arr, 2, None) == EINVAL
    arr[1].S = 2
    arr[1].y = arr[0].y + 4 * 63
    assert lib.jvae_splitk_fold_group_f32(arr, 2, None) == EINVAL
    arr[0].MN = arr[1].MN = 0                # nothing to fold
    assert lib.jvae_splitk_fold_group_f32(arr, 2, None) == 0
