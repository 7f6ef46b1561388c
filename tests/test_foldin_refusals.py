"""The LDS refusals of the four fold-in families (pcr_fold.hip): a rank whose LDS vectors alone exceed a CU's 160 KiB is refused
with PCR_ERR_UNSUPPORTED and an exact text, before the launch, and the process serves the next call.

The rank of each case is derived here from the kernels' byte formulas (fold_small_bytes of pcr_foldin.h; ridge_direct_bytes,
ridge_cg_bytes of pcr_ridge.h; nnls_cg_bytes of pcr_nnls.h): the smallest one the formula refuses, and the test holds the rank
below it on the accepted side of the formula.  One user or item with 1 rating, d2 = 4, both precisions.  The texts were recorded
from the library as it was before the fold-in families moved into a unit of their own.

Refusals this file cannot reach (NOTES.md, "Fold-in is a translation unit of its own"): the nnls direct form's (the direct form
exists up to rank 112 only, where it fits), item fold-in's 1 GiB scratch bound (an item of tens of millions of raters), and the
"launch class outside the kernel's tile range" state errors (the plan never builds such a class)."""
import numpy as np
import pytest

import primalcr_amd as pcr

ERR_UNSUPPORTED = -7
LDS_CU = 160 * 1024
D2 = 4
PREC = {"F64": (pcr.PCR_F64, 8), "F32": (pcr.PCR_F32, 4)}
ONE = (np.array([0, 1], np.int64), np.array([2], np.int32), np.array([3.0]))      # one row with one rating, on row 2 of the factor


def carve(n, elt):
    return (n * elt + 15) & ~15


def ld_of(k):
    return (k + 3) & ~3


def small_bytes(k, elt, block=64):
    """fold_small_bytes(ld, block, elt): a 1-rating row takes the one-wave form."""
    ld, waves = ld_of(k), block // 64
    return carve(ld, elt) + carve(waves + 1, 8) + 7 * carve(ld, 8) + carve(waves * ld, 8)


def ridge_direct_bytes(k, elt):
    """ridge_direct_bytes(mp = 16, ld, block = 64): 1 rating at rank k >= 1 is the dual form, one tile, one wave."""
    mp, block, tile = 16, 64, 16 * 17
    stage, tiles = carve(16 * (mp + 1), 8), carve(tile, 8)
    return carve(8, 8) + carve(block // 16, 8) + carve(16, 8) + 3 * carve(mp, 8) + carve(max(mp, ld_of(k)), 8) + carve(mp, 4) + max(stage, tiles)


def ridge_cg_bytes(k, elt):
    return carve(8, 8) + carve(16, 8) + 4 * carve(ld_of(k), 8) + carve(256, 8) + carve(256, 4)


def nnls_cg_bytes(k, elt):
    ld = ld_of(k)
    return carve(8, 8) + carve(16, 8) + carve(8, 8) + carve(8, 4) + 5 * carve(ld, 8) + carve(ld, 4) + carve(256, 8) + carve(256, 4)


def first_refused(nbytes, elt):
    """The smallest rank whose nbytes(k, elt) exceeds the CU's LDS (nbytes is non-decreasing in k)."""
    lo, hi = 1, 1 << 20
    assert nbytes(lo, elt) <= LDS_CU < nbytes(hi, elt)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if nbytes(mid, elt) > LDS_CU:
            hi = mid
        else:
            lo = mid
    return hi


def factor(rows, k):
    return np.random.default_rng(3).normal(size=(rows, k)) / np.sqrt(k)


def fold_users(k, dtype):
    return pcr.fold_in(factor(D2, k), ONE, 0.1, steps=1, dtype=dtype)


def fold_items(k, dtype):
    train = (np.array([0, 2, 4, 6], np.int64), np.array([0, 1, 1, 3, 0, 2], np.int32), np.array([1.0, 2.0, 3.0, 1.0, 2.0, 5.0]))
    return pcr.fold_in_items(factor(3, k), factor(D2, k), train, ONE, 0.1, steps=1, dtype=dtype)


def fold_ridge(k, dtype):
    return pcr.fold_in_ridge(factor(D2, k), ONE, 0.1, dtype=dtype)


def fold_ridge_cg(k, dtype):
    with pcr.tuned(ridge_form="cg"):
        return pcr.fold_in_ridge(factor(D2, k), ONE, 0.1, dtype=dtype)


def fold_nnls(k, dtype):
    return pcr.fold_in_nnls(factor(D2, k), ONE, 0.1, dtype=dtype)


# family: (the call, the bytes that refuse it, the text at rank k)
CASES = {
    "foldin": (fold_users, small_bytes, lambda k: f"fold-in: rank {k} (with 1 rating levels) is too large for the kernel's LDS"),
    "itemfold": (fold_items, small_bytes,
                 lambda k: f"item fold-in: rank {k} is too large for the LDS of the workgroup form of items of up to {pcr.PCR_ITEMFOLD_WAVE_MAX} raters"),
    "ridge_direct": (fold_ridge, ridge_direct_bytes, lambda k: f"ridge fold-in: rank {k} is too large for the direct forms' LDS"),
    "ridge_cg": (fold_ridge_cg, ridge_cg_bytes, lambda k: f"ridge fold-in: rank {k} is too large for the CG form's LDS"),
    "nnls_cg": (fold_nnls, nnls_cg_bytes, lambda k: f"nnls fold-in: rank {k} is too large for the CG form's LDS"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("pname", list(PREC))
@pytest.mark.parametrize("family", list(CASES))
def test_a_rank_beyond_the_lds_is_refused_with_its_text_and_the_next_call_runs(family, pname):
    call, nbytes, text = CASES[family]
    dtype, elt = PREC[pname]
    k = first_refused(nbytes, elt)
    assert nbytes(k - 1, elt) <= LDS_CU < nbytes(k, elt)
    with pytest.raises(pcr.PcrError) as e:
        call(k, dtype)
    assert str(e.value) == f"libprimalcr error {ERR_UNSUPPORTED}: {text(k)}"
    rows, stats = call(5, dtype)
    assert rows.shape == (1, 5) and np.isfinite(rows).all()
