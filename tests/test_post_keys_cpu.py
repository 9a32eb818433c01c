"""The packed key of sv_topk_indices / sv_segment_topk (csrc/sv_common.h topk_key) without a GPU: its numpy mirror
(tests/post_helpers.topk_key) orders every pair of special values and rows as include/sv_hip.h documents, and agrees with
tests/seg_loss_helpers.topk_rows, the expected result of the GPU tests.  tests/test_gpu_post_edges.py pins the kernel."""
import itertools

import numpy as np

import post_helpers as P
import seg_loss_helpers as H

ROWS = (0, 1, 2**32 - 2)  # 2^32 - 2 is the last row sv_topk_indices admits (N < 2^32 - 1)


def _raw_key(bits, row):
    """the key before NaN and zero were canonicalised: sign-flipped raw bits above ~row"""
    u = np.asarray(bits, dtype=np.uint32)
    u = np.where((u & np.uint32(P.SIGN)) != 0, ~u, u | np.uint32(P.SIGN)).astype(np.uint32)
    return (u.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xffffffff) - np.asarray(row, dtype=np.uint64))


def test_key_order_is_the_contract_order_for_every_pair_of_special_values_and_rows():
    items = list(itertools.product(P.SPECIALS.items(), ROWS))
    keys = {(name, row): int(P.topk_key([bits], [row])[0]) for (name, bits), row in items}
    for ((na, ba), ra), ((nb, bb), rb) in itertools.product(items, items):
        assert (keys[na, ra] > keys[nb, rb]) == P.contract_before(ba, ra, bb, rb), (na, ra, nb, rb)


def test_no_real_key_is_a_sentinel_and_keys_of_distinct_rows_are_distinct():
    """0 is the selection kernels' "nothing left" and ~0 their first "select below this": a value whose key were either
    could never be selected (the raw-bit key of the NaN 0x7fffffff at row 0 was ~0)"""
    rng = np.random.default_rng(0)
    bits = np.concatenate([np.array(list(P.SPECIALS.values()), np.uint32),
                           rng.integers(0, 2**32, size=4096, dtype=np.uint64).astype(np.uint32)])
    for row in ROWS:
        keys = P.topk_key(bits, np.full(len(bits), row))
        assert (keys != 0).all() and (keys != np.uint64(2**64 - 1)).all()
    assert int(_raw_key([0x7fffffff], [0])[0]) == 2**64 - 1
    assert int(P.topk_key([0x7fffffff], [0])[0]) == (0xffc00000 << 32) | 0xffffffff  # the largest real key: a NaN, row 0
    assert int(P.topk_key([0xff800000], [2**32 - 2])[0]) == (0x007fffff << 32) | 1  # the smallest real key: -inf, last row
    rows = np.arange(len(bits))
    assert len(np.unique(P.topk_key(bits, rows))) == len(bits)


def test_descending_key_order_is_topk_rows_on_a_column_of_special_values():
    rng = np.random.default_rng(1)
    bits = np.concatenate([np.array(list(P.SPECIALS.values()) * 3, np.uint32), P.bits_of(rng.normal(size=50))])
    bits = bits[rng.permutation(len(bits))]
    order = np.argsort(P.topk_key(bits, np.arange(len(bits))))[::-1]
    with np.errstate(invalid="ignore"):  # the float64 cast of a signalling NaN
        want = H.topk_rows(P.f32(bits), len(bits))
    assert np.array_equal(order, want)


def test_the_contract_check_tells_the_raw_bit_key_apart():
    """the three orders the raw-bit key got wrong: the check above is able to see them"""
    S = P.SPECIALS
    for (a, ra), (b, rb) in (((S["-0"], 0), (S["+0"], 1)), ((S["-nan"], 0), (S["+inf"], 1)), ((S["nan"], 0), (S["nan_payload"], 1))):
        assert P.contract_before(a, ra, b, rb)
        assert P.topk_key([a], [ra])[0] > P.topk_key([b], [rb])[0]
        assert not _raw_key([a], [ra])[0] > _raw_key([b], [rb])[0]
