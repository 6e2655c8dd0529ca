"""The corpus of tests/primitive_cases.py reaches what it claims to reach (no GPU needed): the library's own plan
(phx_debug_primitive_plan reads the dispatchers' constants) puts its sizes on every digit split of the radix sort and on both sides of
every path switch of the scan; and the numpy references agree with plain Python loops."""
import numpy as np
import pytest

import primitive_cases as pc

# bits -> (digit width, passes): the table of device_radix_sort_pairs
SPLITS = {0: (8, 1), 1: (8, 1), 7: (8, 1), 8: (8, 1), 9: (11, 1), 11: (11, 1), 12: (8, 2), 16: (8, 2), 17: (11, 2), 22: (11, 2),
          23: (8, 3), 24: (8, 3), 25: (11, 3), 31: (11, 3), 32: (11, 3)}


def test_bits_reach_every_digit_split(built_lib):
    got = {b: pc.plan(built_lib, b, 0)[:2] for b in pc.SORT_BITS}
    assert got == SPLITS
    assert set(got.values()) == {(8, 1), (11, 1), (8, 2), (11, 2), (8, 3), (11, 3)}
    # the large sizes keep all six, and both parities of the pass count (the result ends in either buffer)
    assert {got[b] for b in pc.SORT_BITS_LARGE} == set(got.values())
    # every split is entered at its first width and left at its last: the whole table, bit by bit
    for lo, hi, split in ((0, 8, (8, 1)), (9, 11, (11, 1)), (12, 16, (8, 2)), (17, 22, (11, 2)), (23, 24, (8, 3)), (25, 32, (11, 3))):
        for bits in range(lo, hi + 1):
            assert pc.plan(built_lib, bits, 0)[:2] == split, bits
        assert lo in pc.SORT_BITS and hi in pc.SORT_BITS


def test_scan_counts_straddle_the_path_switch(built_lib):
    plans = {c: pc.plan(built_lib, 0, c)[2:] for c in pc.SCAN_COUNTS}
    assert plans[0] == (0, 0)                                 # (an empty scan launches nothing)
    for c in (1, 3, 4, 5, 4095, 4096, 4097, 32767, 32768):
        assert plans[c][0] == 1, c
    assert plans[32768] == (1, 8) and plans[32769] == (0, 9)  # the switch; then nine tiles, the last holding one word
    for c in (36863, 262143, 262144, 262145, 266241, 1228801):
        assert plans[c][0] == 0, c
    assert [plans[c][1] for c in (4095, 4096, 4097)] == [1, 1, 2]
    assert plans[36863][1] == 9
    assert plans[262143][1] == 64 and plans[262144][1] == 64 and plans[262145][1] == 65      # a full look-back window, then one more
    assert plans[266241][1] == 66
    assert plans[1228801][1] == 301                           # five windows
    assert {9, 64, 65, 301} <= {t for _, t in plans.values()}
    for counts, _ in pc.SCAN_SEQUENCES.values():
        assert all(c in plans and plans[c][0] == 0 for c in counts)
    for c in pc.SCAN_LOADER_COUNTS + pc.SCAN_MISALIGN_COUNTS:
        assert c in plans
    assert {plans[c][0] for c in pc.SCAN_LOADER_COUNTS} == {0, 1} and {plans[c][0] for c in pc.SCAN_MISALIGN_COUNTS} == {0, 1}


def test_sort_sizes_put_the_inner_scan_on_both_paths(built_lib):
    """The sort scans its histogram, bins x workgroups words (2048 pairs per workgroup), with the scan above."""
    def hist(n, bits):
        return (1 << pc.plan(built_lib, bits, 0)[0]) * max(1, -(-n // 2048))
    assert hist(34817, 11) == 36864 and pc.plan(built_lib, 0, hist(34817, 11))[2:] == (0, 9)
    assert pc.plan(built_lib, 0, hist(34817, 8))[2] == 1
    assert pc.plan(built_lib, 0, hist(270337, 8))[2] == 0
    assert pc.plan(built_lib, 0, hist(270337, 11))[3] > 64
    assert all(pc.plan(built_lib, 0, hist(4097, b))[2] == 1 for b in pc.SORT_BITS)
    cases = pc.sort_cases()
    assert len(cases) == (len(pc.SORT_N) - 2) * len(pc.SORT_BITS) + 2 * len(pc.SORT_BITS_LARGE)
    assert {n for n, _ in cases} == set(pc.SORT_N)


def test_plan_rejects_what_the_dispatchers_never_see(built_lib):
    import ctypes as C
    v = C.c_int32(0)
    for bits, count in ((-1, 0), (33, 0), (8, -1)):
        assert built_lib.phx_debug_primitive_plan(bits, count, C.byref(v), C.byref(v), C.byref(v), C.byref(v)) == -1


@pytest.mark.parametrize("kind", pc.SCAN_VALUES)
def test_scan_reference_agrees_with_a_loop(kind):
    for count in (0, 1, 3, 4, 5, 4097):
        x = pc.scan_values(kind, count)
        assert x.dtype == np.uint32 and len(x) == count
        out, total = pc.scan_reference(x)
        lo, lt = pc.scan_reference_loop(x)
        assert out.dtype == np.uint32 and out.tobytes() == lo.tobytes() and total == lt, (kind, count)
    # the random and the all-ones-bits values wrap the prefix
    if kind in ("random", "all_ff"):
        out, _ = pc.scan_reference(pc.scan_values(kind, 4097))
        assert (np.diff(out.astype(np.int64)) < 0).any()


@pytest.mark.parametrize("kind", pc.SORT_KEYS)
def test_sort_reference_agrees_with_a_loop(kind):
    for n in (0, 1, 2, 63, 64, 65, 257):
        for bits in (0, 1, 7, 9, 12, 32):
            keys = pc.sort_keys(kind, n, bits)
            vals = np.arange(n, dtype=np.uint32)
            assert keys.dtype == np.uint32 and len(keys) == n and (n == 0 or int(keys.max()) < (1 << bits))
            k, v = pc.sort_reference(keys, vals)
            lk, lv = pc.sort_reference_loop(keys, vals)
            assert k.tobytes() == lk.tobytes() and v.tobytes() == lv.tobytes(), (kind, n, bits)


def test_key_kinds_are_what_they_say():
    n, bits = 513, 12
    assert len(set(pc.sort_keys("two_values", n, bits).tolist())) == 2
    assert len(set(pc.sort_keys("all_equal", n, bits).tolist())) == 1
    assert set(pc.sort_keys("all_max", n, bits).tolist()) == {(1 << bits) - 1}
    assert set(pc.sort_keys("all_max", n, 32).tolist()) == {0xFFFFFFFF}
    d, a = pc.sort_keys("descending", n, bits).astype(np.int64), pc.sort_keys("ascending", n, bits).astype(np.int64)
    assert (np.diff(d) <= 0).all() and d[0] > d[-1] and (np.diff(a) >= 0).all() and a[0] < a[-1]
    assert len(set(pc.sort_keys("random", n, bits).tolist())) > 256
    # ties wherever there are more keys than values: stability is visible in the values
    assert len(set(pc.sort_keys("descending", 513, 8).tolist())) == 256
