"""The two device primitives nearly every kernel family stands on — the exclusive scan (device_scan.h) and the radix sort of pairs
(device_radix.h) — called directly through the library's test entry points and held byte for byte to three lines of numpy, on the corpus of
tests/primitive_cases.py: every digit split of the sort, both scan kernels on both sides of their switch, 64 / 65 / 301 tiles of look-back,
several scans on one scratch (stale status words, the epoch's restart), computed loaders with and without 16-byte loads, unaligned data."""
import numpy as np
import pytest

import primitive_cases as pc

pytestmark = pytest.mark.gpu


def _check_scan(got, arrays, what):
    assert len(got) == len(arrays)
    for k, ((out, total), x) in enumerate(zip(got, arrays)):
        want, want_total = pc.scan_reference(x)
        assert out.dtype == np.uint32 and len(out) == len(x)
        if out.tobytes() != want.tobytes():
            bad = np.flatnonzero(out != want)
            raise AssertionError("%s, scan %d: %d of %d words differ, first at %d (tile %d): got %d, want %d" % (
                what, k, len(bad), len(x), bad[0], bad[0] // 4096, out[bad[0]], want[bad[0]]))
        assert total == want_total, "%s, scan %d: total %d, want %d" % (what, k, total, want_total)


@pytest.mark.parametrize("kind", pc.SCAN_VALUES)
@pytest.mark.parametrize("count", pc.SCAN_COUNTS)
def test_scan(built_lib, count, kind):
    x = pc.scan_values(kind, count)
    _check_scan(pc.device_scan(built_lib, [x]), [x], "%s x %d" % (kind, count))


@pytest.mark.parametrize("name", sorted(pc.SCAN_SEQUENCES))
def test_scan_sequences_on_one_scratch(built_lib, name):
    counts, epoch = pc.SCAN_SEQUENCES[name]
    for kind in ("random", "ones"):
        arrays = [pc.scan_values(kind, c, seed=k) for k, c in enumerate(counts)]
        _check_scan(pc.device_scan(built_lib, arrays, initial_epoch=epoch), arrays, "%s, %s" % (name, kind))


@pytest.mark.parametrize("count", pc.SCAN_LOADER_COUNTS)
@pytest.mark.parametrize("loader", sorted(pc.SCAN_LOADERS))
def test_scan_loaders(built_lib, loader, count):
    for kind in ("random", "all_ff"):
        x = pc.scan_values(kind, count)
        _check_scan(pc.device_scan(built_lib, [x], loader=pc.SCAN_LOADERS[loader]), [x], "%s, %s x %d" % (loader, kind, count))


@pytest.mark.parametrize("count", pc.SCAN_MISALIGN_COUNTS)
@pytest.mark.parametrize("misalign", pc.SCAN_MISALIGN)
def test_scan_of_unaligned_data(built_lib, misalign, count):
    for kind in ("random", "ones"):
        x = pc.scan_values(kind, count)
        _check_scan(pc.device_scan(built_lib, [x], misalign=misalign), [x], "misaligned by %d words, %s x %d" % (misalign, kind, count))


@pytest.mark.parametrize("n,bits", pc.sort_cases())
def test_sort(built_lib, n, bits):
    passes = pc.plan(built_lib, bits, 0)[1]
    vals = np.arange(n, dtype=np.uint32)                     # the indices: a tie out of order shows in them
    for kind in pc.SORT_KEYS:
        keys = pc.sort_keys(kind, n, bits)
        want_k, want_v = pc.sort_reference(keys, vals)
        got_k, got_v, which = pc.device_sort(built_lib, keys, vals, bits)
        what = "%s keys, n = %d, bits = %d" % (kind, n, bits)
        if got_k.tobytes() != want_k.tobytes() or got_v.tobytes() != want_v.tobytes():
            bad = np.flatnonzero((got_k != want_k) | (got_v != want_v))
            raise AssertionError("%s: %d of %d pairs differ, first at %d: got (%d, %d), want (%d, %d)" % (
                what, len(bad), n, bad[0], got_k[bad[0]], got_v[bad[0]], want_k[bad[0]], want_v[bad[0]]))
        assert which == (passes & 1), "%s: the result is in buffer %d after %d passes" % (what, which, passes)
