"""The named corpus of the two device primitives (phyx_amd/csrc/device_scan.h, device_radix.h), their numpy references, and thin wrappers
of the library's test entry points (include/phyx_amd.h: phx_debug_scan, phx_debug_radix_sort, phx_debug_primitive_plan).

The sizes are the primitives' own path switches:
  scan   one workgroup up to 32 768 words (8 tiles of 4096), the look-back kernel beyond; its look-back inspects 64 predecessors per window,
         so the 65th tile (more than 262 144 words) is the first that may need a second window
  sort   2048 pairs per workgroup, 4 waves of 8 x 64 each; its histogram (256 or 2048 bins per workgroup) is scanned by the scan above, so
         18 workgroups put the wide histogram on the look-back path (36 864 words) and 133 put the narrow one there too (34 048 words; the
         wide one is then 272 384 words, 67 tiles)
test_primitives_cpu.py proves, through the library's own plan, that these sizes reach what they claim."""
import ctypes as C

import numpy as np

U32 = np.uint32

# ---- scan --------------------------------------------------------------------------------------------------------------------------
SCAN_COUNTS = (0, 1, 3, 4, 5, 4095, 4096, 4097, 32767, 32768, 32769, 36863, 262143, 262144, 262145, 266241, 1228801)
SCAN_VALUES = ("random", "zeros", "ones", "last_one", "all_ff")
# (counts, initial_epoch): several scans on one scratch
SCAN_SEQUENCES = {
    "grow_then_stale": ((1228801, 32769, 1228801, 266241), 0),       # stale status words of older epochs inside and beyond the live tiles
    "epoch_reset": ((32769, 32769, 32769), (1 << 30) - 3),           # the scratch starts over between the first and the second scan
}
SCAN_LOADERS = {"in_place": 0, "computed": 1, "computed_load4": 2}
SCAN_LOADER_COUNTS = (4097, 32768, 32769, 262145)
SCAN_MISALIGN = (1, 2, 3)
SCAN_MISALIGN_COUNTS = (4097, 32769)


def scan_values(kind, count, seed=0):
    if kind == "random":
        return np.random.default_rng([count, seed]).integers(0, 1 << 32, size=count, dtype=np.uint64).astype(U32)
    if kind == "zeros":
        return np.zeros(count, dtype=U32)
    if kind == "ones":
        return np.ones(count, dtype=U32)
    if kind == "last_one":
        x = np.zeros(count, dtype=U32)
        x[-1:] = 1
        return x
    if kind == "all_ff":
        return np.full(count, 0xFFFFFFFF, dtype=U32)
    raise KeyError(kind)


def scan_reference(x):
    """(exclusive prefix sums, grand total), both modulo 2^32."""
    c = np.cumsum(x.astype(np.uint64), dtype=np.uint64)      # (wraps modulo 2^64, a multiple of 2^32)
    out = np.concatenate([np.zeros(1, dtype=np.uint64), c[:-1]])[:len(x)]
    return (out & 0xFFFFFFFF).astype(U32), int(c[-1]) & 0xFFFFFFFF if len(x) else 0


def scan_reference_loop(x):
    out, run = [], 0
    for v in x.tolist():
        out.append(run)
        run = (run + v) & 0xFFFFFFFF
    return np.array(out, dtype=U32), run


# ---- sort --------------------------------------------------------------------------------------------------------------------------
SORT_BITS = (0, 1, 7, 8, 9, 11, 12, 16, 17, 22, 23, 24, 25, 31, 32)
SORT_N = (0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4097, 34817, 270337)
SORT_N_LARGE = (34817, 270337)
SORT_BITS_LARGE = (8, 11, 12, 17, 24, 32)
SORT_KEYS = ("random", "two_values", "all_equal", "all_max", "descending", "ascending")


def sort_cases():
    """Every (n, bits) of the corpus; the two largest n run with SORT_BITS_LARGE only."""
    return [(n, b) for n in SORT_N for b in (SORT_BITS_LARGE if n in SORT_N_LARGE else SORT_BITS)]


def sort_keys(kind, n, bits, seed=0):
    """n keys below 2^bits."""
    top = 1 << bits
    rng = np.random.default_rng([n, bits, seed])
    if kind == "random":
        k = rng.integers(0, top, size=n, dtype=np.uint64)
    elif kind == "two_values":
        a = int(rng.integers(0, top))
        b = a ^ ((top >> 1) | 1) if bits else 0      # (differs in the highest and the lowest bit: two bins in the first pass and in the last)
        k = np.where(rng.integers(0, 2, size=n) == 1, a, b).astype(np.uint64)
    elif kind == "all_equal":
        k = np.full(n, int(rng.integers(0, top)), dtype=np.uint64)
    elif kind == "all_max":
        k = np.full(n, top - 1, dtype=np.uint64)
    elif kind == "descending":
        # n keys spread over the whole range, largest first (ties where n > 2^bits)
        k = ((np.arange(n, dtype=np.uint64)[::-1] * np.uint64(top)) // np.uint64(max(n, 1)))
    elif kind == "ascending":
        k = (np.arange(n, dtype=np.uint64) * np.uint64(top)) // np.uint64(max(n, 1))
    else:
        raise KeyError(kind)
    assert len(k) == n and (n == 0 or int(k.max()) < top)
    return k.astype(U32)


def sort_reference(keys, vals):
    o = np.argsort(keys, kind="stable")
    return keys[o], vals[o]


def sort_reference_loop(keys, vals):
    """Insertion of each pair behind every pair whose key is not larger: a stable sort by definition."""
    out = []
    for k, v in zip(keys.tolist(), vals.tolist()):
        at = len(out)
        while at > 0 and out[at - 1][0] > k:
            at -= 1
        out.insert(at, (k, v))
    return np.array([p[0] for p in out], dtype=U32), np.array([p[1] for p in out], dtype=U32)


# ---- the library's entry points ----------------------------------------------------------------------------------------------------
def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def plan(lib, bits, scan_count):
    """(digit_bits, passes, scan_single, scan_tiles) as the library's dispatchers choose them (host only)."""
    v = [C.c_int32(-1) for _ in range(4)]
    assert lib.phx_debug_primitive_plan(bits, scan_count, *[C.byref(x) for x in v]) == 0, lib.phx_last_error()
    return tuple(x.value for x in v)


def device_scan(lib, arrays, loader=0, misalign=0, initial_epoch=0):
    """The scans of `arrays`, back to back on one scratch: [(prefix sums, total)]."""
    counts = np.array([len(a) for a in arrays], dtype=np.int32)
    words = np.ascontiguousarray(np.concatenate(list(arrays) + [np.zeros(0, dtype=U32)]), dtype=U32)
    out = np.full(len(words), 0xDEADBEEF, dtype=U32)
    totals = np.full(len(arrays), 0xDEADBEEF, dtype=U32)
    st = lib.phx_debug_scan(0, _vp(words), _vp(counts), len(arrays), loader, misalign, initial_epoch, _vp(out), _vp(totals))
    assert st == 0, lib.phx_last_error()
    ends = np.cumsum(counts)
    return [(out[e - c:e], int(t)) for e, c, t in zip(ends.tolist(), counts.tolist(), totals.tolist())]


def device_sort(lib, keys, vals, bits):
    """(keys_out, vals_out, which)."""
    keys, vals = np.ascontiguousarray(keys, dtype=U32), np.ascontiguousarray(vals, dtype=U32)
    ko, vo = np.full(len(keys), 0xDEADBEEF, dtype=U32), np.full(len(keys), 0xDEADBEEF, dtype=U32)
    which = C.c_int32(-1)
    st = lib.phx_debug_radix_sort(0, _vp(keys), _vp(vals), len(keys), bits, _vp(ko), _vp(vo), C.byref(which))
    assert st == 0, lib.phx_last_error()
    return ko, vo, which.value
