"""The radix select's host-visible rules (csrc/hmc_select.hpp: the key map, its inverse, the pick
rule) as the kernels compile them, through the host-only program lib/select_host; no GPU."""
import os
import struct
import subprocess

import numpy as np

from conftest import PKG_DIR

SELECT_HOST = os.path.join(PKG_DIR, "lib", "select_host")
NAN_KEY = 0xFFFFFFFFFFFFFFFF


def run(mode, text):
    assert os.path.exists(SELECT_HOST), "lib/select_host is missing: build() makes it (make in csrc/)"
    r = subprocess.run([SELECT_HOST, mode], input=text, capture_output=True, text=True, check=True)
    return [line.split() for line in r.stdout.splitlines()]


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def keys_of(bit_patterns):
    out = run("key", "\n".join("%016x" % b for b in bit_patterns))
    assert len(out) == len(bit_patterns)
    return [int(k, 16) for k, _ in out], [int(b, 16) for _, b in out]


DENORM_MIN, DBL_MIN, DBL_MAX = 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308
FINITE = [0.0, DENORM_MIN, DBL_MIN, 1.0, 1.0 + 2.0 ** -52, DBL_MAX, float("inf")]
SPECIALS = [bits_of(s * v) for v in FINITE for s in (1.0, -1.0)]
NANS = [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001,   # quiet / signalling,
        0x7FF8000000000123, 0xFFFFFFFFFFFFFFFF]                                           # both signs, payloads


def test_key_order_matches_np_sort():
    """Sorting the specials by key gives np.sort's order (+-0 compare equal), the inverse map gives the
    bits back, and every NaN maps to one key, the largest."""
    pats = SPECIALS + NANS
    keys, back = keys_of(pats)
    vals = np.array(pats, dtype=np.uint64).view(np.float64)
    by_key = vals[np.argsort(np.array(keys, dtype=np.uint64), kind="stable")]
    ref = np.sort(vals)
    n = len(SPECIALS)
    assert np.array_equal(by_key[:n], ref[:n])                      # == : -0.0 and +0.0 are equal
    assert np.isnan(by_key[n:]).all() and np.isnan(ref[n:]).all()
    for p, k, b in zip(SPECIALS, keys, back):
        assert b == p, ("%016x" % p, "%016x" % b)
        assert k < NAN_KEY
    assert len(set(keys[:n])) == n                                  # distinct values, distinct keys (-0 < +0)
    for k, b in zip(keys[n:], back[n:]):
        assert k == NAN_KEY
        assert np.isnan(np.array([b], dtype=np.uint64).view(np.float64)[0])


def test_key_is_monotone_on_random_doubles():
    rs = np.random.RandomState(0)
    pats = rs.randint(0, 2 ** 63, size=4000, dtype=np.int64).astype(np.uint64) | \
        (rs.randint(0, 2, size=4000).astype(np.uint64) << np.uint64(63))
    vals = pats.view(np.float64)
    keep = ~np.isnan(vals)
    pats, vals = pats[keep], vals[keep]
    keys, back = keys_of([int(p) for p in pats])
    assert back == [int(p) for p in pats]
    order = np.argsort(np.array(keys, dtype=np.uint64), kind="stable")
    assert np.array_equal(vals[order], np.sort(vals))


def reference_pick(c, r):
    cum = np.cumsum(c)
    digit = int(np.searchsorted(cum, r, side="right"))
    return digit, int(r - (cum[digit - 1] if digit > 0 else 0))


def test_pick_matches_searchsorted():
    """The chosen digit and the new remaining rank on random histograms, with ranks on both edges of
    every non-empty bin and empty bins before, between and after."""
    rs = np.random.RandomState(1)
    cases = []
    for nbins in (2, 16, 256):
        for trial in range(6):
            c = rs.randint(0, 50, size=nbins).astype(np.int64)
            c[rs.random_sample(nbins) < 0.5] = 0                    # empty bins anywhere
            if trial % 2:
                c[:nbins // 4] = 0                                  # ... a run of them first
                c[-(nbins // 4):] = 0                               # ... and last
            if c.sum() == 0:
                c[nbins // 2] = 3
            if trial == 5:
                c = c * (2 ** 40)                                   # totals past 32 bits
            cum = np.cumsum(c)
            edges = set()
            for d in np.nonzero(c)[0]:
                edges.update((int(cum[d] - c[d]), int(cum[d] - 1)))  # first and last rank of bin d
            ranks = sorted(edges | {int(v) for v in rs.randint(0, cum[-1], size=8)})
            cases += [(c, r) for r in ranks]
    text = "\n".join("%d %d %s" % (len(c), r, " ".join(str(int(v)) for v in c)) for c, r in cases)
    out = run("pick", text)
    assert len(out) == len(cases)
    for (c, r), (digit, rem) in zip(cases, out):
        assert (int(digit), int(rem)) == reference_pick(c, r), (c.tolist(), r)
        assert c[int(digit)] > 0 and 0 <= int(rem) < c[int(digit)]


def test_bad_input_is_refused():
    assert os.path.exists(SELECT_HOST)
    r = subprocess.run([SELECT_HOST, "key"], input="xyz", capture_output=True, text=True)
    assert r.returncode == 2
    r = subprocess.run([SELECT_HOST], input="", capture_output=True, text=True)
    assert r.returncode == 2
