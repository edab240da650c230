"""The Box-Muller radius t = -2 log(u1) as the kernels compile it (csrc/hmc_bm_radius.hpp: table
entries, ln 2 and series coefficients scaled by -2) against the form it replaced (the unscaled series
over the unscaled table, the result times -2), through the host-only program bm_host that make builds
next to libhmc.so; no GPU.

For u1 = j 2^-52 the program prints frexp's mantissa and exponent and the two results.  Asserted for
every case: the two results are the same bits.  One exception is stated, not a tolerance: where a
result is an exact zero the new form gives +0 (x - x) and the old one -0 (-2 times +0);
hmc_device.hpp's bm_sqrt takes max(t, 2^-1000) of either.  The identity holds for any table contents,
so the program's tables come from libm.  (The integer exponent/mantissa split the header was also
meant to carry was not built: the three instructions it replaces cost what a v_fma_f64 costs,
profiles/rr_instr_prices.txt.)

Cases: j = 1, 2, 3, 2^52 - 1, 2^52; every power of two with its two neighbours; both edges of the
first, the last and two middle table buckets in three binades; 10^6 seeded random j."""
import os
import subprocess

import numpy as np
import pytest

LOG_N = 1024                      # buckets of [0.5, 1): the top 10 mantissa bits
TOP = 1 << 52


def _host(js):
    from hmc_amd import _lib
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), "bm_host")
    assert os.path.exists(exe), f"{exe} not found: build it with make -C understanding-hmc_amd/csrc"
    js = np.asarray(js, dtype=np.uint64)
    assert js.min() >= 1 and js.max() <= TOP
    text = "\n".join(str(int(j)) for j in js) + "\n"
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout
    rows = np.array([[int(x, 16) for x in line.split()] for line in out.splitlines()], dtype=np.uint64)
    assert rows.shape == (len(js), 4)
    return rows


def _check(js):
    rows = _host(js)
    fm, fk, new, old = rows.T
    mant, expo = np.frexp(np.asarray(js, dtype=np.float64) * 2.0 ** -52)
    assert np.array_equal(fm.view(np.float64), mant) and np.array_equal(fk.view(np.float64), expo.astype(np.float64))
    zero = (new << np.uint64(1)) == 0
    assert np.array_equal(zero, (old << np.uint64(1)) == 0)
    assert np.array_equal(new[~zero], old[~zero]), "-2 log(u1) differs from the frexp form times -2"
    assert np.all(new[zero] == 0), "an exact zero of the new form is +0"
    # the cases are what they claim: the mantissa is in [0.5, 1) and the result a finite number >= 0
    t = new.view(np.float64)
    assert np.all((fm >> np.uint64(52)) == 0x3FE) and np.all(np.isfinite(t)) and np.all(t >= 0)
    return rows


def _bucket_edges(binade):
    """Both edges of the first, the last and two middle buckets of the binade [2^(b-1), 2^b) of j:
    the first and the last j of each bucket (bucket = top 10 mantissa bits)."""
    lo = 1 << (binade - 1)
    width = lo // LOG_N
    assert width >= 2
    out = []
    for b in (0, LOG_N // 2 - 1, LOG_N // 2, LOG_N - 1):
        out += [lo + b * width, lo + (b + 1) * width - 1]
    return out


def test_ends_of_the_range():
    rows = _check([1, 2, 3, TOP - 1, TOP])
    t = rows[:, 2].view(np.float64)
    np.testing.assert_allclose(t[:4], -2.0 * np.log(np.array([1, 2, 3, TOP - 1], dtype=np.float64) * 2.0 ** -52), rtol=1e-15)
    assert abs(t[4]) < 1e-15                       # u1 = 1: zero up to the table's rounding


def test_powers_of_two_and_neighbours():
    js = sorted({j for k in range(53) for j in (2 ** k - 1, 2 ** k, 2 ** k + 1) if 1 <= j <= TOP})
    assert len(js) == 3 * 53 - 5                   # 0 and 2^52 + 1 are out; 1, 2, 3 are counted once
    _check(js)


@pytest.mark.parametrize("binade", [52, 30, 12])
def test_bucket_edges(binade):
    """Top, middle and a low binade (12: buckets of two values each)."""
    js = _bucket_edges(binade)
    rows = _check(js)
    # each pair is one bucket and neighbouring pairs are different buckets: the top 10 mantissa bits
    bucket = (rows[:, 0] >> np.uint64(42)) & np.uint64(LOG_N - 1)
    assert np.array_equal(bucket, np.repeat([0, LOG_N // 2 - 1, LOG_N // 2, LOG_N - 1], 2).astype(np.uint64))


def test_random_million():
    rng = np.random.default_rng(0xB0C5)
    js = rng.integers(1, TOP, size=1_000_000, endpoint=True, dtype=np.uint64)
    # half of them spread over the binades (a uniform j is in the top binade half of the time)
    shift = rng.integers(0, 52, size=js.size // 2).astype(np.uint64)
    js[:js.size // 2] = np.maximum(js[:js.size // 2] >> shift, np.uint64(1))
    rows = _check(js)
    assert len(np.unique(rows[:, 1])) >= 40        # exponents from many binades
