"""The four-chain kernel's split Philox block (csrc/hmc_philox_split.hpp: a per-pair table entry, two
loop-invariant words per lane, and a block function that starts at round 3) against
tests/philox_host.np_philox, word for word.  The header is exercised through the host-only program
split_host that make builds next to libhmc.so; no GPU.

Cases: pairs 0..55 (the table's whole range at D = 112), iterations 0, 1 and 2^32 - 1, chain ids on
both sides of a 2^32 boundary and past 2^33, two seeds whose high words are non-zero."""
import os
import subprocess

import numpy as np
import pytest

from philox_host import np_philox

PAIRS = range(56)
ITERS = (0, 1, 2 ** 32 - 1)
CHAINS = (0, 5, 2 ** 32 - 1, 2 ** 32, 2 ** 33 + 5)
SEEDS = (0x9E3779B97F4A7C15, 0x0000000100000000 | 0xF00D)


def _host(cases):
    from hmc_amd import _lib
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), "split_host")
    assert os.path.exists(exe), f"{exe} not found: build it with make -C understanding-hmc_amd/csrc"
    text = "".join(f"{seed:#x} {chain:#x} {it} {k}\n" for seed, chain, it, k in cases)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout
    rows = np.array([[int(x) for x in line.split()] for line in out.splitlines()], dtype=np.uint64)
    assert rows.shape == (len(cases), 4)
    return rows


@pytest.mark.parametrize("seed", SEEDS, ids=hex)
def test_split_block_equals_philox(seed):
    assert seed >> 32 != 0
    cases = [(seed, c, it, k) for c in CHAINS for it in ITERS for k in PAIRS]
    got = _host(cases)
    ctr = np.array([[k, it, c & 0xFFFFFFFF, c >> 32] for _, c, it, k in cases], dtype=np.uint64)
    ref = np.stack(np_philox(ctr, (seed & 0xFFFFFFFF, seed >> 32)), axis=1)
    assert np.array_equal(got, ref)


def test_blocks_depend_on_every_counter_word():
    """The cases are not degenerate: changing the pair, the iteration, either chain word or either
    seed word changes the block."""
    base = (SEEDS[0], 2 ** 33 + 5, 1, 7)
    variants = [base, (SEEDS[0], 2 ** 33 + 5, 1, 8), (SEEDS[0], 2 ** 33 + 5, 2, 7), (SEEDS[0], 2 ** 33 + 6, 1, 7),
                (SEEDS[0], 2 ** 32 + 5, 1, 7), (SEEDS[0] ^ 1, 2 ** 33 + 5, 1, 7), (SEEDS[0] ^ (1 << 32), 2 ** 33 + 5, 1, 7)]
    rows = _host(variants)
    assert len({tuple(r) for r in rows.tolist()}) == len(variants)
