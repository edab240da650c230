"""The radix select's C entries (include/hmc.h: hmc_select_*, hmc_order_stats) driven raw through
ctypes: every HMC_EINVAL condition is refused on the host before any launch, so fake device pointers
never reach a GPU and none is needed here.  The launches themselves: tests/test_gpu_quantiles.py."""
import ctypes

import pytest

PTR = 0x7000_0000                                        # fake device pointers (never dereferenced)


@pytest.fixture
def L(monkeypatch):
    from hmc_amd import _lib as H
    monkeypatch.setattr(H, "_lib", None)                 # argtypes bound to this module's classes
    return H, H.lib()


def view(H, D, q=PTR, n_chains=4, rows=(1, 6, 1), row_stride=None, chain_stride=None):
    rs = D if row_stride is None else row_stride
    return H.Samples(q, n_chains, 6 * rs if chain_stride is None else chain_stride, rs, *rows)


def ranks(*r):
    return (ctypes.c_int64 * len(r))(*r)


def einval(H, status, match=None):
    assert status == H.HMC_EINVAL
    with pytest.raises(AssertionError, match=match):
        H.check(status, "x")


def test_constants_match_header(L):
    import os
    import re
    from conftest import ROOT
    H, _ = L
    src = open(os.path.join(ROOT, "include", "hmc.h")).read()
    for name, mine in (("BITS", H.SELECT_BITS), ("MAX_RANKS", H.SELECT_MAX_RANKS),
                       ("STATE_STRIDE", H.SELECT_STATE_STRIDE)):
        assert int(re.search(r"HMC_SELECT_%s\s*=\s*(\d+)" % name, src).group(1)) == mine
    assert H.SELECT_BINS == 1 << H.SELECT_BITS and H.SELECT_PASSES * H.SELECT_BITS == 64


def test_size_and_grid_queries(L):
    H, lib = L
    for D, T in ((1, 1), (100, 8), (1000, 3)):
        assert lib.hmc_select_workspace_size(D, T) == D * T * (H.SELECT_STATE_STRIDE + H.SELECT_BINS) * 8
    for D, T in ((0, 1), (5, 0), (5, 9)):
        assert lib.hmc_select_workspace_size(D, T) == 0
    assert lib.hmc_select_grid(100, 0) == 0 and lib.hmc_select_grid(0, 100) == 0
    assert lib.hmc_select_grid(100, 1) == 1
    # a function of (D, n_samples) alone, covering every sample: blocks x per >= M > (blocks - 1) x per
    for D, M in ((1, 5000), (100, 6_488_064), (1000, 104_857_600), (16, 1 << 40)):
        blocks = lib.hmc_select_grid(D, M)
        assert blocks >= 1 and blocks == lib.hmc_select_grid(D, M)
        per = -(-M // blocks)
        assert per <= 1 << 31                            # the 32-bit LDS counters cannot wrap


def test_order_stats_refuses_bad_arguments(L):
    H, lib = L
    D, T = 5, 3
    nbytes = lib.hmc_select_workspace_size(D, T)
    ok = view(H, D)                                       # M = 4 x 5 = 20
    call = lambda s=ok, D=D, T=T, r=ranks(0, 7, 19), out=PTR, ws=PTR, nb=nbytes: \
        lib.hmc_order_stats(ctypes.byref(s) if s is not None else None, D, T, r, out, ws, nb, None)
    einval(H, call(s=None))
    einval(H, call(s=view(H, D, q=None)))
    einval(H, call(r=None))
    einval(H, call(out=None))
    einval(H, call(ws=None))
    einval(H, call(D=0))
    einval(H, call(T=0))
    einval(H, call(T=9, r=ranks(*range(9))))
    einval(H, call(r=ranks(0, 7, 20)), match="rank")      # M itself
    einval(H, call(r=ranks(-1, 7, 19)), match="rank")
    einval(H, call(s=view(H, D, row_stride=D - 1)), match="row_stride")
    einval(H, call(s=view(H, D, rows=(1, 6, 0))), match="row_step")
    einval(H, call(s=view(H, D, rows=(-1, 6, 1))))
    einval(H, call(s=view(H, D, rows=(3, 2, 1))))
    einval(H, call(s=view(H, D, n_chains=-1)))
    einval(H, call(nb=nbytes - 8), match="needs")         # an undersized workspace
    einval(H, call(nb=0), match="needs")


def test_empty_view_is_ok_and_launches_nothing(L):
    """M == 0 (no chains, or no rows): HMC_OK before anything could touch the fake pointers; the ranks
    are not looked at, as no rank is valid."""
    H, lib = L
    D, T = 5, 2
    nbytes = lib.hmc_select_workspace_size(D, T)
    for s in (view(H, D, n_chains=0), view(H, D, rows=(3, 3, 1))):
        assert lib.hmc_order_stats(ctypes.byref(s), D, T, ranks(0, 0), PTR, PTR, nbytes, None) == H.HMC_OK
        assert lib.hmc_order_stats(ctypes.byref(s), D, T, ranks(0, 0), None, None, 0, None) == H.HMC_OK
    for s in (view(H, D, q=None, n_chains=0), view(H, D, q=None, rows=(3, 3, 1))):     # no storage: q may be NULL
        assert lib.hmc_order_stats(ctypes.byref(s), D, T, ranks(0, 0), None, None, 0, None) == H.HMC_OK
    assert lib.hmc_select_init(PTR, D, T, ranks(0, 0), 0, None) == H.HMC_OK


def test_staged_entries_refuse_bad_arguments(L):
    H, lib = L
    D, T = 5, 3
    ok = view(H, D)
    # init
    einval(H, lib.hmc_select_init(None, D, T, ranks(0, 1, 2), 20, None))
    einval(H, lib.hmc_select_init(PTR, D, T, None, 20, None))
    einval(H, lib.hmc_select_init(PTR, 0, T, ranks(0, 1, 2), 20, None))
    einval(H, lib.hmc_select_init(PTR, D, 0, ranks(0, 1, 2), 20, None))
    einval(H, lib.hmc_select_init(PTR, D, 9, ranks(*range(9)), 20, None))
    einval(H, lib.hmc_select_init(PTR, D, T, ranks(0, 1, 20), 20, None), match="rank")
    einval(H, lib.hmc_select_init(PTR, D, T, ranks(0, -1, 2), 20, None), match="rank")
    einval(H, lib.hmc_select_init(PTR, D, T, ranks(0, 1, 2), -1, None))
    # count
    count = lambda s=ok, D=D, T=T, p=0, st=PTR, c=PTR: \
        lib.hmc_select_count(ctypes.byref(s) if s is not None else None, D, T, p, st, c, None)
    einval(H, count(s=None))
    einval(H, count(s=view(H, D, q=None)))
    einval(H, count(st=None))
    einval(H, count(c=None))
    einval(H, count(D=0))
    einval(H, count(T=0))
    einval(H, count(T=9))
    einval(H, count(p=-1), match="pass")
    einval(H, count(p=H.SELECT_PASSES), match="pass")
    einval(H, count(s=view(H, D, row_stride=D - 1)), match="row_stride")
    einval(H, count(s=view(H, D, rows=(1, 6, 0))), match="row_step")
    # pick
    einval(H, lib.hmc_select_pick(D, T, 0, None, PTR, None))
    einval(H, lib.hmc_select_pick(D, T, 0, PTR, None, None))
    einval(H, lib.hmc_select_pick(0, T, 0, PTR, PTR, None))
    einval(H, lib.hmc_select_pick(D, 9, 0, PTR, PTR, None))
    einval(H, lib.hmc_select_pick(D, T, -1, PTR, PTR, None), match="pass")
    einval(H, lib.hmc_select_pick(D, T, H.SELECT_PASSES, PTR, PTR, None), match="pass")
    # values
    einval(H, lib.hmc_select_values(D, T, None, PTR, None))
    einval(H, lib.hmc_select_values(D, T, PTR, None, None))
    einval(H, lib.hmc_select_values(0, T, PTR, PTR, None))
    einval(H, lib.hmc_select_values(D, 0, PTR, PTR, None))
