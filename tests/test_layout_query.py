"""Host-side layout query (no GPU): hmc_random_layout answers which (K coordinate pairs per lane,
lpc lanes per chain, cpw chains per wave) hmc_random_iters would launch
(hmc_route.cpp::choose_layout and wave_layout themselves, not a restatement).

The table below is every layout the lane-group kernel (D <= 64) can take; the GPU cases of
tests/test_gpu_lane_groups.py must reach each of them, so a change to the scoring that adds a layout
or drops one from those cases fails here, without a GPU."""
import ctypes

import pytest

# K -> lanes per chain; cpw = 64 // lpc
LANES = {
    1: [1, 2, 3, 4, 7, 8, 9, 10, 11, 12, 15, 16, 19, 20, 21, 25, 26, 27, 28, 29, 30, 31, 32],
    2: [3, 7, 9, 11, 12],
    4: [3, 7],
    5: [1, 2, 3, 4, 5],
    8: [3],
}
TABLE = {(K, lpc, 64 // lpc) for K, lanes in LANES.items() for lpc in lanes}


@pytest.fixture(autouse=True)
def _fresh_library(monkeypatch):
    from hmc_amd import _lib as H
    monkeypatch.setattr(H, "_lib", None)     # argtypes bound to this module's structure classes


def _layout():
    from hmc_amd import _lib as H
    return H.random_layout


def test_table_has_36_layouts():
    assert len(TABLE) == 36 and not any(K == 16 for K, _, _ in TABLE)


def test_lane_group_layouts_are_exactly_the_table():
    """D = 1..64 over 1 <= L_low <= 40, L_low < L_high <= L_low + 40: the layouts returned are the
    table's, all of them; each covers the chain's pairs and fits a wave."""
    layout = _layout()
    seen = set()
    for D in range(1, 65):
        npairs = (D + 1) // 2
        for lo in range(1, 41):
            for hi in range(lo + 1, lo + 41):
                K, lpc, cpw, wave = layout(D, lo, hi)
                assert wave == 0, (D, lo, hi)
                assert K * lpc >= npairs, (D, lo, hi, K, lpc)
                assert 1 <= lpc * cpw <= 64 and cpw == 64 // lpc, (D, lo, hi, lpc, cpw)
                seen.add((K, lpc, cpw))
    assert seen == TABLE, (sorted(seen - TABLE), sorted(TABLE - seen))


def test_first_wave_per_chain_shape():
    layout = _layout()
    assert layout(64, 5, 20) == (1, 32, 2, 0)
    assert layout(65, 5, 20) == (1, 64, 1, 1)
    assert layout(129, 5, 20) == (2, 64, 1, 1) and layout(2048, 5, 20) == (16, 64, 1, 1)


def test_refusals():
    """HMC_EINVAL (AssertionError) for null arguments, D < 1 and an empty trajectory-length range;
    HMC_ENOTSUP (NotImplementedError) for dense targets and the large-D path."""
    from hmc_amd import _lib as H
    L = H.lib()
    out = (ctypes.c_int32 * 4)()
    T = H.Target(10, H.HMC_TARGET_DIAG, None, None, 0.0)
    S = H.Schedule(0, 0, 1, 0, 1, 2, 5, 20, 1, 1, H.HMC_RNG_PHILOX, H.HMC_MODE_FAST, 10, 0, 0)
    assert L.hmc_random_layout(ctypes.byref(T), ctypes.byref(S), ctypes.byref(out)) == H.HMC_OK
    assert tuple(out) == (5, 1, 64, 0)
    for args in ((None, ctypes.byref(S), ctypes.byref(out)), (ctypes.byref(T), None, ctypes.byref(out)),
                 (ctypes.byref(T), ctypes.byref(S), None)):
        assert L.hmc_random_layout(*args) == H.HMC_EINVAL
    with pytest.raises(AssertionError):
        H.random_layout(0, 5, 20)
    with pytest.raises(AssertionError):
        H.random_layout(10, 5, 5)
    with pytest.raises(NotImplementedError):
        H.random_layout(2050, 5, 20)                     # diagonal D > 2048: the large-D path
    T.kind = H.HMC_TARGET_DENSE
    assert L.hmc_random_layout(ctypes.byref(T), ctypes.byref(S), ctypes.byref(out)) == H.HMC_ENOTSUP


def test_gpu_cases_reach_every_layout():
    """The (D, L_low, L_high) cases of tests/test_gpu_lane_groups.py hit every layout of the table,
    the Philox cases one each and under the layout they are listed for."""
    import test_gpu_lane_groups as G
    layout = _layout()
    assert {layout(*c)[:3] for c in G.all_cases()} == TABLE
    assert set(G.PHILOX_CASES) == TABLE
    for lay, case in G.PHILOX_CASES.items():
        assert layout(*case) == lay + (0,), case
    assert {layout(*c)[:3] for c in G.REPLAY_CASES} == TABLE           # the replay cases alone do too
    assert {layout(*c[:3])[0] for c in G.GEN_CASES} == {1, 2, 4, 5, 8}
    assert all(layout(*c[:3])[1] > 1 and c[0] % 2 == 1 for c in G.GEN_CASES)
    for D, lo, hi in sorted(G.PHILOX_CASES.values()):
        K, lpc, cpw, _ = layout(D, lo, hi)
        odd = [d for d in range(1, 65, 2) if layout(d, lo, hi)[:3] == (K, lpc, cpw)]
        assert D % 2 == 1 or not odd, (D, odd)


def test_routes_are_the_recorded_ones():
    """tests/golden/random_routes.json (scripts/dev/gen_random_routes.py, written from the library
    of the commit before the kernel choice moved into csrc/hmc_route.cpp): layout, leapfrog form and
    workspace sizes over a grid that crosses every edge of the choice, entry for entry."""
    import importlib.util
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gen_random_routes",
                                                  os.path.join(root, "scripts", "dev", "gen_random_routes.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(root, "tests", "golden", "random_routes.json")) as f:
        want = json.load(f)["entries"]
    assert len(want) == 862                   # a regenerated file cannot shrink unnoticed
    got = gen.table()
    assert [c for c, _ in got] == [c for c, _ in want]
    bad = [(c, a, b) for (c, a), (_, b) in zip(got, want) if a != b]
    assert not bad, (len(bad), bad[:5])
    statuses = {a[0] for _, a in want}
    layouts = {tuple(a[1:5]) for _, a in want if a[0] == 0}
    # both sides of the three-term rule's length bound where m = 2 decides it (dt = 1.999: 199 | 200)
    assert {c[3]: a[5] for c, a in want if c[0] == 129 and c[7] == 1.999} == {199: 1, 200: 0, 399: 0, 400: 0}
    assert statuses == {0, 5} and (4, 16, 4, 0) in layouts and {a[5] for _, a in want} == {0, 1}
