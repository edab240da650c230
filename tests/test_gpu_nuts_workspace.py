"""A NUTS launch stays inside exactly the workspace its size query asks for.

Each of the four NUTS kernels carves its regions (slot vectors, replay-tape cursors, queue words,
pre-drawn momenta) out of one caller-provided buffer; only the slot vectors go through a bounded
buffer descriptor (csrc/hmc_nuts_layout.hpp).  Every case runs an engine on a workspace of exactly
the queried size that sits between two guard bands inside one larger allocation, so a write past
either end lands in a guard, where it is seen and cannot fault: both guards must come back bit for
bit, and the run must equal an identically seeded engine's on its own allocation.  Chain counts
are no multiple of the 16-chain tiles, and the Philox tree cases fill the momenta region (the last
one of that layout) completely.
"""
import numpy as np
import pytest
import torch

import glm_cases as G
import make_golden_shapes as S
from oracle import hmc_oracle as O

pytestmark = pytest.mark.gpu

GUARD = 512                      # doubles on either side: keeps the workspace 16-byte aligned
SENTINEL = -6.02214076e23


def _tree_engine(D, N, d_max, calls, rng="philox", cov_p=None, rho=0.5):
    """NutsEngine on a correlated MVN, sized for the longest of `calls` (so that with Philox momenta
    and a diagonal cov_p the momenta region is exactly full), started and ready to run."""
    from hmc_amd.engine import NutsEngine
    from hmc_amd.target import MVNTarget
    n_iter = calls[-1][1] - 1
    rs = np.random.RandomState(100 + D)
    eng = NutsEngine(MVNTarget(np.zeros(D), O.mvn_cov(D, rho)), N, n_iter, 0, 1, d_max, 0.15, cov_p=cov_p, rng=rng,
                     seed=9, fp_mode="fast", on_dmax="break", iters_per_call=max(b - a for a, b in calls))
    q_start = rs.standard_normal((N, D))
    if rng == "replay":                                      # the tape recipe of tests/test_gpu_nuts.py
        p0 = rs.standard_normal((N, D))
        P = rs.standard_normal((N, n_iter, D))
        eng.set_replay(p0, P, rs.uniform(0.0, 2.0, (N, n_iter * 2 * (2 ** d_max + d_max + 2))))
    eng.init(q_start)
    return eng


def _glm_engine(calls):
    from hmc_amd.engine import GLMNutsEngine
    c = G.recipe("poisson", 3, 32, 20, 0.5, 31)
    eng = GLMNutsEngine(G.glm_target(c), c["N"], calls[-1][1] - 1, 0, 1, 5, c["dt"], rng="philox", seed=9,
                        on_dmax="break")
    eng.init(c["q_start"])
    return eng


def _diag(D):
    return np.diag(np.linspace(0.7, 1.6, D))


CASES = {
    # tree kernel (hmc_nuts.hip): Philox momenta drawn ahead, 3 + 3 iterations at iters_per_call = 3
    "tree_philox_D5": (lambda calls: _tree_engine(5, 20, 6, calls), [(1, 4), (4, 7)]),
    # its short-last-tile instance (D = 97..100)
    "tree_short_tile_D100": (lambda calls: _tree_engine(100, 3, 8, calls, rho=0.9), [(1, 3), (3, 5)]),
    # replay: the tape cursors persist from the first launch to the second
    "tree_replay_D16": (lambda calls: _tree_engine(16, 17, 6, calls, rng="replay"), [(1, 3), (3, 5)]),
    # full cov_p: in-kernel draws, no momenta region
    "tree_full_cov_p_D8": (lambda calls: _tree_engine(8, 5, 6, calls, cov_p=S.dense_cov_p(8)), [(1, 3), (3, 5)]),
    # lockstep kernel (hmc_nuts_lock.hip), 128 < D <= 320: one and three fragment sets
    "lock_diag_cov_p_D144": (lambda calls: _tree_engine(144, 40, 5, calls, cov_p=_diag(144)), [(1, 2), (2, 4)]),
    "lock_full_cov_p_D130": (lambda calls: _tree_engine(130, 17, 4, calls, cov_p=S.dense_cov_p(130)),
                             [(1, 2), (2, 3)]),
    # one wave per chain (hmc_nuts_big.hip), D > 320
    "per_chain_D330": (lambda calls: _tree_engine(330, 2, 4, calls), [(1, 2), (2, 3)]),
    # GLM NUTS (hmc_glm_nuts.hip)
    "glm_poisson_D3": (_glm_engine, [(1, 3), (3, 5)]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_launch_stays_inside_queried_workspace(name):
    from hmc_amd import _lib as H
    make, calls = CASES[name]
    ref, eng = make(calls), make(calls)
    n = eng.ws.numel()                                       # the size query's bytes / 8, exactly
    assert n > 0 and n == ref.ws.numel()
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float64, device=eng.device)
    eng.ws = buf[GUARD:GUARD + n]
    eng.ws.zero_()
    assert eng.ws.data_ptr() % 16 == 0
    for e in (ref, eng):
        for it0, it1 in calls:
            e.run(it0, it1)
    torch.cuda.synchronize()
    sentinel = torch.full((GUARD,), SENTINEL, dtype=torch.float64, device=eng.device).view(torch.int64)
    assert torch.equal(buf[:GUARD].view(torch.int64), sentinel), "write before the workspace"
    assert torch.equal(buf[GUARD + n:].view(torch.int64), sentinel), "write past the queried workspace size"
    for k in ("q", "q_chain", "E_chain"):
        a, b = getattr(eng, k), getattr(ref, k)
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)), k
    assert np.isfinite(eng.q_chain.cpu().numpy()).all()
    # every counter but the steps of the schedule (which slot ran which tree: not a result)
    res = [i for i in range(H.NCOUNTERS) if i != H.CNT_LEAPFROG_SQ]
    assert np.array_equal(eng.read_counters()[res], ref.read_counters()[res])
    assert eng.read_counters()[H.CNT_LEAPFROG] > 0 and eng.read_counters()[H.CNT_HANDOFF_GIVEUP] == 0
