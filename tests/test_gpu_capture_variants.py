"""Production instance against FULL instance of the Random iteration kernels.

A launch with chain-0 capture takes the FULL instances (csrc/hmc_route.cpp full_variant: the
lane-group kernel has one instance for both, hmc_wave.hip compiles the capture in only there); a
launch without it takes the production ones.  The capture only records: the same seeded Philox run
with and without it must leave the same bits in every output.

Shapes, the smallest that select each instance at L in [1, 4): D = 6 the lane-group kernel, D = 66
the wave kernel at K = 1 with the even ring (npairs = 33, the first past the lane-group limit),
D = 67 its ODD ring, D = 130 K = 2 (npairs = 65, the first past one pair per lane).  D = 97..112 is
left out: without capture the four-chain kernel (hmc_rows.hip) runs there, which is another kernel.
17 chains: two K = 1 blocks of 16 waves, the second with one.
"""
import numpy as np
import pytest
import torch

from philox_host import host_L_lnu

pytestmark = pytest.mark.gpu

N, NITER, WU, THIN, LO, HI, DT, SEED, N_SAVE = 17, 6, 2, 2, 1, 4, 0.1, 0xCA97, 3
# D -> (K, lanes per chain, chains per wave, wave kernel) of hmc_random_layout
LAYOUTS = {6: (1, 3, 21, 0), 66: (1, 64, 1, 1), 67: (1, 64, 1, 1), 130: (2, 64, 1, 1)}


def run(D, fp_mode, n_save):
    from hmc_amd.engine import RandomEngine
    from hmc_amd.target import MVNTarget
    eng = RandomEngine(MVNTarget(np.zeros(D), np.eye(D)), N, NITER, WU, THIN, LO, HI, DT, rng="philox", seed=SEED,
                       fp_mode=fp_mode, n_save=n_save)
    eng.init(np.random.RandomState(D).standard_normal((N, D)))
    eng.run(1, NITER + 1)
    torch.cuda.synchronize()
    return eng


@pytest.mark.parametrize("fp_mode", ["fast", "exact"])
@pytest.mark.parametrize("D", sorted(LAYOUTS))
def test_capture_instance_equals_production_instance(D, fp_mode):
    from hmc_amd import _lib as H
    assert H.random_layout(D, LO, HI) == LAYOUTS[D], "D = %d no longer selects the instance this case is for" % D
    cap, prod = run(D, fp_mode, N_SAVE), run(D, fp_mode, 0)
    assert cap.traj_stride == HI and prod.traj is None
    for k in ("q", "q_chain", "E_chain", "dE_chain", "E_prev"):
        assert torch.equal(getattr(cap, k).view(torch.int64), getattr(prod, k).view(torch.int64)), k   # bits
    assert np.array_equal(cap.read_counters(), prod.read_counters())
    # the captured trajectories hold the start point and one point per leapfrog step
    L, _ = host_L_lnu(SEED, np.zeros(1, dtype=np.uint64), NITER, LO, HI)
    assert np.array_equal(cap.traj_len.cpu().numpy()[:N_SAVE], L[0, :N_SAVE] + 1)
