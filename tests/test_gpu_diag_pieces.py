"""Three diagnostics entry points that had no direct test, each against a float64 NumPy
restatement on small shapes:
  * hmc_split_moments (k_split_moments): per-split-chain mean and std (ddof 1);
  * hmc_variogram with t0 > 1: the delayed-stream lag groups of the VALU pass (gofs > 0);
  * hmc_stream_accumulate on halves shorter than tmax: the difference-form kernel, its whole-chunk
    branch, its masked branch and the half boundary."""
import numpy as np
import pytest
import torch

from oracle import hmc_oracle as O

pytestmark = pytest.mark.gpu


def _ar1(N, Niter, D, seed):
    """AR(1) chains around a per-dim offset of about 5 (as test_gpu_convergence_sums.py)."""
    rng = np.random.default_rng(seed)
    q = np.empty((N, Niter, D))
    q[:, 0] = rng.normal(size=(N, D))
    for t in range(1, Niter):
        q[:, t] = 0.8 * q[:, t - 1] + rng.normal(size=(N, D))
    return q + rng.normal(size=D) * 5.0


def _split(view, n):
    """(2N, n, D): split chain 2m + h = view[m, h n : (h + 1) n]."""
    N, _, D = view.shape
    return np.stack([view[:, :n], view[:, n:2 * n]], axis=1).reshape(2 * N, n, D)


@pytest.mark.parametrize("N,Niter,D,thin,wu", [
    (3, 10, 70, 1, 0),     # n = 5; two dim tiles, the second ragged; 6 split chains: a ragged last block
    (2, 23, 3, 2, 1),      # thinned, warm-up-offset view: n = 5
])
def test_split_moments_vs_numpy(N, Niter, D, thin, wu):
    """At most 11 terms per sum and condition numbers below 1e2 for this data: rtol 1e-12."""
    from hmc_amd.diagnostics import _Split, split_moments
    q = _ar1(N, Niter, D, seed=N + Niter + D)
    sp = _Split(torch.as_tensor(q).cuda(), thin, wu)
    assert sp.n == 5
    mean, std = split_moments(sp)
    xs = _split(q[:, wu::thin], sp.n)
    np.testing.assert_allclose(mean.cpu().numpy(), xs.mean(axis=1), rtol=1e-12)
    np.testing.assert_allclose(std.cpu().numpy(), xs.std(axis=1, ddof=1), rtol=1e-12)


@pytest.fixture(scope="module", params=[7, 100])
def lag_view(request):
    """N = 3 chains of 2 n = 260 samples and their difference-form lag sums, every lag 1 .. n - 1."""
    from hmc_amd.diagnostics import _Split
    N, n, D = 3, 130, request.param
    q = _ar1(N, 2 * n, D, seed=D)
    xs = _split(q, n)
    want = np.stack([((xs[:, t:] - xs[:, :-t]) ** 2).sum(axis=(0, 1)) for t in range(1, n)])
    want.setflags(write=False)
    sp = _Split(torch.as_tensor(q).cuda(), 1, 0)
    assert sp.n == n
    return sp, want


@pytest.mark.parametrize("t0,t1", [
    (1, 5),         # L0 = 0
    (17, 41),       # L0 = 16, skip 0: one delayed group
    (20, 100),      # L0 = 16, skip 3: two groups, the second ragged
    (120, 130),     # gofs + 1 close to n; the last lag is n - 1
])
def test_variogram_range_vs_numpy(lag_view, t0, t1):
    from hmc_amd.diagnostics import variogram_sums
    sp, want_all = lag_view
    want = want_all[t0 - 1:t1 - 1]
    got = variogram_sums(sp, t0, t1).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-9 * np.abs(want).max())


@pytest.mark.parametrize("N,D,L,tmax,segs", [
    (5, 70, 23, 16, (3, 8)),     # n = 11; segments of 8 = the kernel's chunk: whole-chunk and masked rows
    (5, 3, 11, 8, (4,)),         # n = 5
])
def test_stream_segments_short_halves(N, D, L, tmax, segs):
    """Segment mode on halves of n < tmax samples (the difference form): lag sums, split moments
    and R-hat against NumPy and the oracle (the module's 1e-10: fp64 sums in another order)."""
    from hmc_amd.diagnostics import StreamingDiagnostics
    q = _ar1(N, L, D, seed=L + D)
    n = L // 2
    assert n < tmax                                        # the host's rule for the difference form
    xs = _split(q, n)
    want_v = np.stack([((xs[:, t:] - xs[:, :-t]) ** 2).sum(axis=(0, 1)) for t in range(1, n)])
    R_ref, _ = O.convergence_stats(q, thin_rate=1, warm_up_num=0)
    x = torch.as_tensor(q).cuda()
    for seg in segs:
        sd = StreamingDiagnostics(N, D, L, tmax=tmax, mode="stream")
        assert sd.n == n
        p = 0
        while p < L:
            rows = min(seg, L - p)
            carry = min(tmax, p)
            sd.update(x[:, p - carry:p + rows, :], carry, rows)
            p += rows
        got_v = sd.vsum[:n - 1].cpu().numpy()
        np.testing.assert_allclose(got_v, want_v, rtol=1e-10, atol=1e-9 * np.abs(want_v).max())
        mean, std = sd.moments()
        np.testing.assert_allclose(mean.cpu().numpy(), xs.mean(axis=1), rtol=1e-10)
        np.testing.assert_allclose(std.cpu().numpy(), xs.std(axis=1, ddof=1), rtol=1e-10)
        R, _ = sd.finish()
        np.testing.assert_allclose(R, R_ref, rtol=1e-10)
