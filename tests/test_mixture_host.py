"""Gaussian-mixture target, host side (no GPU): MixtureTarget's potential, gradient and moments, the
hmc_mixture struct mirror, and the argument validation of the four hmc_mix_* entries, which runs
before any device access (fake device pointers, as tests/test_abi.py drives invalid arguments)."""
import ctypes

import numpy as np
import pytest
from scipy.special import logsumexp
from scipy.stats import multivariate_normal


def _mixture(K, D, seed, sep=3.0):
    from hmc_amd.target import MixtureTarget
    rs = np.random.RandomState(seed)
    w = rs.uniform(0.5, 1.5, K)
    w /= w.sum()
    mu = rs.standard_normal((K, D))
    mu *= sep / np.linalg.norm(mu, axis=1, keepdims=True)
    var = rs.uniform(0.5, 2.0, (K, D))
    return MixtureTarget(w, mu, var), rs


@pytest.mark.parametrize("K,D", [(1, 1), (2, 2), (3, 37), (8, 130)])
def test_V_matches_scipy_logsumexp(K, D):
    t, rs = _mixture(K, D, 100 + K)
    assert (t.D, t.K) == (D, K) and t.q0.shape == (D,)
    for _ in range(8):
        q = t.mu[rs.randint(K)] + 1.5 * rs.standard_normal(D)
        want = -logsumexp([np.log(t.w[k]) + multivariate_normal.logpdf(q, t.mu[k], np.diag(t.variances[k]))
                           for k in range(K)])
        assert np.isclose(t.V(q), want, rtol=1e-12, atol=1e-12)
    # far from every mean exp() underflows without the max-shift: V must stay finite
    far = t.mu[0] + 40.0 * np.sqrt(t.variances.max()) * np.ones(D)
    assert np.isfinite(t.V(far)) and np.all(np.isfinite(t.dVdq(far)))
    # batched rows agree with single rows
    Q = rs.standard_normal((5, D))
    np.testing.assert_allclose(t.V(Q), [t.V(q) for q in Q], rtol=1e-14)
    np.testing.assert_allclose(t.dVdq(Q), [t.dVdq(q) for q in Q], rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("K,D", [(2, 2), (3, 37), (4, 100)])
def test_dVdq_matches_central_difference(K, D):
    """Central difference with step h = 1e-5 against dVdq.  Error model per coordinate d:
      truncation  h^2/6 |V'''|, and for V = -log sum_k exp(l_k) with l_k' = -a_kd (a = prec (q - mu)),
                  l_k'' = -prec_kd, l_k''' = 0:  V''' = -(kappa_3(l') + 3 cov(l', l'')), so
                  |V'''| <= R1^3 + 3 R1 R2 with R1 = range_k a_kd, R2 = range_k prec_kd;
      rounding    each V carries an error of about (D + K) eps max_k |l_k| (a D-term sum, then K
                  terms), and the difference divides two of them by 2h.
    The tolerance is the sum of the two bounds, computed from the inputs (about 1e-7 .. 1e-6)."""
    t, rs = _mixture(K, D, 7 + D)
    h, eps = 1e-5, np.finfo(float).eps
    for _ in range(4):
        q = t.mu[rs.randint(K)] + rs.standard_normal(D)
        g = t.dVdq(q)
        a = t.prec * (q - t.mu)                                   # (K, D)
        R1 = a.max(axis=0) - a.min(axis=0)
        R2 = t.prec.max(axis=0) - t.prec.min(axis=0)
        lmax = np.abs(t.logw - 0.5 * (t.logdet_const + np.sum(a * (q - t.mu), axis=1))).max()
        tol = h * h / 6.0 * (R1 ** 3 + 3 * R1 * R2) + (D + K) * eps * lmax / h
        for d in range(D):
            e = np.zeros(D)
            e[d] = h
            fd = (t.V(q + e) - t.V(q - e)) / (2 * h)
            assert abs(fd - g[d]) <= tol[d], (d, fd, g[d], tol[d])
        assert tol.max() < 1e-4                                   # the bound is a meaningful one


def test_moments():
    t, _ = _mixture(3, 5, 2)
    m = (t.w[:, None] * t.mu).sum(axis=0)
    np.testing.assert_allclose(t.mean(), m, rtol=1e-14)
    np.testing.assert_allclose(t.var(), (t.w[:, None] * (t.variances + t.mu ** 2)).sum(axis=0) - m ** 2, rtol=1e-13)
    np.testing.assert_array_equal(t.q0, t.mean())
    # against a large exact sample: 6 standard errors
    x = t.sample(200000, np.random.RandomState(0))
    assert np.all(np.abs(x.mean(axis=0) - t.mean()) < 6 * np.sqrt(t.var() / len(x)))


def test_constructor_assertions():
    from hmc_amd.target import MixtureTarget
    mu, var = np.zeros((2, 3)), np.ones((2, 3))
    MixtureTarget([0.25, 0.75], mu, var)
    for w in ([0.5, 0.6], [0.5, 0.5 + 1e-9], [1.5, -0.5], [1.0, 0.0]):
        with pytest.raises(AssertionError):
            MixtureTarget(w, mu, var)
    with pytest.raises(AssertionError):
        MixtureTarget([0.5, 0.5], mu, np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 1.0]]))
    with pytest.raises(AssertionError):
        MixtureTarget([0.5, 0.5], mu, -var)
    with pytest.raises(AssertionError):
        MixtureTarget([0.5, 0.5], mu, np.ones((2, 4)))
    with pytest.raises(AssertionError):
        MixtureTarget([1.0], mu, var)


def test_mixture_struct_layout():
    from hmc_amd import _lib as H
    assert ctypes.sizeof(H.Mixture) == 40
    assert [(n, getattr(H.Mixture, n).offset) for n, _ in H.Mixture._fields_] == \
        [("D", 0), ("K", 4), ("logw", 8), ("mu", 16), ("prec", 24), ("logdet_const", 32)]
    assert (H.MIX_MAX_COMPONENTS, H.MIX_MAX_D) == (8, 512)


def test_mix_entries_validate_before_any_launch(monkeypatch):
    """HMC_EINVAL for null arrays, D < 1, K < 1; HMC_ENOTSUP for D > 512, K > 8 and a full cov_p
    (minv_full, p_chol_t or kick): on the host, with fake device pointers that nothing reads."""
    from hmc_amd import _lib as H
    monkeypatch.setattr(H, "_lib", None)     # argtypes bound to this module's structure classes
    L = H.lib()
    P = 0x7000_0000
    K = H.Kinetic(None, None, None, 0.1, None, None, None)
    S = H.Schedule(4, 0, 10, 0, 1, 11, 5, 20, 1, 11, H.HMC_RNG_PHILOX, H.HMC_MODE_FAST, 10, 0, 0)
    st = H.State(P, P)

    def calls(M, Kin):
        return [L.hmc_mix_chain_init(M, Kin, S, None, P, st, None),
                L.hmc_mix_random_iters(M, Kin, S, None, st, None),
                L.hmc_mix_leapfrog(M, Kin, 4, P, P + 64, P + 128, P + 192, None),
                L.hmc_mix_energy(M, Kin, 4, P, P, P, None)]

    def mix(D=3, Kc=2, logw=P, mu=P, prec=P, ldc=P):
        return H.Mixture(D, Kc, logw, mu, prec, ldc)

    for bad in (mix(D=0), mix(Kc=0), mix(logw=None), mix(mu=None), mix(prec=None), mix(ldc=None)):
        assert calls(bad, K) == [H.HMC_EINVAL] * 4
        assert L.hmc_last_error()
    for bad in (mix(D=513), mix(Kc=9)):
        assert calls(bad, K) == [H.HMC_ENOTSUP] * 4
    for i in (4, 5, 6):                       # minv_full, p_chol_t, kick
        args = [None, None, None, 0.1, None, None, None]
        args[i] = P
        assert calls(mix(), H.Kinetic(*args)) == [H.HMC_ENOTSUP] * 4
    assert b"cov_p" in L.hmc_last_error()
    # the limits themselves pass this check: a wrong L_chain is then the schedule's HMC_EINVAL
    S.L_chain = 7
    assert L.hmc_mix_random_iters(mix(D=512, Kc=8), K, S, None, st, None) == H.HMC_EINVAL
    assert b"L_chain" in L.hmc_last_error()
    with pytest.raises(NotImplementedError):
        H.check(L.hmc_mix_energy(mix(D=513), K, 4, P, P, P, None), "x")
    # a diagonal mass and a per-dimension dt are supported: an empty batch returns HMC_OK untouched
    S.L_chain, S.n_chains = 11, 0
    assert L.hmc_mix_random_iters(mix(), H.Kinetic(P, P, P, 0.0, None, None, None), S, None, st, None) == H.HMC_OK
    assert L.hmc_mix_leapfrog(mix(), H.Kinetic(P, P, P, 0.0, None, None, None), 0, None, None, None, None, None) == \
        H.HMC_EINVAL   # outputs alias inputs (all NULL), as hmc_leapfrog


def test_sampler_refuses_unsupported_mixture_setups():
    """NUTS, a full cov_p, D > 512 and K > 8 raise NotImplementedError in the constructor, before
    anything touches a device."""
    from hmc_amd.samplers import HMC_sampler
    from hmc_amd.target import MixtureTarget
    t, _ = _mixture(2, 4, 1)
    kw = dict(Nchain=2, Niter=10, dt=0.1, device="cpu")
    with pytest.raises(NotImplementedError):
        HMC_sampler(4, None, None, sampler_type="NUTS", d_max=5, target=t, **kw)
    cov_p = np.eye(4)
    cov_p[0, 1] = cov_p[1, 0] = 0.2
    with pytest.raises(NotImplementedError):
        HMC_sampler(4, None, None, sampler_type="Random", L_low=5, L_high=20, cov_p=cov_p, target=t, **kw)
    big = MixtureTarget([1.0], np.zeros((1, 513)), np.ones((1, 513)))
    with pytest.raises(NotImplementedError):
        HMC_sampler(513, None, None, sampler_type="Random", L_low=5, L_high=20, target=big, **kw)
    many = MixtureTarget(np.full(9, 1.0 / 9), np.zeros((9, 2)), np.ones((9, 2)))
    with pytest.raises(NotImplementedError):
        HMC_sampler(2, None, None, sampler_type="Random", L_low=5, L_high=20, target=many, **kw)
    h = HMC_sampler(4, None, None, sampler_type="Random", L_low=5, L_high=20, cov_p=np.diag([0.9, 1.0, 1.1, 1.0]),
                    target=t, **kw)
    q = np.arange(4.0)
    assert h.V(q) == t.V(q) and np.array_equal(h.dVdq(q), t.dVdq(q))
