"""GLMTarget (hmc_amd/target.py) and the hmc_glm_* entries on the host: the struct mirror, the enum
and the prototypes, every HMC_EINVAL / HMC_ENOTSUP path of the six entries (all validation runs before
any device access), the NUTS workspace-size formula, the target's validation and its gradient against a
central difference of V, and the sampler's constructor (NUTS on a GLMTarget constructs, on a
LogisticTarget it still raises).  No GPU."""
import ctypes

import numpy as np
import pytest


def _glm(family, n, D, seed, prior="vector"):
    from hmc_amd.target import GLMTarget
    rs = np.random.RandomState(seed)
    X = 0.3 * rs.standard_normal((n, D))
    beta = rs.standard_normal(D)
    if family == "poisson":
        y = rs.poisson(np.exp(X @ beta)).astype(float)
    else:
        y = (rs.random_sample(n) < 1 / (1 + np.exp(-X @ beta))).astype(float)
    pv = rs.uniform(0.5, 2.0, D) if prior == "vector" else 1.7
    return GLMTarget(X, y, family, pv), rs


def _restated(t, q):
    """V and dV/dq of one row, from the formulas of include/hmc.h."""
    z = t.X @ q
    if t.family == "poisson":
        nll, mean = np.exp(z), np.exp(z)
    else:
        nll, mean = np.logaddexp(0.0, z), 1 / (1 + np.exp(-z))
    return np.sum(nll - t.y * z) + 0.5 * np.sum(q * q / t.prior_var), t.X.T @ (mean - t.y) + q / t.prior_var


# ------------------------------------------------------------------------------------------ target
@pytest.mark.parametrize("family", ["poisson", "bernoulli"])
@pytest.mark.parametrize("n,D,prior", [(1, 1, "scalar"), (20, 2, "vector"), (100, 37, "vector")])
def test_V_and_gradient_match_restatement(family, n, D, prior):
    t, rs = _glm(family, n, D, 100 + D, prior)
    assert (t.n, t.D, t.family) == (n, D, family) and t.diagonal is True
    assert t.family_id == {"bernoulli": 0, "poisson": 1}[family]
    assert np.array_equal(t.q0, np.zeros(D))
    q = 0.5 * rs.standard_normal((9, D))
    for row in q:
        V, g = _restated(t, row)
        np.testing.assert_allclose(t.V(row), V, rtol=1e-12)
        np.testing.assert_allclose(t.dVdq(row), g, rtol=1e-12, atol=1e-13)
    Vb, gb = t.V(q), t.dVdq(q)
    assert Vb.shape == (9,) and gb.shape == (9, D)
    np.testing.assert_allclose(Vb, [t.V(r) for r in q], rtol=1e-12)
    np.testing.assert_allclose(gb, [t.dVdq(r) for r in q], rtol=1e-12, atol=1e-13)
    q3 = q[:8].reshape(2, 4, D)
    assert t.V(q3).shape == (2, 4) and t.dVdq(q3).shape == (2, 4, D)


def test_bernoulli_is_the_logistic_posterior():
    from hmc_amd.target import LogisticTarget
    t, rs = _glm("bernoulli", 30, 5, 4)
    ref = LogisticTarget(t.X, t.y, t.prior_var)
    q = rs.standard_normal((6, 5))
    assert np.array_equal(t.V(q), ref.V(q)) and np.array_equal(t.dVdq(q), ref.dVdq(q))


def test_poisson_overflow_is_inf_not_an_error():
    from hmc_amd.target import GLMTarget
    t = GLMTarget(np.array([[1.0, 0.5], [0.5, 1.0]]), np.array([3.0, 0.0]), "poisson")
    with np.errstate(over="raise"):                      # the target silences its own overflow
        assert t.V(np.array([709.0, 0.0])) < np.inf
        assert t.V(np.array([710.0, 0.0])) == np.inf
        g = t.dVdq(np.array([710.0, 0.0]))
    assert np.all(g == np.inf)
    assert np.isfinite(t.V(np.array([-1e4, -1e4])))


@pytest.mark.parametrize("family", ["poisson", "bernoulli"])
@pytest.mark.parametrize("n,D", [(20, 2), (60, 17)])
def test_gradient_against_central_differences(family, n, D):
    """|fd - g_d| <= h^2/6 max|V'''_d| + (n + D) eps |V| / h.  The third derivative along dim d is
    sum_j X_jd^3 f'''(z_j): f''' = exp(z) for Poisson, bounded here by exp(max z + h max|X|);
    |sigma''| <= 1 / (6 sqrt 3) for Bernoulli.  The quadratic prior has none."""
    t, rs = _glm(family, n, D, 7 + D)
    h, eps = 1e-5, np.finfo(float).eps
    for q in 0.5 * rs.standard_normal((4, D)):
        z = t.X @ q
        f3 = np.exp(z + h * np.abs(t.X).max()) if family == "poisson" else np.full(n, 1 / (6 * np.sqrt(3)))
        third = np.abs(t.X.T) ** 3 @ f3
        g = t.dVdq(q)
        tol = h * h / 6 * third + (n + D) * eps * abs(t.V(q)) / h
        for d in range(D):
            e = np.zeros(D)
            e[d] = h
            fd = (t.V(q + e) - t.V(q - e)) / (2 * h)
            assert abs(fd - g[d]) <= tol[d], (d, fd, g[d], tol[d])
        assert tol.max() < 1e-4                                   # the bound is a meaningful one


def test_constructor_assertions():
    from hmc_amd.target import GLMTarget
    X = np.ones((4, 3))
    GLMTarget(X, np.array([0.0, 3.0, 1.0, 7.0]))                                  # poisson is the default
    GLMTarget(X, np.array([0, 3, 1, 7]), "poisson", prior_var=[1.0, 2.0, 3.0])
    GLMTarget(X, np.array([0.0, 1.0, 1.0, 0.0]), "bernoulli", prior_var=2.0)
    GLMTarget(X, np.array([0, 1, 1, 0]) > 0, family="bernoulli")
    for bad_y in (np.array([0.0, 1.0, 2.0, 0.0]), np.array([0.0, 0.5, 1.0, 0.0]), np.array([0.0, 1.0, -1.0, 0.0]),
                  np.array([0.0, 1.0, np.nan, 0.0])):
        with pytest.raises(AssertionError):
            GLMTarget(X, bad_y, "bernoulli")
    for bad_y in (np.array([0.0, 1.5, 2.0, 0.0]), np.array([0.0, 1.0, -1.0, 0.0]), np.array([0.0, 1.0, np.nan, 0.0]),
                  np.array([0.0, 1.0, np.inf, 0.0]), np.zeros(3), np.zeros((4, 1))):
        with pytest.raises(AssertionError):
            GLMTarget(X, bad_y, "poisson")
    for bad_family in ("gaussian", "Poisson", None, 1):
        with pytest.raises(AssertionError):
            GLMTarget(X, np.zeros(4), bad_family)
    for bad_X in (np.ones(4), np.ones((0, 3)), np.ones((4, 0)), np.ones((4, 3, 1))):
        with pytest.raises(AssertionError):
            GLMTarget(bad_X, np.zeros(bad_X.shape[0]))
    for bad_pv in (0.0, -1.0, [1.0, 1.0], [1.0, 0.0, 1.0], np.ones((3, 1))):
        with pytest.raises(AssertionError):
            GLMTarget(X, np.zeros(4), prior_var=bad_pv)


# ------------------------------------------------------------------------------------------ C ABI
def test_glm_struct_enum_and_prototypes():
    from hmc_amd import _lib as H
    assert ctypes.sizeof(H.GLM) == 48
    assert [(n, getattr(H.GLM, n).offset) for n, _ in H.GLM._fields_] == \
        [("D", 0), ("n", 4), ("ldx", 8), ("X", 16), ("y", 24), ("prior_prec", 32), ("family", 40)]
    assert (H.HMC_GLM_BERNOULLI, H.HMC_GLM_POISSON) == (0, 1)
    L = H.lib()                                           # every declared symbol is exported
    g, k, s, r, st = (ctypes.POINTER(c) for c in (H.GLM, H.Kinetic, H.Schedule, H.Replay, H.State))
    dp, i64, i32 = H.c_dp, ctypes.c_int64, ctypes.c_int32
    want = {
        "hmc_glm_chain_init": (ctypes.c_int, [g, k, s, r, dp, st, dp]),
        "hmc_glm_random_iters": (ctypes.c_int, [g, k, s, r, st, dp]),
        "hmc_glm_leapfrog": (ctypes.c_int, [g, k, i64, dp, dp, dp, dp, dp]),
        "hmc_glm_energy": (ctypes.c_int, [g, k, i64, dp, dp, dp, dp]),
        "hmc_glm_nuts_workspace_size": (i64, [i32, i64, i32]),
        "hmc_glm_nuts_iters": (ctypes.c_int, [g, k, s, r, st, dp, i64, dp]),
    }
    for name, (res, args) in want.items():
        assert H.SYMBOLS[name] == (res, args), name
        assert getattr(L, name) is not None
    # argument for argument the hmc_logit_* entries, with hmc_glm in place of hmc_logistic
    for a, b in (("chain_init", "chain_init"), ("random_iters", "random_iters"), ("leapfrog", "leapfrog"),
                 ("energy", "energy")):
        la, ga = H.SYMBOLS["hmc_logit_" + a][1], H.SYMBOLS["hmc_glm_" + b][1]
        assert la[1:] == ga[1:] and la[0] == ctypes.POINTER(H.Logistic)


def test_nuts_workspace_size_formula():
    """Per 16-chain tile 8 + 2 (d_max + 1) vectors of 16 MT dims times 64 lanes... i.e. 4 MT registers
    of 64 lanes each, then 16 int64 tape cursors; MT = 1, 2, 4, 8 covers D <= 16, 32, 64, 128."""
    from hmc_amd import _lib as H
    size = H.lib().hmc_glm_nuts_workspace_size
    for D, MT in ((1, 1), (16, 1), (17, 2), (32, 2), (33, 4), (64, 4), (65, 8), (128, 8)):
        for N in (1, 16, 17, 100):
            for d_max in (1, 5, 30):
                tiles = (N + 15) // 16
                assert size(D, N, d_max) == 8 * (tiles * (8 + 2 * (d_max + 1)) * 4 * MT * 64 + tiles * 16), (D, N, d_max)
    assert size(8, 0, 5) == 0
    for bad in ((0, 4, 5), (129, 4, 5), (8, -1, 5), (8, 4, 0), (8, 4, 31)):
        assert size(*bad) == 0, bad


def test_glm_entries_validate_before_any_launch(monkeypatch):
    """On the host, with fake device pointers that nothing reads.  HMC_EINVAL: a null descriptor or
    array, D < 1, n < 1, ldx < D, an unknown family, and for NUTS a null or too small workspace.
    HMC_ENOTSUP: D > 128, n > 2^20, a full cov_p, and for NUTS d_max outside 1 .. 30."""
    from hmc_amd import _lib as H
    monkeypatch.setattr(H, "_lib", None)     # argtypes bound to this module's structure classes
    L = H.lib()
    P = 0x7000_0000
    K = H.Kinetic(None, None, None, 0.1, None, None, None)
    st = H.State(P, P)

    def sched(d_max=5, n_chains=4, L_chain=11):
        return H.Schedule(n_chains, 0, 10, 0, 1, L_chain, 5, 20, 1, 11, H.HMC_RNG_PHILOX, H.HMC_MODE_FAST, d_max, 0, 0)

    S = sched()
    big = 1 << 40

    def calls(M, Kin):
        return [L.hmc_glm_chain_init(M, Kin, S, None, P, st, None),
                L.hmc_glm_random_iters(M, Kin, S, None, st, None),
                L.hmc_glm_leapfrog(M, Kin, 4, P, P + 64, P + 128, P + 192, None),
                L.hmc_glm_energy(M, Kin, 4, P, P, P, None),
                L.hmc_glm_nuts_iters(M, Kin, S, None, st, P, big, None)]

    def glm(D=3, n=5, ldx=None, X=P, y=P, prec=P, family=H.HMC_GLM_POISSON):
        return H.GLM(D, n, D if ldx is None else ldx, X, y, prec, family)

    for bad in (glm(D=0), glm(n=0), glm(D=-1), glm(n=-3), glm(ldx=2), glm(X=None), glm(y=None), glm(prec=None),
                glm(family=2), glm(family=-1), None):
        assert calls(bad, K) == [H.HMC_EINVAL] * 5
        assert L.hmc_last_error()
    assert L.hmc_glm_energy(glm(family=7), K, 4, P, P, P, None) == H.HMC_EINVAL
    assert b"family" in L.hmc_last_error()
    for family in (H.HMC_GLM_BERNOULLI, H.HMC_GLM_POISSON):
        for bad in (glm(D=129, family=family), glm(n=(1 << 20) + 1, family=family)):
            assert calls(bad, K) == [H.HMC_ENOTSUP] * 5
        for i in (4, 5, 6):                       # minv_full, p_chol_t, kick
            args = [None, None, None, 0.1, None, None, None]
            args[i] = P
            assert calls(glm(family=family), H.Kinetic(*args)) == [H.HMC_ENOTSUP] * 5
        assert b"cov_p" in L.hmc_last_error()
    # NUTS: d_max, the workspace pointer and its size
    for d_max in (0, -1, 31):
        assert L.hmc_glm_nuts_iters(glm(), K, sched(d_max), None, st, P, big, None) == H.HMC_ENOTSUP
        assert b"d_max" in L.hmc_last_error()
    assert L.hmc_glm_nuts_iters(glm(), K, S, None, st, None, big, None) == H.HMC_EINVAL
    assert b"workspace" in L.hmc_last_error()
    need = L.hmc_glm_nuts_workspace_size(3, 4, 5)
    assert need > 0
    for small in (0, 8, need - 1):
        assert L.hmc_glm_nuts_iters(glm(), K, S, None, st, P, small, None) == H.HMC_EINVAL
        assert b"workspace" in L.hmc_last_error()
    with pytest.raises(AssertionError):
        H.check(L.hmc_glm_nuts_iters(glm(), K, S, None, st, P, need - 1, None), "x")
    with pytest.raises(NotImplementedError):
        H.check(L.hmc_glm_nuts_iters(glm(), K, sched(31), None, st, P, big, None), "x")
    # replay mode without its streams; a bad iteration range; a wrong L_chain
    Sr = sched()
    Sr.rng_mode = H.HMC_RNG_REPLAY
    assert L.hmc_glm_nuts_iters(glm(), K, Sr, None, st, P, big, None) == H.HMC_EINVAL
    assert L.hmc_glm_nuts_iters(glm(), K, Sr, H.Replay(P, P, None, None, None, 0), st, P, big, None) == H.HMC_EINVAL
    Sb = sched()
    Sb.iter_begin = 0
    assert L.hmc_glm_nuts_iters(glm(), K, Sb, None, st, P, big, None) == H.HMC_EINVAL
    assert L.hmc_glm_nuts_iters(glm(D=128, n=1 << 20, ldx=200), K, sched(L_chain=7), None, st, P, big, None) == \
        H.HMC_EINVAL
    assert b"L_chain" in L.hmc_last_error()
    assert L.hmc_glm_nuts_iters(glm(), K, S, None, None, P, big, None) == H.HMC_EINVAL
    # an empty batch and an empty iteration range return HMC_OK untouched (a diagonal mass and a
    # per-dimension dt are supported)
    Kd = H.Kinetic(P, P, P, 0.0, None, None, None)
    S0 = sched(n_chains=0)
    assert L.hmc_glm_chain_init(glm(), Kd, S0, None, None, st, None) == H.HMC_OK
    assert L.hmc_glm_random_iters(glm(), Kd, S0, None, st, None) == H.HMC_OK
    assert L.hmc_glm_nuts_iters(glm(), Kd, S0, None, st, None, 0, None) == H.HMC_OK
    assert L.hmc_glm_energy(glm(), Kd, 0, None, None, None, None) == H.HMC_OK
    Se = sched()
    Se.iter_end = Se.iter_begin
    assert L.hmc_glm_nuts_iters(glm(), Kd, Se, None, st, P, need, None) == H.HMC_OK
    assert L.hmc_glm_random_iters(glm(), Kd, Se, None, st, None) == H.HMC_OK


# ------------------------------------------------------------------------------------------ sampler
def test_sampler_constructs_nuts_on_glm_and_still_refuses_it_on_logistic():
    from hmc_amd.samplers import HMC_sampler
    from hmc_amd.target import GLMTarget, LogisticTarget
    kw = dict(Nchain=2, Niter=10, dt=0.1, device="cpu")
    for family in ("poisson", "bernoulli"):
        t, _ = _glm(family, 12, 4, 1)
        h = HMC_sampler(4, None, None, sampler_type="NUTS", d_max=5, target=t, **kw)
        q = np.arange(4.0) / 4
        assert h.d_max == 5 and h.V(q) == t.V(q) and np.array_equal(h.dVdq(q), t.dVdq(q))
        HMC_sampler(4, None, None, sampler_type="Random", L_low=5, L_high=20, cov_p=np.diag([0.9, 1.0, 1.1, 1.0]),
                    target=t, **kw)
        cov_p = np.eye(4)
        cov_p[0, 1] = cov_p[1, 0] = 0.2
        for st in (dict(sampler_type="NUTS", d_max=5), dict(sampler_type="Random", L_low=5, L_high=20)):
            with pytest.raises(NotImplementedError):
                HMC_sampler(4, None, None, cov_p=cov_p, target=t, **st, **kw)
    t, _ = _glm("bernoulli", 12, 4, 1)
    with pytest.raises(NotImplementedError):
        HMC_sampler(4, None, None, sampler_type="NUTS", d_max=5, target=LogisticTarget(t.X, t.y, t.prior_var), **kw)
    wide = GLMTarget(np.zeros((2, 129)), np.array([0.0, 1.0]))
    with pytest.raises(NotImplementedError):
        HMC_sampler(129, None, None, sampler_type="NUTS", d_max=5, target=wide, **kw)
    n = (1 << 20) + 1
    tall = GLMTarget(np.zeros((n, 1)), np.zeros(n))
    with pytest.raises(NotImplementedError):
        HMC_sampler(1, None, None, sampler_type="Random", L_low=5, L_high=20, target=tall, **kw)
