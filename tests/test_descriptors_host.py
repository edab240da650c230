"""Host layer of hmc_amd.descriptors (no GPU; only the large-D cases load the library, host-only):
the rules that turn (target, cov_p, dt, dense) into the arrays of hmc_target / hmc_kinetic, the one
table of targets with kernels of their own, and the large-D test of the workspace allocation."""
import ctypes
import hashlib

import numpy as np
import pytest

from hmc_amd import _lib as H
from hmc_amd import descriptors as Dsc
from hmc_amd.target import GLMTarget, LogisticTarget, MixtureTarget, MVNTarget

D = 3
KINETIC_ARRAYS = ("minv", "p_scale", "dt_vec", "minv_full", "p_chol_t", "kick")
FULL_COV_P = np.array([[2.0, 0.3, 0.1], [0.3, 1.5, -0.2], [0.1, -0.2, 1.2]])
DENSE_PREC = np.linalg.inv(np.array([[1.0, 0.4, 0.0], [0.4, 2.0, 0.5], [0.0, 0.5, 3.0]]))


def same(a, b):
    return a is not None and a.dtype == np.float64 and a.shape == b.shape and np.array_equal(a, b)


def test_identity_mass_scalar_dt():
    for cov_p in (None, np.eye(D)):
        kin = Dsc.host_kinetic(D, cov_p, 0.1)
        assert all(getattr(kin, a) is None for a in KINETIC_ARRAYS)
        assert kin.dt == 0.1 and isinstance(kin.dt, float)


def test_diagonal_mass():
    cov_p = np.diag([0.5, 2.0, 3.0])
    kin = Dsc.host_kinetic(D, cov_p, 0.1)
    assert same(kin.minv, np.diag(np.linalg.inv(cov_p)))
    assert same(kin.p_scale, np.sqrt(np.diag(cov_p)))
    assert kin.minv_full is None and kin.p_chol_t is None and kin.kick is None and kin.dt_vec is None


@pytest.mark.parametrize("prec", [DENSE_PREC, np.diag([1.0, 2.0, 4.0])], ids=["dense", "diagonal"])
def test_full_mass(prec):
    """A full cov_p: the dense kind even for a diagonal target, and p_chol_t only where asked."""
    t = MVNTarget(np.zeros(D), prec=prec)
    for chol in (True, False):
        mvn, kin = Dsc.host_descriptors(t, FULL_COV_P, 0.1, chol=chol)
        assert mvn.kind == H.HMC_TARGET_DENSE and same(mvn.prec, t.prec) and mvn.prec.shape == (D, D)
        assert same(kin.minv_full, np.linalg.inv(FULL_COV_P))
        assert same(kin.kick, np.linalg.inv(FULL_COV_P) @ t.prec)
        assert kin.minv is None and kin.p_scale is None
        if chol:
            assert same(kin.p_chol_t, np.linalg.cholesky(FULL_COV_P).T)
        else:
            assert kin.p_chol_t is None


def test_vector_dt():
    dt = np.array([0.1, 0.2, 0.3])
    kin = Dsc.host_kinetic(D, None, dt)
    assert same(kin.dt_vec, dt) and kin.dt == 0.0
    assert same(Dsc.host_kinetic(D, None, dt.reshape(D, 1)).dt_vec, dt)
    for bad in (np.ones(D + 1), np.ones(D - 1)):
        with pytest.raises(AssertionError):
            Dsc.host_kinetic(D, None, bad)


def test_diagonal_target():
    mvn = Dsc.host_mvn(MVNTarget(np.zeros(D), np.eye(D)))
    assert mvn == (H.HMC_TARGET_DIAG, None, None)
    q0 = np.array([1.0, -2.0, 0.5])
    mvn = Dsc.host_mvn(MVNTarget(q0, np.eye(D)))
    assert mvn.kind == H.HMC_TARGET_DIAG and same(mvn.q0, q0) and mvn.prec is None
    t = MVNTarget(np.zeros(D), np.diag([0.5, 2.0, 4.0]))
    mvn = Dsc.host_mvn(t)
    assert mvn.kind == H.HMC_TARGET_DIAG and mvn.q0 is None
    assert same(mvn.prec, np.diag(t.prec)) and mvn.prec.shape == (D,)
    mvn = Dsc.host_mvn(t, dense=True)
    assert mvn.kind == H.HMC_TARGET_DENSE and same(mvn.prec, t.prec) and mvn.prec.shape == (D, D)
    mvn = Dsc.host_mvn(MVNTarget(np.zeros(D), prec=DENSE_PREC))
    assert mvn.kind == H.HMC_TARGET_DENSE and same(mvn.prec, DENSE_PREC)


def _digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def _kernel_targets():
    rng = np.random.RandomState(0)
    X = rng.standard_normal((4, D))
    mix = MixtureTarget([0.3, 0.7], rng.standard_normal((2, D)), 0.5 + rng.random_sample((2, D)))
    logit = LogisticTarget(X, [0, 1, 1, 0], prior_var=2.0)
    glms = [GLMTarget(X, [0, 1, 1, 0], family="bernoulli", prior_var=[1.0, 2.0, 3.0]),
            GLMTarget(X, [0, 3, 1, 2], family="poisson")]
    yield mix, (mix.logw, mix.mu, mix.prec, mix.logdet_const), ()
    yield logit, (logit.X, logit.y, logit.prior_prec), ()
    for g in glms:
        yield g, (g.X, g.y, g.prior_prec), (np.float64(g.family_id),)


def test_kernel_target_table():
    """Each row lists the target's arrays once: the device descriptor takes them in that order and a
    checkpoint fingerprints them in that order, a GLM's family id last."""
    from hmc_amd.engine import KERNEL_TARGETS, kernel_target
    assert set(KERNEL_TARGETS) == {MixtureTarget, LogisticTarget, GLMTarget}
    assert kernel_target(MVNTarget(np.zeros(D), np.eye(D))) is None
    for t, arrays, last in _kernel_targets():
        row = kernel_target(t)
        assert row is KERNEL_TARGETS[type(t)]
        got = row.arrays(t)
        assert len(got) == len(arrays) and all(a is b for a, b in zip(got, arrays))
        assert Dsc.fingerprint(row.fingerprint_arrays(t)) == _digest(arrays + last)
    assert [r.name for r in KERNEL_TARGETS.values()] == ["mixture", "logistic", "GLM"]
    assert [r.nuts_engine is not None for r in KERNEL_TARGETS.values()] == [False, False, True]


def test_kernel_target_limits():
    from hmc_amd.engine import kernel_target
    t = MixtureTarget(np.full(9, 1.0 / 9), np.zeros((9, D)), np.ones((9, D)))
    with pytest.raises(NotImplementedError, match=r"mixture kernels: D=3, K=9 \(D <= 512, K <= 8\)"):
        kernel_target(t).check(t)
    t = GLMTarget(np.ones((2, 129)), [0, 1])
    with pytest.raises(NotImplementedError, match=r"GLM kernels: D=129, n=2 \(D <= 128, n <= 1048576\)"):
        kernel_target(t).check(t)
    with pytest.raises(NotImplementedError, match="GLM kernels: a full cov_p is not supported"):
        kernel_target(t).engine.check_supported(GLMTarget(np.ones((2, D)), [0, 1]), FULL_COV_P)


@pytest.fixture
def library(monkeypatch):
    monkeypatch.setattr(H, "_lib", None)     # argtypes bound to this module's structure classes
    return H.lib()


def _ws_bytes(library, kind, D_, full_mass):
    T = H.Target(D_, kind, None, None, 0.0)
    K = H.Kinetic(None, None, None, 0.1, None, None, None)
    return library.hmc_random_workspace_size_ex(ctypes.byref(T), None if full_mass else ctypes.byref(K), 1)


def test_large_d_helper_matches_library(library):
    """RandomEngine._large_d against the library's own answers (host-only size queries, one chain).
    Diagonal kind: hmc_random_workspace_size_ex is 0 off the large-D path and the chain state's size
    on it.  Dense kind: the query is positive on both sides of the edge (tile scratch below, chain
    state above), but only the large-D chain state holds the products of a full cov_p, so the size
    asked with a kinetic descriptor that has none differs from the size for either cov_p (a NULL
    descriptor) exactly on the large-D path."""
    from hmc_amd.engine import RandomEngine
    large_d = RandomEngine._large_d
    for D_ in (1, 2048, 2049, 2050):
        assert large_d(H.HMC_TARGET_DIAG, D_) == (_ws_bytes(library, H.HMC_TARGET_DIAG, D_, False) > 0), D_
    assert not large_d(H.HMC_TARGET_DIAG, 2048) and large_d(H.HMC_TARGET_DIAG, 2049)
    for D_ in (1, 128, 129, 130):
        some, either = (_ws_bytes(library, H.HMC_TARGET_DENSE, D_, f) for f in (False, True))
        assert some > 0 and either >= some
        assert large_d(H.HMC_TARGET_DENSE, D_) == (either != some), D_
    assert not large_d(H.HMC_TARGET_DENSE, 128) and large_d(H.HMC_TARGET_DENSE, 129)
