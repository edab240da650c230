"""Posterior predictive reductions, the parts that need no GPU.

(a) The merge rule as hmc_pred.hip compiles it (csrc/hmc_pred.hpp::pred_merge, behind the host
    program pred_host that make builds next to libhmc.so) against hmc_amd.predictive.merge_partials
    at 1e-12 and against the two-pass reference of tests/test_gpu_predictive.py on the concatenated
    data under that file's tolerance rule; records carrying -inf, records carrying NaN and the n = 0
    record (the identity) included.
(b) hmc_amd.predictive.finish against the closed forms.
(c) The surface: every host-side refusal of hmc_glm_predictive, the empty cases, the sample-block
    rule as a function of the shapes, hmc_samples against include/hmc.h, and the sampler methods'
    refusals."""
import ctypes
import os
import re
import subprocess
from math import lgamma

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_predictive import check_records, records_of


def _host(records):
    from hmc_amd import _lib
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), "pred_host")
    assert os.path.exists(exe), f"{exe} not found: build it with make -C understanding-hmc_amd/csrc"
    text = "\n".join(" ".join(repr(float(v)) for v in r) for r in records) + "\n"
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout
    row = np.array([float(x) for x in out.split()])
    assert row.shape == (8,)
    return row


def _fold(records):
    from hmc_amd.predictive import merge_partials
    acc = np.asarray(records[0], dtype=np.float64)[None]
    for r in records[1:]:
        acc = merge_partials(acc, np.asarray(r, dtype=np.float64)[None])
    return acc[0]


def _chunks(kind):
    """(mu, ll) chunks of one evaluation row's values."""
    rs = np.random.RandomState({"plain": 1, "concentrated": 2, "neg_inf": 3, "all_neg_inf": 4, "nan": 5}[kind])
    sizes = [1, 16, 7, 300, 2, 41]
    if kind == "concentrated":                       # counts ~ e^6 within 3e-3: the cancellation case
        z = [6.0 + 3e-3 * rs.standard_normal(n) for n in sizes]
    else:
        z = [0.3 + 0.8 * rs.standard_normal(n) for n in sizes]
    y = 3.0
    with np.errstate(over="ignore", invalid="ignore"):
        chunks = [(np.exp(v), y * v - np.exp(v)) for v in z]
    if kind == "neg_inf":                            # mu = +inf, ll = -inf in two chunks
        for k in (1, 3):
            chunks[k][0][::5], chunks[k][1][::5] = np.inf, -np.inf
    if kind == "all_neg_inf":
        chunks = [(np.full(n, np.inf), np.full(n, -np.inf)) for n in sizes]
    if kind == "nan":
        chunks[3][0][17], chunks[3][1][17] = np.nan, np.nan
    return chunks


@pytest.mark.parametrize("kind", ["plain", "concentrated", "neg_inf", "all_neg_inf", "nan"])
def test_merge_rule_matches_numpy_and_the_two_pass_reference(kind):
    chunks = _chunks(kind)
    recs = [records_of(mu[None], ll[None])[0] for mu, ll in chunks]
    # n = 0 records are the identity, whatever their other slots hold
    recs = [np.zeros(8)] + recs[:2] + [np.array([0.0] + [np.nan] * 6 + [0.0])] + recs[2:] + [np.zeros(8)]
    got = _host(recs)
    mine = _fold(recs)
    np.testing.assert_allclose(got, mine, rtol=1e-12, atol=0, equal_nan=True)
    mu, ll = (np.concatenate([c[k] for c in chunks]) for k in (0, 1))
    r64 = records_of(mu[None], ll[None])
    r80 = records_of(mu[None].astype(np.longdouble), ll[None].astype(np.longdouble))
    check_records(got[None], r64, r80, "pred_host %s" % kind)
    check_records(mine[None], r64, r80, "merge_partials %s" % kind)
    if kind == "neg_inf":
        assert got[1] == np.inf and np.isnan(got[2]) and got[3] == -np.inf and np.isnan(got[4])
        assert np.isfinite(got[5]) and got[6] >= 1.0
    if kind == "all_neg_inf":
        assert got[3] == -np.inf and got[5] == -np.inf and got[6] == 0.0
    if kind == "nan":
        assert got[0] == len(mu) and got[7] == 0.0 and np.isnan(got[1:7]).all()


def test_merge_identity_and_no_records():
    from hmc_amd.predictive import merge_partials
    assert np.array_equal(_host([]), np.zeros(8))
    r = np.array([5.0, 1.5, 0.25, -2.0, 0.5, -1.0, 3.5, 0.0])
    assert np.array_equal(_host([r]), r) and np.array_equal(_host([np.zeros(8), r, np.zeros(8)]), r)
    assert np.array_equal(merge_partials(r[None], np.zeros((1, 8)))[0], r)
    assert np.array_equal(merge_partials(np.zeros((1, 8)), r[None])[0], r)
    # y = None records (slots 3-6 NaN) keep their moments of mu
    a = np.array([4.0, 1.0, 2.0] + [np.nan] * 4 + [0.0])
    b = np.array([12.0, 3.0, 1.0] + [np.nan] * 4 + [0.0])
    got = _host([a, b])
    assert got[0] == 16.0 and got[1] == 1.0 + 2.0 * 0.75 and got[2] == 3.0 + 4.0 * (4.0 * 12.0 / 16.0)
    assert np.isnan(got[3:7]).all()
    np.testing.assert_array_equal(got, merge_partials(a[None], b[None])[0])


# ------------------------------------------------------------------------------------------ finish
def test_finish_closed_forms():
    from hmc_amd.predictive import finish
    n = 50.0
    p = np.array([[n, 0.3, 0.49, -1.2, 4.9, -0.4, 7.5, 0.0],
                  [n, 2.5, 9.8, -3.0, 0.98, -2.0, 20.0, 0.0],
                  [n, 0.9, 0.0, -0.1, 0.0, -0.1, 50.0, 0.0]])
    y = np.array([0.0, 4.0, 1.0])
    lppd_i = p[:, 5] + np.log(p[:, 6]) - np.log(n)
    p_i = p[:, 4] / (n - 1)
    for family, const in (("bernoulli", 0.0), ("poisson", np.array([lgamma(v + 1) for v in y]))):
        f = finish(p, y, family)
        np.testing.assert_array_equal(f["mean"], p[:, 1])
        var = p[:, 1] * (1 - p[:, 1]) if family == "bernoulli" else p[:, 1] + p[:, 2] / (n - 1)
        np.testing.assert_allclose(f["var"], var, rtol=1e-15)
        np.testing.assert_allclose(f["lppd_i"], lppd_i - const, rtol=1e-15)
        np.testing.assert_allclose(f["p_waic_i"], p_i, rtol=1e-15)
        e = (lppd_i - const) - p_i
        np.testing.assert_allclose(f["elpd_waic_i"], e, rtol=1e-15)
        np.testing.assert_allclose([f["lppd"], f["p_waic"], f["elpd_waic"], f["waic"]],
                                   [(lppd_i - const).sum(), p_i.sum(), e.sum(), -2 * e.sum()], rtol=1e-15)
        np.testing.assert_allclose(f["se"], np.sqrt(3 * np.var(e, ddof=1)), rtol=1e-15)
    assert f["lppd_i"][2] == pytest.approx(-0.1, abs=1e-14)        # identical ll: lppd_i is that ll
    f = finish(p, None, "poisson")                                  # no y: the predictive part alone
    assert set(f) == {"n", "mean", "var"}
    assert set(finish(p)) == {"n", "mean"}
    one = p.copy()
    one[:, 0] = 1.0                                                 # n == 1: NumPy's ddof=1 variances
    f = finish(one, y, "poisson")
    assert np.isnan(f["var"]).all() and np.isnan(f["p_waic_i"]).all() and np.isnan(f["waic"])
    assert np.isfinite(f["lppd_i"]).all() and np.isfinite(finish(one, y, "bernoulli")["var"]).all()
    with pytest.raises(AssertionError):
        finish(p, y, "gamma")


# ------------------------------------------------------------------------------------------ surface
def test_hmc_samples_binding_matches_header():
    from hmc_amd import _lib as H
    src = open(os.path.join(ROOT, "include", "hmc.h")).read()
    assert int(re.search(r"HMC_PRED_STRIDE\s*=\s*(\d+)", src).group(1)) == H.PRED_STRIDE == 8
    body = re.search(r"typedef struct hmc_samples \{(.*?)\} hmc_samples;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            m = re.match(r"((?:const\s+)?\w+\s*\**)\s*(.*)", decl)
            assert m.group(1).replace(" ", "") in ("constdouble*", "int64_t")
            names += [n.strip() for n in m.group(2).split(",")]
    assert names == [f[0] for f in H.Samples._fields_]
    assert [getattr(H.Samples, f).offset for f in names] == [0, 8, 16, 24, 32, 40, 48] and ctypes.sizeof(H.Samples) == 56
    assert H.SYMBOLS["hmc_glm_predictive"] == (ctypes.c_int, [ctypes.POINTER(H.GLM), ctypes.POINTER(H.Samples), H.c_dp,
                                                             H.c_dp, ctypes.c_int64, H.c_dp])
    assert H.SYMBOLS["hmc_glm_predictive_blocks"] == (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int64, ctypes.c_int64])
    assert H.SYMBOLS["hmc_glm_predictive_workspace_size"] == (ctypes.c_int64,
                                                               [ctypes.c_int32, ctypes.c_int64, ctypes.c_int64])


def test_predictive_entry_validates_on_the_host(monkeypatch):
    """Every refusal happens before any launch: fake device pointers, no device needed."""
    from hmc_amd import _lib as H
    monkeypatch.setattr(H, "_lib", None)
    L = H.lib()
    P = 0x7000_0000
    D, n, N, Lc = 4, 12, 8, 11
    S = N * (Lc - 1)
    need = L.hmc_glm_predictive_workspace_size(D, n, S)
    assert need == L.hmc_glm_predictive_blocks(D, n, S) * n * 8 * 8 > 0

    def glm(D=D, n=n, ldx=D, X=P, y=P, family=H.HMC_GLM_POISSON):
        return H.GLM(D, n, ldx, X, y, None, family)

    def smp(q=P, n_chains=N, chain_stride=Lc * D, row_stride=D, row_begin=1, row_end=Lc, row_step=1):
        return H.Samples(q, n_chains, chain_stride, row_stride, row_begin, row_end, row_step)

    def call(g, s, out=P, ws=P, nbytes=need):
        return L.hmc_glm_predictive(g, s, out, ws, nbytes, None)
    einval = [(None, smp()), (glm(), None), (glm(X=None), smp()), (glm(), smp(q=None)),
              (glm(ldx=D - 1), smp()), (glm(), smp(row_stride=D - 1)), (glm(), smp(row_step=0)),
              (glm(), smp(row_step=-1)), (glm(), smp(row_begin=-1)), (glm(), smp(row_begin=5, row_end=4)),
              (glm(), smp(n_chains=-1)), (glm(family=2), smp()), (glm(family=-1), smp()), (glm(D=0, ldx=0), smp()),
              (glm(n=-1), smp())]
    for g, s in einval:
        assert call(g, s) == H.HMC_EINVAL, (None if g is None else (g.D, g.n, g.ldx, g.family),
                                            None if s is None else (s.row_stride, s.row_begin, s.row_end, s.row_step))
    assert call(glm(), smp(), out=None) == H.HMC_EINVAL
    assert call(glm(), smp(), ws=None) == H.HMC_EINVAL and b"workspace" in L.hmc_last_error()
    assert call(glm(), smp(), nbytes=need - 1) == H.HMC_EINVAL and b"workspace" in L.hmc_last_error()
    assert call(glm(), smp(), nbytes=0) == H.HMC_EINVAL
    with pytest.raises(AssertionError):
        H.check(call(glm(), smp(), nbytes=0), "hmc_glm_predictive")
    # limits
    assert call(glm(D=H.LOGIT_MAX_D + 1, ldx=H.LOGIT_MAX_D + 1), smp(row_stride=200), nbytes=1 << 40) == H.HMC_ENOTSUP
    assert call(glm(n=H.LOGIT_MAX_N + 1), smp(), nbytes=1 << 40) == H.HMC_ENOTSUP
    assert L.hmc_glm_predictive_workspace_size(H.LOGIT_MAX_D + 1, n, S) == 0
    assert L.hmc_glm_predictive_workspace_size(D, H.LOGIT_MAX_N + 1, S) == 0
    assert L.hmc_glm_predictive_blocks(D, n, 0) == 0 and L.hmc_glm_predictive_blocks(0, n, S) == 0
    # nothing to reduce: HMC_OK before any launch, also without a workspace; y may be NULL
    for g, s in ((glm(n=0), smp()), (glm(), smp(n_chains=0)), (glm(), smp(row_begin=4, row_end=4)),
                 (glm(y=None), smp(row_begin=Lc, row_end=Lc))):
        assert call(g, s) == H.HMC_OK and call(g, s, ws=None, nbytes=0) == H.HMC_OK


def _blocks_rule(D, n_eval, S):
    """csrc/hmc_pred.hpp::pred_sample_blocks, restated."""
    if not (1 <= D <= 128 and 1 <= n_eval <= 1 << 20 and S >= 1):
        return 0
    tiles, groups = -(-S // 16), -(-n_eval // 64)
    want = min(-(-2048 // groups), 65535)
    per = max(-(-tiles // want), 8, -(-tiles // 65535))
    return -(-tiles // per)


def test_sample_blocks_depend_on_the_shapes_only():
    from hmc_amd import _lib as H
    L = H.lib()
    shapes = [(1, 1, 1), (1, 1, 2), (17, 17, 64), (8, 20, 512), (5, 1000, 9), (32, 1024, 655360), (128, 1 << 20, 10 ** 7),
              (128, 64, 128), (128, 64, 129), (64, 65, 10 ** 9), (16, 1, 3 * 10 ** 10), (129, 5, 5), (4, 0, 5)]
    for D, n, S in shapes:
        b = L.hmc_glm_predictive_blocks(D, n, S)
        assert b == _blocks_rule(D, n, S), (D, n, S)
        assert L.hmc_glm_predictive_workspace_size(D, n, S) == b * n * 64
        assert b <= 65535 and (b == 0 or b <= -(-S // 16))
    assert L.hmc_glm_predictive_blocks(17, 17, 64) == 1 and L.hmc_glm_predictive_blocks(8, 20, 512) == 4
    assert L.hmc_glm_predictive_blocks(32, 1024, 655360) == 128


def test_sampler_methods_refuse_other_targets_and_unrun_samplers():
    from hmc_amd.samplers import HMC_sampler
    from hmc_amd.target import GLMTarget, MixtureTarget, MVNTarget
    rs = np.random.RandomState(0)
    X, y = rs.standard_normal((12, 3)), (rs.uniform(size=12) < 0.5).astype(float)
    kw = dict(Nchain=2, Niter=10, dt=0.1, sampler_type="Random", L_low=5, L_high=20, device="cpu")
    others = [HMC_sampler(3, None, None, target=MVNTarget(np.zeros(3), np.eye(3)), **kw),
              HMC_sampler(3, None, None, target=MixtureTarget(np.array([0.5, 0.5]), rs.standard_normal((2, 3)),
                                                              np.ones((2, 3))), **kw),
              HMC_sampler(3, lambda q: 0.5 * q @ q, lambda q: q, **kw)]          # probed closures: an MVN target
    for h in others:
        with pytest.raises(NotImplementedError):
            h.waic()
        with pytest.raises(NotImplementedError):
            h.posterior_predictive()
        with pytest.raises(NotImplementedError):
            h.posterior_predictive(X)
    for family, yy in (("bernoulli", y), ("poisson", np.arange(12.0))):
        for st in (dict(sampler_type="Random", L_low=5, L_high=20), dict(sampler_type="NUTS", d_max=6)):
            g = HMC_sampler(3, None, None, Nchain=2, Niter=10, dt=0.1, device="cpu",
                            target=GLMTarget(X, yy, family, np.ones(3)), **st)
            with pytest.raises(RuntimeError, match="gen_sample"):
                g.waic()
            with pytest.raises(RuntimeError, match="gen_sample"):
                g.posterior_predictive()
            with pytest.raises(RuntimeError, match="gen_sample"):
                g.posterior_predictive(X[:4])
