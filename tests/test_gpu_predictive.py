"""Posterior predictive and WAIC reductions of the GLM targets on the GPU (csrc/hmc_pred.hip behind
hmc_glm_predictive, hmc_amd.predictive, HMC_sampler.posterior_predictive / .waic).

The reference is written here, in NumPy, independently of hmc_amd.predictive: z = X @ Q.T, two-pass
mean and M2, max-shifted log-sum-exp; it runs once in float64 and once in np.longdouble.  Tolerance,
per output and row:

    |got - ref80| <= max(1e-10 |ref80|, 16 |ref64 - ref80|)

1e-10 relative is the project's bound for energies (MFMA k-order sums against BLAS);
the second term is the float64 reference's own measured distance from the 80-bit one, with a margin
of 16 for another summation order and fast_exp's 1 ulp against libm's 1/2 ulp.  Every check prints
both terms.  tests/test_predictive_host.py imports the reference from here."""
import ctypes
import functools

import numpy as np
import pytest

import glm_cases as G

SLOTS = ("n", "mu_mean", "mu_M2", "ll_mean", "ll_M2", "ll_max", "ll_sumexp", "reserved")
FAMILIES = ("poisson", "bernoulli")


# ------------------------------------------------------------------------------------------ reference
def mu_ll(z, y, family):
    """mu and ll of every (row, sample) entry in z's dtype."""
    with np.errstate(over="ignore", invalid="ignore"):
        if family == "poisson":
            mu = np.exp(z)
            ll = None if y is None else y[:, None] * z - mu
        else:
            t = np.exp(-np.abs(z))
            mu = np.where(z >= 0, 1 / (1 + t), t / (1 + t))
            ll = None if y is None else y[:, None] * z - (np.maximum(z, 0) + np.log1p(t))
    return mu, ll


def records_of(mu, ll):
    """Two-pass moments and the max-shifted log-sum-exp over axis 1: (n_eval, 8) in mu's dtype."""
    n = mu.shape[1]
    out = np.zeros((mu.shape[0], 8), dtype=mu.dtype)
    out[:, 0] = n
    with np.errstate(over="ignore", invalid="ignore"):
        def moments(x):
            mean = x.sum(axis=1) / n
            return mean, ((x - mean[:, None]) ** 2).sum(axis=1)
        out[:, 1], out[:, 2] = moments(mu)
        if ll is None:
            out[:, 3:7] = np.nan
            return out
        out[:, 3], out[:, 4] = moments(ll)
        mx = ll.max(axis=1)                                   # NaN if any NaN; -inf if all -inf
        shift = np.where(np.isneginf(mx), 0, mx)              # all -inf: exp(-inf - 0) = 0 each
        out[:, 5], out[:, 6] = mx, np.exp(ll - shift[:, None]).sum(axis=1)
    return out


def reference(X, y, Q, family, dtype):
    """Records of rows X (n_eval, D), y (n_eval,) or None against samples Q (S, D) in `dtype`."""
    X, Q = np.asarray(X, dtype=dtype), np.asarray(Q, dtype=dtype)
    y = None if y is None else np.asarray(y, dtype=dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        z = X @ Q.T
    return records_of(*mu_ll(z, y, family))


def both_references(X, y, Q, family):
    return reference(X, y, Q, family, np.float64), reference(X, y, Q, family, np.longdouble)


def check_records(got, ref64, ref80, label, slots=range(1, 7), rows=None):
    """The tolerance rule on every finite reference entry; exact agreement on inf / NaN entries."""
    sel = slice(None) if rows is None else rows
    got, ref64, ref80 = got[sel], ref64[sel], ref80[sel]
    assert np.array_equal(got[:, 0], ref80[:, 0].astype(np.float64)) and np.all(got[:, 7] == 0.0), label
    for k in slots:
        r80, r64, g = ref80[:, k], ref64[:, k], got[:, k]
        fin = np.isfinite(r80)
        assert np.array_equal(np.isnan(g[~fin]), np.isnan(r80[~fin])), (label, SLOTS[k])
        inf = ~fin & ~np.isnan(r80)
        assert np.array_equal(g[inf], r80[inf].astype(np.float64)), (label, SLOTS[k])
        if not fin.any():
            continue
        t1 = (1e-10 * np.abs(r80[fin])).astype(np.float64)
        t2 = (16 * np.abs(r64[fin] - r80[fin])).astype(np.float64)
        err = np.abs(g[fin] - r80[fin]).astype(np.float64)
        w = int(np.argmax(err - np.maximum(t1, t2)))
        print("%s %-9s worst row: err %.3g   1e-10|ref80| %.3g   16|ref64-ref80| %.3g"
              % (label, SLOTS[k], err[w], t1[w], t2[w]))
        assert np.all(err <= np.maximum(t1, t2)), (label, SLOTS[k], err[w], t1[w], t2[w])


# ------------------------------------------------------------------------------------------ inputs
def draw_case(family, D, n_eval, N, L, seed=0, spread=0.5):
    """X, y and an [N][L][D] sample set around one coefficient vector, z moderate at every D."""
    rs = np.random.RandomState(1000 * D + n_eval + seed)
    if family == "poisson":
        X = 0.3 * rs.standard_normal((n_eval, D))
        beta = 2.0 * rs.standard_normal(D) / np.sqrt(D)
        y = rs.poisson(np.exp(X @ beta)).astype(float)
    else:
        X = rs.standard_normal((n_eval, D))
        beta = rs.standard_normal(D)
        y = (rs.random_sample(n_eval) < 1 / (1 + np.exp(-X @ beta))).astype(float)
    Q = beta + spread * rs.standard_normal((N, L, D)) / np.sqrt(D)
    return X, y, Q


def run(X, y, family, samples, rows=slice(1, None)):
    from hmc_amd.predictive import glm_predictive_partials
    return glm_predictive_partials(X, y, family, samples, rows=rows, device="cuda:0")


def blocks(D, n_eval, S):
    from hmc_amd import _lib as H
    return H.lib().hmc_glm_predictive_blocks(D, n_eval, S)


# ------------------------------------------------------------------------------------------ 1
PARITY_SHAPES = [(1, 1, 1, 3), (2, 20, 17, 3), (17, 17, 16, 5), (64, 40, 4, 7), (65, 33, 18, 4), (128, 100, 3, 6),
                 (5, 1000, 3, 4), (8, 20, 64, 9), (1, 1, 1, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", PARITY_SHAPES, ids=lambda s: "D%d_n%d_N%d_L%d" % s)
@pytest.mark.parametrize("family", FAMILIES)
def test_parity(family, shape):
    D, n_eval, N, L = shape
    X, y, Q = draw_case(family, D, n_eval, N, L)
    S = N * (L - 1)
    if shape == (8, 20, 64, 9):
        assert blocks(D, n_eval, S) >= 2                 # several sample blocks: the merge kernel's loop
    if shape == (17, 17, 16, 5):
        assert blocks(D, n_eval, S) == 1
    got = run(X, y, family, Q)
    r64, r80 = both_references(X, y, Q[:, 1:].reshape(-1, D), family)
    check_records(got, r64, r80, "%s %s" % (family, shape))
    if S == 1:                                           # a single sample: M2 == 0, variances NaN
        from hmc_amd.predictive import finish
        assert got[0, 0] == 1.0 and got[0, 2] == 0.0 and got[0, 4] == 0.0 and got[0, 6] == 1.0
        f = finish(got, y, family)
        assert np.isnan(f["p_waic_i"]).all() and np.isnan(f["elpd_waic"]) and np.isnan(f["se"])
        if family == "poisson":
            assert np.isnan(f["var"]).all()


# ------------------------------------------------------------------------------------------ 2
def concentrated_case(family):
    """D = 37, n_eval = 33, S = 1035 samples within 3e-3 of one coefficient vector: the spread of mu
    and ll is a small fraction of their size, so sum x^2 - (sum x)^2 / n cancels.  Everything from
    RandomState(3), in the order X, beta, y, Q.  poisson: X[:, 0] = 1 and beta[0] = 6 (counts ~ e^6)."""
    D, n_eval, N, L = 37, 33, 45, 24
    rs = np.random.RandomState(3)
    if family == "poisson":
        X = 0.3 * rs.standard_normal((n_eval, D))
        X[:, 0] = 1.0
        beta = 2.0 * rs.standard_normal(D) / np.sqrt(D)
        beta[0] = 6.0
        y = rs.poisson(np.exp(X @ beta)).astype(float)
    else:
        X = rs.standard_normal((n_eval, D))
        beta = rs.standard_normal(D)
        y = (rs.random_sample(n_eval) < 1 / (1 + np.exp(-X @ beta))).astype(float)
    Q = beta + 3e-3 * rs.standard_normal((N, L, D))
    return X, y, Q


def naive_M2(X, y, Q, family):
    """sum x^2 - (sum x)^2 / n in float64: (mu_M2, ll_M2)."""
    mu, ll = mu_ll(X @ Q.T, y, family)
    n = mu.shape[1]
    return tuple((x * x).sum(axis=1) - x.sum(axis=1) ** 2 / n for x in (mu, ll))


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_concentrated_samples(family):
    X, y, Q = concentrated_case(family)
    Qs = Q[:, 1:].reshape(-1, Q.shape[2])
    assert Qs.shape[0] == 1035
    r64, r80 = both_references(X, y, Qs, family)
    # conditions on the inputs, from the references alone
    rel = np.abs(r64[:, 1:7] - r80[:, 1:7]) / np.abs(r80[:, 1:7])
    print("float64 two-pass reference vs 80-bit: max rel %.3g" % rel.max())
    assert rel.max() <= 1e-10
    nm, nl = naive_M2(X, y, Qs, family)
    off = max(float((np.abs(nm - r80[:, 2]) / r80[:, 2]).max()), float((np.abs(nl - r80[:, 4]) / r80[:, 4]).max()))
    print("naive sum x^2 - (sum x)^2 / n vs 80-bit: max rel %.3g" % off)
    assert off > 1e-7
    got = run(X, y, family, Q)
    check_records(got, r64, r80, "concentrated %s" % family)


# ------------------------------------------------------------------------------------------ 3
@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_views_match_contiguous_copies_bit_for_bit(family):
    import torch
    D, n_eval, N, L = 13, 21, 19, 12
    X, y, Q = draw_case(family, D, n_eval, N, L)
    big = torch.full((N + 2, L + 3, D + 5), float("nan"), dtype=torch.float64, device="cuda:0")
    big[1:N + 1, 2:L + 2, 3:D + 3] = torch.as_tensor(Q, device="cuda:0")
    view = big[1:N + 1, 2:L + 2, 3:D + 3]
    assert view.stride(0) > L * D and view.stride(1) > D and not view.is_contiguous()
    copy = view.contiguous()
    for rows in (slice(1, None), slice(1, None, 2), slice(3, None), slice(2, 9, 3)):
        a, b = run(X, y, family, view, rows=rows), run(X, y, family, copy, rows=rows)
        assert a.tobytes() == b.tobytes(), rows
        assert a.tobytes() == run(X, y, family, view, rows=rows).tobytes(), rows      # and run to run
        r64, r80 = both_references(X, y, Q[:, rows].reshape(-1, D), family)
        check_records(a, r64, r80, "view %s %s" % (family, rows))
    # a host array takes the same path
    assert run(X, y, family, Q).tobytes() == run(X, y, family, copy).tobytes()


# ------------------------------------------------------------------------------------------ 4
@pytest.mark.gpu
def test_non_finite_rows_follow_numpy_and_stay_in_their_row():
    D, n_eval, N, L, j = 5, 20, 7, 9, 7
    X, y, Q = draw_case("poisson", D, n_eval, N, L)
    rs = np.random.RandomState(4)
    Q[:, :, 0] = 1.0 + 0.2 * rs.standard_normal((N, L))          # 800 q_0 straddles exp's overflow at 709.78
    benign = run(X, y, "poisson", Q)
    Xo = X.copy()
    Xo[j] = 0.0
    Xo[j, 0] = 800.0
    got = run(Xo, y, "poisson", Q)
    Qs = Q[:, 1:].reshape(-1, D)
    z = 800.0 * Qs[:, 0]
    assert (z > 710).any() and (z < 709).any()
    others = np.arange(n_eval) != j
    assert got[others].tobytes() == benign[others].tobytes()
    r = got[j]
    assert r[0] == len(Qs) and r[1] == np.inf and np.isnan(r[2]) and r[3] == -np.inf and np.isnan(r[4]) and r[7] == 0
    with np.errstate(over="ignore"):
        ll = y[j] * z - np.exp(z)                                # float64: -inf where exp overflows
    fin = np.isfinite(ll)
    mx = ll[fin].max()
    se = np.exp(ll[fin] - mx).sum()
    print("overflow row: ll_max %.17g (ref %.17g)  ll_sumexp %.17g (ref %.17g)" % (r[5], mx, r[6], se))
    assert abs(r[5] - mx) <= 1e-10 * abs(mx) and abs(r[6] - se) <= 1e-10 * se
    # every ll -inf: max = -inf, sumexp = 0
    Qi = Q.copy()
    Qi[:, :, 0] = 1.0 + 0.01 * rs.standard_normal((N, L))
    r = run(Xo, y, "poisson", Qi)[j]
    assert r[1] == np.inf and r[3] == -np.inf and r[5] == -np.inf and r[6] == 0.0
    # a NaN in the row: every slot but 0 and 7 is NaN, in that row alone
    for family in FAMILIES:
        Xf, yf, Qf = draw_case(family, D, n_eval, N, L)
        base = run(Xf, yf, family, Qf)
        Xn = Xf.copy()
        Xn[j, 0] = np.nan
        got = run(Xn, yf, family, Qf)
        assert got[others].tobytes() == base[others].tobytes()
        assert got[j, 0] == N * (L - 1) and got[j, 7] == 0.0 and np.isnan(got[j, 1:7]).all()


# ------------------------------------------------------------------------------------------ 5
@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_without_y(family):
    X, y, Q = draw_case(family, 33, 37, 6, 8)
    with_y, without = run(X, y, family, Q), run(X, None, family, Q)
    assert np.isnan(without[:, 3:7]).all()
    assert without[:, :3].tobytes() == with_y[:, :3].tobytes() and np.all(without[:, 7] == 0.0)


# ------------------------------------------------------------------------------------------ 6
@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_merge_of_two_shards(family):
    from hmc_amd.predictive import merge_partials
    D, n_eval, N, L = 19, 35, 40, 6
    X, y, Q = draw_case(family, D, n_eval, N, L)
    merged = merge_partials(run(X, y, family, Q[:24]), run(X, y, family, Q[24:]))
    r64, r80 = both_references(X, y, Q[:, 1:].reshape(-1, D), family)
    check_records(merged, r64, r80, "merged %s" % family)
    check_records(run(X, y, family, Q), r64, r80, "whole %s" % family)


# ------------------------------------------------------------------------------------------ 7
@pytest.mark.gpu
def test_undersized_workspace_is_refused_before_any_launch():
    import torch
    from hmc_amd import _lib as H
    L_ = H.lib()
    D, n_eval, N, L = 8, 20, 64, 9
    X, y, Q = draw_case("poisson", D, n_eval, N, L)
    dev = "cuda:0"
    Xd, yd, Qd = (torch.as_tensor(a, device=dev) for a in (X, y, Q))
    S = N * (L - 1)
    need = L_.hmc_glm_predictive_workspace_size(D, n_eval, S)
    assert need == L_.hmc_glm_predictive_blocks(D, n_eval, S) * n_eval * 64
    ws = torch.zeros(need // 8, dtype=torch.float64, device=dev)
    out = torch.full((n_eval, 8), -7.0, dtype=torch.float64, device=dev)
    glm = H.GLM(D, n_eval, D, H.ptr(Xd), H.ptr(yd), None, H.HMC_GLM_POISSON)
    sm = H.Samples(H.ptr(Qd), N, L * D, D, 1, L, 1)
    stream = torch.cuda.current_stream().cuda_stream
    for short in (need - 1, 0):
        assert L_.hmc_glm_predictive(ctypes.byref(glm), ctypes.byref(sm), H.ptr(out), H.ptr(ws), short,
                                     stream) == H.HMC_EINVAL
        assert b"workspace" in L_.hmc_last_error()
    assert L_.hmc_glm_predictive(ctypes.byref(glm), ctypes.byref(sm), H.ptr(out), None, need, stream) == H.HMC_EINVAL
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((ws == 0.0).all())
    assert L_.hmc_glm_predictive(ctypes.byref(glm), ctypes.byref(sm), H.ptr(out), H.ptr(ws), need, stream) == H.HMC_OK
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == run(X, y, "poisson", Q).tobytes()


# ------------------------------------------------------------------------------------------ 8
@functools.lru_cache(maxsize=None)
def nuts_run(family):
    from hmc_amd.samplers import HMC_sampler
    pvs, cdt, seed = {"poisson": (0.2, 0.8, 5), "bernoulli": (0.2, 1.2, 3)}[family]   # test_gpu_glm_nuts.py: D17
    c = G.recipe(family, 17, 17, 16, cdt, seed, pvs=pvs)
    h = HMC_sampler(17, None, None, Nchain=16, Niter=10, sampler_type="NUTS", dt=c["dt"], d_max=8,
                    target=G.glm_target(c), rng="philox", seed=5)
    h.gen_sample(c["q_start"], verbose=False)
    return c, h


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_sampler_methods_end_to_end(family):
    from scipy.special import gammaln
    c, h = nuts_run(family)
    X, y, D = c["X"], c["y"], c["D"]
    Qs = h.q_chain[:, 1:].reshape(-1, D)
    assert Qs.shape[0] == 16 * 10
    r64, r80 = both_references(X, y, Qs, family)
    n = float(len(Qs))

    def bound(a64, a80):
        return np.maximum(1e-10 * np.abs(a80), 16 * np.abs(a64 - a80)).astype(np.float64)

    def pred_var(r):
        return r[:, 1] * (1 - r[:, 1]) if family == "bernoulli" else r[:, 1] + r[:, 2] / (n - 1)
    pp = h.posterior_predictive()
    assert np.all(pp["n"] == n)
    assert np.all(np.abs(pp["mean"] - r80[:, 1]) <= bound(r64[:, 1], r80[:, 1]))
    assert np.all(np.abs(pp["var"] - pred_var(r80)) <= bound(pred_var(r64), pred_var(r80)))
    X_new = np.random.RandomState(8).standard_normal((23, D)) * (0.3 if family == "poisson" else 1.0)
    n64, n80 = both_references(X_new, None, Qs, family)
    pn = h.posterior_predictive(X_new)
    assert pn["mean"].shape == (23,) and "lppd" not in pn
    assert np.all(np.abs(pn["mean"] - n80[:, 1]) <= bound(n64[:, 1], n80[:, 1]))
    assert np.all(np.abs(pn["var"] - pred_var(n80)) <= bound(pred_var(n64), pred_var(n80)))

    def waic_terms(r):
        const = gammaln(y + 1).astype(r.dtype) if family == "poisson" else 0
        lppd_i = r[:, 5] + np.log(r[:, 6]) - np.log(r[:, 0]) - const
        p_i = r[:, 4] / (r[:, 0] - 1)
        return lppd_i, p_i, lppd_i - p_i
    w = h.waic()
    t64, t80 = waic_terms(r64), waic_terms(r80)
    for name, a64, a80 in zip(("lppd_i", "p_waic_i", "elpd_waic_i"), t64, t80):
        err = np.abs(w[name] - a80).astype(np.float64)
        print("%s %-11s max err %.3g  bound there %.3g" % (family, name, err.max(), bound(a64, a80)[np.argmax(err)]))
        assert np.all(err <= bound(a64, a80)), name
    # the sums: every lppd_i is a log probability (<= 0) and every p_waic_i a variance (>= 0), so a
    # sum of terms each within 1e-10 of its own size is within 1e-10 of the sum's size; 1e-9 leaves
    # room for the rows bounded by the reference's own error.  se divides by the spread of elpd_i,
    # which is of the order of elpd_i itself here: 1e-8.
    elpd80 = t80[2].astype(np.float64)
    np.testing.assert_allclose([w["lppd"], w["p_waic"], w["elpd_waic"], w["waic"]],
                               [float(t80[0].sum()), float(t80[1].sum()), elpd80.sum(), -2 * elpd80.sum()], rtol=1e-9)
    np.testing.assert_allclose(w["se"], np.sqrt(len(y) * np.var(elpd80, ddof=1)), rtol=1e-8)
