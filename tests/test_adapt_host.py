"""Step-size adaptation, the parts that need no GPU.

(a) The update rule as the ADAPT kernels compile it (csrc/hmc_adapt.hpp, printed by the host program
    adapt_host that make builds next to libhmc.so) against the NumPy restatement
    tests/adapt_model.py::DualAverage, rtol 1e-12, both clamps included.
(b) The surface: adapt_step / step_scale0 with any target but a GLMTarget raise NotImplementedError in
    the constructor; hmc_adapt and the new prototypes of hmc_amd/_lib.py match include/hmc.h; the
    _adapt entries validate their own argument on the host."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import adapt_model as A
from conftest import ROOT


def _host(delta, s0, adapt_end, alphas):
    from hmc_amd import _lib
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), "adapt_host")
    assert os.path.exists(exe), f"{exe} not found: build it with make -C understanding-hmc_amd/csrc"
    args = [exe, repr(float(delta)), repr(float(s0)), str(adapt_end)] + [repr(float(a)) for a in alphas]
    out = subprocess.run(args, check=True, capture_output=True, text=True).stdout
    rows = np.array([[float(x) for x in line.split()] for line in out.splitlines()])
    assert rows.shape == (len(alphas), 9)
    return rows


def _model(delta, s0, adapt_end, alphas):
    da, rows = A.DualAverage(s0, delta), []
    for i, a in enumerate(alphas, start=1):
        da.end_iteration(a, i < adapt_end)
        rows.append(np.append(da.slots(), da.scale(i + 1 < adapt_end)))
    return np.array(rows), da.clamped


SEQUENCES = {
    "alpha0": (0.8, 1.0, np.zeros(200)),
    "alpha1": (0.8, 1.0, np.ones(200)),
    # seeded sequences whose mean is delta, so that log_s wanders inside the clamps
    "random": (0.65, 0.37, np.random.RandomState(11).uniform(0.3, 1.0, 150)),
    "random_low_delta": (0.2, 3.0, np.random.RandomState(12).beta(0.5, 2.0, 150)),
}


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_update_rule_matches_numpy(name):
    delta, s0, alphas = SEQUENCES[name]
    ref, clamped = _model(delta, s0, len(alphas) + 1, alphas)
    got = _host(delta, s0, len(alphas) + 1, alphas)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)
    lo, hi = np.log(s0) - A.CLAMP, np.log(s0) + A.CLAMP
    if name == "alpha0":        # delta - alpha > 0 throughout: the step shrinks into the lower clamp
        assert clamped and got[-1, 0] == lo and np.all(np.diff(got[:, 0]) <= 0)
    elif name == "alpha1":
        assert clamped and got[-1, 0] == hi and np.all(np.diff(got[:, 0]) >= 0)
    else:
        assert not clamped
    assert np.all(got[:, 0] >= lo) and np.all(got[:, 0] <= hi)
    # the first update moves s by at most e^(20 max(delta, 1 - delta) / 11) either way (include/hmc.h):
    # up by e^(20 * 0.2 / 11) ~ 1.44 after a perfect acceptance, down by e^(20 * 0.8 / 11) ~ 4.3 after none
    if name == "alpha1":
        np.testing.assert_allclose(got[0, 8] / s0, np.exp(20 * 0.2 / 11), rtol=1e-12)
    if name == "alpha0":
        np.testing.assert_allclose(s0 / got[0, 8], np.exp(20 * 0.8 / 11), rtol=1e-12)


def test_iterations_after_adapt_end_only_count():
    """adapt_end = 6: iterations 1..5 adapt, the rest add to slots 6 and 7 and run at exp(log_s_bar);
    adapt_end = 0 or 1: nothing adapts and the multiplier stays exp(log(s0))."""
    alphas = np.random.RandomState(3).uniform(0, 1, 12)
    got, (ref, _) = _host(0.8, 0.5, 6, alphas), _model(0.8, 0.5, 6, alphas)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)
    assert got[-1, 3] == 5 and got[-1, 7] == 7
    assert np.all(got[4:, :5] == got[4, :5])                       # slots 0-4 frozen from iteration 5 on
    np.testing.assert_allclose(got[4:, 8], np.exp(got[4, 1]), rtol=1e-15)
    np.testing.assert_allclose(got[-1, 6], alphas[5:].sum(), rtol=1e-14)
    for end in (0, 1):
        g = _host(0.8, 0.5, end, alphas)
        assert np.all(g[:, 3] == 0) and np.all(g[:, 8] == np.exp(np.log(0.5)))
    assert np.all(_host(0.8, 1.0, 0, alphas)[:, 8] == 1.0)          # s0 = 1: exactly 1


# ------------------------------------------------------------------------------------------ surface
def test_adapt_step_needs_a_glm_target():
    from hmc_amd.samplers import HMC_sampler
    from hmc_amd.target import GLMTarget, LogisticTarget, MixtureTarget, MVNTarget
    rs = np.random.RandomState(0)
    X, y = rs.standard_normal((12, 3)), (rs.uniform(size=12) < 0.5).astype(float)
    others = [MVNTarget(np.zeros(3), np.eye(3)),
              MixtureTarget(np.array([0.5, 0.5]), rs.standard_normal((2, 3)), np.ones((2, 3))),
              LogisticTarget(X, y, np.ones(3))]
    kw = dict(Nchain=2, Niter=10, warm_up_num=4, dt=0.1, sampler_type="Random", L_low=5, L_high=20, device="cpu")
    for t in others:
        HMC_sampler(3, None, None, target=t, **kw)                   # constructs without adaptation
        with pytest.raises(NotImplementedError):
            HMC_sampler(3, None, None, target=t, adapt_step=True, **kw)
        with pytest.raises(NotImplementedError):
            HMC_sampler(3, None, None, target=t, step_scale0=0.5, **kw)
    with pytest.raises(NotImplementedError):                          # probed closures: an MVN target
        HMC_sampler(3, lambda q: 0.5 * q @ q, lambda q: q, adapt_step=True, **kw)
    for st in (dict(sampler_type="Random", L_low=5, L_high=20), dict(sampler_type="NUTS", d_max=6)):
        g = HMC_sampler(3, None, None, Nchain=2, Niter=10, warm_up_num=4, dt=0.1, device="cpu",
                        target=GLMTarget(X, y, "bernoulli", np.ones(3)), adapt_step=True, adapt_delta=0.7, **st)
        assert g.step_scale is None and g.accept_stat is None and g.accept_stat_warm_up is None
        with pytest.raises(AssertionError):
            HMC_sampler(3, None, None, Nchain=2, Niter=10, dt=0.1, device="cpu",
                        target=GLMTarget(X, y, "bernoulli", np.ones(3)), adapt_step=True, adapt_delta=1.0, **st)


def _c_struct_fields(name):
    src = open(os.path.join(ROOT, "include", "hmc.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"((?:const\s+)?\w+\s*\**)\s*(.*)", decl)
        ctype = m.group(1).replace(" ", "")
        fields += [(n.strip(), ctype) for n in m.group(2).split(",")]
    return fields


def test_hmc_adapt_binding_matches_header():
    from hmc_amd import _lib as H
    src = open(os.path.join(ROOT, "include", "hmc.h")).read()
    assert int(re.search(r"HMC_ADAPT_STRIDE\s*=\s*(\d+)", src).group(1)) == H.ADAPT_STRIDE == len(A.SLOTS)
    size = {"double*": 8, "int32_t": 4, "double": 8}
    fields = _c_struct_fields("hmc_adapt")
    assert [f[0] for f in fields] == [f[0] for f in H.Adapt._fields_]
    for (name, ctype), (_, pytype) in zip(fields, H.Adapt._fields_):
        assert ctypes.sizeof(pytype) == size[ctype], name
    assert [getattr(H.Adapt, f[0]).offset for f in fields] == [0, 8, 16, 24, 32, 40] and ctypes.sizeof(H.Adapt) == 48
    # prototypes: the plain entry's arguments with POINTER(Adapt) before the stream
    for plain, adapt in (("hmc_glm_random_iters", "hmc_glm_random_iters_adapt"),
                         ("hmc_glm_nuts_iters", "hmc_glm_nuts_iters_adapt")):
        (r0, a0), (r1, a1) = H.SYMBOLS[plain], H.SYMBOLS[adapt]
        assert r0 is r1 and a1 == a0[:-1] + [ctypes.POINTER(H.Adapt)] + a0[-1:]
        decl = re.search(r"hmc_status %s\((.*?)\);" % adapt, re.sub(r"/\*.*?\*/", "", src, flags=re.S), re.S).group(1)
        params = [p.strip() for p in decl.split(",")]
        assert len(params) == len(a1) and params[-2] == "const hmc_adapt* ad" and params[-1] == "void* stream"
    decl = re.search(r"hmc_status hmc_adapt_init\((.*?)\);", re.sub(r"/\*.*?\*/", "", src, flags=re.S), re.S).group(1)
    assert [p.split()[0] for p in decl.split(",")] == ["double*", "int64_t", "const", "void*"]
    assert H.SYMBOLS["hmc_adapt_init"] == (ctypes.c_int, [H.c_dp, ctypes.c_int64, H.c_dp, H.c_dp])


def test_adapt_entries_validate_on_the_host(monkeypatch):
    """HMC_EINVAL for a null block or state, delta outside (0, 1), non-positive gamma / t0 / kappa;
    what the plain entry refuses is refused as it refuses it.  Fake device pointers: nothing launches."""
    from hmc_amd import _lib as H
    monkeypatch.setattr(H, "_lib", None)
    L = H.lib()
    P = 0x7000_0000
    D, n, N = 4, 12, 8
    glm = H.GLM(D, n, D, P, P, P, H.HMC_GLM_POISSON)
    K = H.Kinetic(None, None, None, 0.1, None, None, None)
    S = H.Schedule(N, 0, 10, 0, 1, 11, 5, 20, 1, 11, H.HMC_RNG_PHILOX, H.HMC_MODE_FAST, 5, 0, 0)
    st = H.State(P, P)
    ws = L.hmc_glm_nuts_workspace_size(D, N, 5)

    def calls(ad):
        return (L.hmc_glm_random_iters_adapt(glm, K, S, None, st, ad, None),
                L.hmc_glm_nuts_iters_adapt(glm, K, S, None, st, P, ws, ad, None))
    bad = [None, H.Adapt(None, 4, 0.8, 0.05, 10.0, 0.75)]
    bad += [H.Adapt(P, 4, d, 0.05, 10.0, 0.75) for d in (0.0, 1.0, -0.1, 1.5, float("nan"))]
    bad += [H.Adapt(P, 4, 0.8, *g) for g in ((0.0, 10.0, 0.75), (0.05, -1.0, 0.75), (0.05, 10.0, 0.0),
                                             (float("nan"), 10.0, 0.75))]
    for ad in bad:
        assert calls(ad) == (H.HMC_EINVAL, H.HMC_EINVAL), None if ad is None else (ad.state, ad.delta, ad.gamma)
    ok = H.Adapt(P, 4, 0.8, 0.05, 10.0, 0.75)
    wide = H.GLM(129, n, 129, P, P, P, H.HMC_GLM_POISSON)
    assert L.hmc_glm_random_iters_adapt(wide, K, S, None, st, ok, None) == H.HMC_ENOTSUP
    assert L.hmc_glm_nuts_iters_adapt(wide, K, S, None, st, P, 1 << 40, ok, None) == H.HMC_ENOTSUP
    full = H.Kinetic(None, None, None, 0.1, P, None, None)
    assert L.hmc_glm_random_iters_adapt(glm, full, S, None, st, ok, None) == H.HMC_ENOTSUP
    assert L.hmc_glm_nuts_iters_adapt(glm, K, S, None, st, P, ws - 1, ok, None) == H.HMC_EINVAL
    assert b"workspace" in L.hmc_last_error()
    S31 = H.Schedule(N, 0, 10, 0, 1, 11, 5, 20, 1, 11, H.HMC_RNG_PHILOX, H.HMC_MODE_FAST, 31, 0, 0)
    assert L.hmc_glm_nuts_iters_adapt(glm, K, S31, None, st, P, 1 << 40, ok, None) == H.HMC_ENOTSUP
    # an empty range or an empty batch returns HMC_OK before any launch
    S0 = H.Schedule(N, 0, 10, 0, 1, 11, 5, 20, 3, 3, H.HMC_RNG_PHILOX, H.HMC_MODE_FAST, 5, 0, 0)
    assert L.hmc_glm_random_iters_adapt(glm, K, S0, None, st, ok, None) == H.HMC_OK
    assert L.hmc_glm_nuts_iters_adapt(glm, K, S0, None, st, P, ws, ok, None) == H.HMC_OK
    assert L.hmc_adapt_init(None, 4, None, None) == H.HMC_EINVAL and L.hmc_adapt_init(None, 0, None, None) == H.HMC_OK
