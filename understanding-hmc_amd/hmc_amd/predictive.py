"""Posterior predictive summaries and WAIC of a GLM target, reduced on the device.

For evaluation rows X (n_eval, D) and stored samples q_s, z[j][s] = x_j . q_s is never stored:
`glm_predictive_partials` (hmc_glm_predictive, csrc/hmc_pred.hip) reads the samples once, where they
are, and returns one mergeable record per evaluation row (include/hmc.h: HMC_PRED_STRIDE slots):

    0 n   1 mu_mean   2 mu_M2   3 ll_mean   4 ll_M2   5 ll_max   6 ll_sumexp   7 reserved (0)

    bernoulli  mu = sigma(z),  ll = y z - softplus(z)
    poisson    mu = exp(z),    ll = y z - exp(z)      (-lgamma(y + 1) is added by `finish`)

`merge_partials` combines the records of disjoint sample sets (the ranks of a sharded run) by the
rule of csrc/hmc_pred.hpp, and `finish` turns records into the predictive mean and variance and, with
y, into lppd, p_waic and WAIC (Gelman, Hwang & Vehtari 2014)."""
import ctypes
from math import lgamma

import numpy as np

from . import _lib as H
from .views import SamplesView

FAMILIES = {"bernoulli": H.HMC_GLM_BERNOULLI, "poisson": H.HMC_GLM_POISSON}


def _family_id(family):
    if family in FAMILIES:
        return FAMILIES[family]
    if family in FAMILIES.values():
        return int(family)
    raise AssertionError("family must be one of %s" % sorted(FAMILIES))


def glm_predictive_partials(X, y, family, samples, rows=slice(1, None), device=None):
    """Partial records (n_eval, 8) of the evaluation set (X, y) over samples[:, rows, :].

    X (n_eval, D) and y (n_eval,) or None: NumPy arrays or torch tensors.  samples: an [N][L][D]
    torch tensor or NumPy array; a device tensor is read in place, a non-contiguous view by its
    strides (the last dimension must be contiguous), never copied.  rows: a slice with a positive
    step, the rows of every chain to use; the default drops the start row as
    compute_convergence_stats does.  device: where a host `samples` goes (default: X's device if it is
    a device tensor, else the current device)."""
    import torch
    fam = _family_id(family)
    if device is None and not getattr(samples, "is_cuda", False) and isinstance(X, torch.Tensor) and X.is_cuda:
        device = X.device                          # host samples go where X is
    view = SamplesView(samples, rows, device)
    device, D, S = view.device, view.D, view.M

    def up(a):
        if isinstance(a, torch.Tensor):
            return a.to(device=device, dtype=torch.float64).contiguous()
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(device)
    Xd = up(X)
    if Xd.dim() != 2 or Xd.shape[1] != D:
        raise AssertionError("X must be (n_eval, D) with the samples' D")
    n_eval = Xd.shape[0]
    yd = None
    if y is not None:
        yd = up(y)
        if yd.shape != (n_eval,):
            raise AssertionError("y must be (n_eval,)")
    L_ = H.lib()
    out = torch.zeros((n_eval, H.PRED_STRIDE), dtype=torch.float64, device=device)
    if n_eval == 0 or S == 0:
        return out.cpu().numpy()
    nbytes = L_.hmc_glm_predictive_workspace_size(D, n_eval, S)
    if nbytes <= 0:
        raise NotImplementedError("hmc_glm_predictive: D=%d (<= %d), n_eval=%d (<= %d) unsupported"
                                  % (D, H.LOGIT_MAX_D, n_eval, H.LOGIT_MAX_N))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
    G = H.GLM(D, n_eval, Xd.stride(0) if n_eval > 1 else D, H.ptr(Xd), H.ptr(yd), None, fam)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        H.check(L_.hmc_glm_predictive(ctypes.byref(G), ctypes.byref(view.c), H.ptr(out), H.ptr(ws), nbytes, stream),
                "hmc_glm_predictive")
        return out.cpu().numpy()


def _merge_moments(na, mean_a, M2_a, nb, mean_b, M2_b):
    n = na + nb
    with np.errstate(invalid="ignore", over="ignore"):
        delta = mean_b - mean_a
        ok = np.isfinite(delta)
        d = np.where(ok, delta, 0.0)
        mean = np.where(ok, mean_a + d * (nb / n), mean_a + mean_b)
        M2 = np.where(ok, (M2_a + M2_b) + (d * d) * (na * nb / n), np.nan)
    return mean, M2


def merge_partials(a, b):
    """Records of the union of two disjoint sample sets: the rule of csrc/hmc_pred.hpp (pred_merge).
    Chan's update for (n, mean, M2); a difference of means that is not finite gives the sum of the
    means and M2 = NaN, as NumPy's two-pass result on the concatenated data.  (max, sumexp): the side
    holding the maximum keeps its sum, the other is rescaled; NaN on either side gives NaN.  A record
    with n == 0 is the identity."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape and a.shape[-1] == H.PRED_STRIDE
    na, nb = a[..., 0], b[..., 0]
    out = np.zeros_like(a)
    out[..., 0] = na + nb
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        safe_na, safe_nb = np.where(na == 0, 1.0, na), np.where(nb == 0, 1.0, nb)
        for m_, v_ in ((1, 2), (3, 4)):
            out[..., m_], out[..., v_] = _merge_moments(safe_na, a[..., m_], a[..., v_], safe_nb, b[..., m_], b[..., v_])
        ma, sa, mb, sb = a[..., 5], a[..., 6], b[..., 5], b[..., 6]
        bad = np.isnan(ma) | np.isnan(mb) | np.isnan(sa) | np.isnan(sb)
        m = np.where(ma > mb, ma, mb)
        ta = np.where(ma == m, sa, sa * np.exp(ma - m))
        tb = np.where(mb == m, sb, sb * np.exp(mb - m))
        out[..., 5] = np.where(bad, np.nan, m)
        out[..., 6] = np.where(bad, np.nan, ta + tb)
    out[nb == 0] = a[nb == 0]
    out[(na == 0) & (nb != 0)] = b[(na == 0) & (nb != 0)]
    out[..., 7] = 0.0
    return out


def finish(partials, y=None, family=None):
    """Predictive summaries from records (n_eval, 8).  Always: n, mean (= mu_mean) and, with a
    family, var of a new observation: mean (1 - mean) (bernoulli), mean + mu_M2 / (n - 1) (poisson:
    the expected Poisson variance plus the posterior variance of the rate).  With y, per row:
    lppd_i = ll_max + log(ll_sumexp) - log n (poisson: - lgamma(y + 1)), p_waic_i = ll_M2 / (n - 1),
    elpd_waic_i = lppd_i - p_waic_i; their sums lppd, p_waic, elpd_waic; waic = -2 elpd_waic and
    se = sqrt(n_eval var(elpd_waic_i)) (ddof = 1).  n == 1: the variances are NaN, as NumPy's ddof=1."""
    p = np.asarray(partials, dtype=np.float64)
    assert p.ndim == 2 and p.shape[1] == H.PRED_STRIDE
    fam = None if family is None else _family_id(family)
    n = p[:, 0]
    out = {"n": n, "mean": p[:, 1].copy()}
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        var_mu = np.where(n > 1, p[:, 2] / np.where(n > 1, n - 1, 1.0), np.nan)
        if fam == H.HMC_GLM_BERNOULLI:
            out["var"] = out["mean"] * (1.0 - out["mean"])
        elif fam == H.HMC_GLM_POISSON:
            out["var"] = out["mean"] + var_mu
        if y is None:
            return out
        y = np.asarray(y, dtype=np.float64)
        assert y.shape == n.shape
        lppd_i = p[:, 5] + np.log(p[:, 6]) - np.log(n)
        if fam == H.HMC_GLM_POISSON:
            lppd_i = lppd_i - np.array([lgamma(v + 1.0) for v in y])
        p_waic_i = np.where(n > 1, p[:, 4] / np.where(n > 1, n - 1, 1.0), np.nan)
        elpd_i = lppd_i - p_waic_i
        out.update(lppd_i=lppd_i, p_waic_i=p_waic_i, elpd_waic_i=elpd_i, lppd=lppd_i.sum(), p_waic=p_waic_i.sum(),
                   elpd_waic=elpd_i.sum(), waic=-2.0 * elpd_i.sum(),
                   se=float(np.sqrt(len(elpd_i) * np.var(elpd_i, ddof=1))) if len(elpd_i) > 1 else float("nan"))
    return out
