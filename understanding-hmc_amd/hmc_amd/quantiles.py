"""Posterior quantiles on the device: exact order statistics by radix select.

`order_stats` (hmc_order_stats / hmc_select_*, csrc/hmc_select.hip) returns, for every dimension of
samples[:, rows, :], the k-th smallest of its M = chains x rows values, bit for bit what
np.sort(x[:, d])[k] gives (a zero may come back with either sign; NaNs sort last).  The samples are
read where they are, by their strides, 8 times (8 bits of the key per pass); nothing is copied or
sorted.  `quantiles` interpolates NumPy's method="linear" on the host from two order statistics per
probability, and `credible_interval` is the pair of quantiles around the centre.

Only integer counts are added on the device, so the result depends on the multiset of values of
each dimension alone.  With `group`, every rank passes its own chains: the count tables are
all-reduced between the count and the pick step of each pass, and every rank returns the order
statistics of the union."""
import ctypes

import numpy as np

from . import _lib as H
from .views import SamplesView as _View


def _allreduce(x, group):
    from .diagnostics import _allreduce as reduce
    return reduce(x, group)


def _order_stats(view, ranks, M, group):
    """(len(ranks), D) order statistics of the view (this rank's shard of M samples in all)."""
    import torch
    D, dev = view.D, view.device
    L_ = H.lib()
    out = np.empty((len(ranks), D), dtype=np.float64)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        for b in range(0, len(ranks), H.SELECT_MAX_RANKS):
            batch = ranks[b:b + H.SELECT_MAX_RANKS]
            T = len(batch)
            rk = (ctypes.c_int64 * T)(*batch)
            res = torch.empty((T, D), dtype=torch.float64, device=dev)
            nbytes = L_.hmc_select_workspace_size(D, T)
            ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
            if group is None:
                H.check(L_.hmc_order_stats(ctypes.byref(view.c), D, T, rk, H.ptr(res), H.ptr(ws), nbytes, stream),
                        "hmc_order_stats")
            else:
                state = ws[:D * T * H.SELECT_STATE_STRIDE]
                counts = ws[D * T * H.SELECT_STATE_STRIDE:]
                H.check(L_.hmc_select_init(H.ptr(state), D, T, rk, M, stream), "hmc_select_init")
                for p in range(H.SELECT_PASSES):
                    H.check(L_.hmc_select_count(ctypes.byref(view.c), D, T, p, H.ptr(state), H.ptr(counts), stream),
                            "hmc_select_count")
                    _allreduce(counts, group)
                    H.check(L_.hmc_select_pick(D, T, p, H.ptr(state), H.ptr(counts), stream), "hmc_select_pick")
                H.check(L_.hmc_select_values(D, T, H.ptr(state), H.ptr(res), stream), "hmc_select_values")
            out[b:b + T] = res.cpu().numpy()
    return out


def _total(view, group):
    """M over all ranks of the group."""
    if group is None:
        return view.M
    import torch
    m = torch.tensor([view.M], dtype=torch.int64, device=view.device)
    return int(_allreduce(m, group).item())


def _check_ranks(ranks, M):
    ranks = [int(k) for k in ranks]
    for k in ranks:
        if not 0 <= k < M:
            raise AssertionError("rank %d outside [0, %d)" % (k, M))
    return ranks


def order_stats(samples, ranks, rows=slice(1, None), group=None, device=None):
    """out[i][d] = np.sort(x[:, d])[ranks[i]] for x = samples[:, rows, :].reshape(-1, D), as a
    (len(ranks), D) NumPy array.

    samples: an [N][L][D] torch tensor or NumPy array; a device tensor is read in place, a
    non-contiguous view by its strides (the last dimension must be contiguous), never copied.  rows: a
    slice with a positive step, the rows of every chain to use; the default drops the start row as
    compute_convergence_stats does.  ranks: integers in [0, M), M = N x rows (over all ranks of
    `group`); more than 8 run as several calls.  group: a torch.distributed process group whose ranks
    each pass their own chains; None reads this process's samples alone.  device: where a host
    `samples` goes (default: the current device)."""
    view = _View(samples, rows, device, min_D=1)
    M = _total(view, group)
    ranks = _check_ranks(ranks, M)
    if not ranks:
        return np.empty((0, view.D), dtype=np.float64)
    return _order_stats(view, ranks, M, group)


def quantile_ranks(M, probs):
    """NumPy's method="linear" positions for M values: (lo, hi, g) arrays with h = (M - 1) p in
    float64, lo = floor(h), hi = ceil(h), g = h - lo."""
    p = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    if p.ndim != 1 or not np.all((p >= 0.0) & (p <= 1.0)):
        raise AssertionError("probabilities must lie in [0, 1]")
    h = (M - 1) * p
    lo = np.floor(h)
    hi = np.ceil(h)
    return lo.astype(np.int64), hi.astype(np.int64), h - lo


def lerp(a, b, g):
    """NumPy's _lerp: a + (b - a) g, and b - (b - a)(1 - g) where g >= 0.5."""
    with np.errstate(invalid="ignore", over="ignore"):
        diff = b - a
        out = a + diff * g
        upper = b - diff * (1 - g)
    return np.where(g >= 0.5, upper, out)


def quantiles(samples, probs, rows=slice(1, None), group=None, device=None):
    """np.quantile(x, probs, axis=0) (method="linear") for x = samples[:, rows, :].reshape(-1, D), as
    a (len(probs), D) NumPy array, from exact order statistics selected on the device and NumPy's
    lerp of x_(lo) and x_(hi) on the host.  A dimension that holds a NaN gives NaN for every
    probability (its largest order statistic is then NaN).  Arguments as `order_stats`."""
    view = _View(samples, rows, device, min_D=1)
    M = _total(view, group)
    if M < 1:
        raise AssertionError("quantiles of an empty sample set")
    lo, hi, g = quantile_ranks(M, probs)
    need = sorted(set(lo.tolist()) | set(hi.tolist()) | {M - 1})
    stats = _order_stats(view, need, M, group)
    at = {k: i for i, k in enumerate(need)}
    a = stats[[at[k] for k in lo.tolist()]]
    b = stats[[at[k] for k in hi.tolist()]]
    out = lerp(a, b, g[:, None])
    out[:, np.isnan(stats[at[M - 1]])] = np.nan
    return out


def credible_interval(samples, level=0.9, rows=slice(1, None), group=None, device=None):
    """The central credible interval of every dimension: the (lo, hi) pair of (D,) arrays of the
    quantiles (1 - level) / 2 and 1 - (1 - level) / 2."""
    if not 0.0 < level < 1.0:
        raise AssertionError("level must lie in (0, 1)")
    tail = (1.0 - level) / 2.0
    q = quantiles(samples, (tail, 1.0 - tail), rows=rows, group=group, device=device)
    return q[0], q[1]
