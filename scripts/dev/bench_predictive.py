"""Posterior predictive / WAIC reduction: hmc_glm_predictive (csrc/hmc_pred.hip) against the code a
user would write today on the same GPU, chunked float64 torch.

    python scripts/dev/bench_predictive.py [--chains 65536] [--rows-per-chain 10] [--repeats 5]

Config: poisson, D = 32, n_eval = 1024, 65,536 chains x 10 stored rows after the start row
(samples [N][11][D], rows 1.. as HMC_sampler.waic reads them), RandomState(3) data as bench_glm.py,
samples = beta + 0.5 N(0, 1) / sqrt(D) from a seeded device generator.
  hip:   one hmc_glm_predictive call on the strided view samples[:, 1:], workspace and output
         allocated before; `--inner` calls back to back per timed window.
  torch: per chunk of `--chunk` samples z = X @ q.T, mu = exp(z), ll = y z - mu, torch.var_mean of
         both and torch.logsumexp of ll over the chunk; chunks combine by Chan's rule and logaddexp.
Before any time is reported the two results must agree (rtol 1e-9 on the means, the M2s and
logsumexp(ll)).  One warm-up and `--repeats` timed windows each, alternating hip / torch in one
session, between device events.  Writes profiles/predictive_bench.json.  Needs a GPU: there is no
fallback.  Not a gate: bench.py is the project's benchmark.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "understanding-hmc_amd")]
from hmc_amd import _lib as H                                                   # noqa: E402


def stats(ms):
    ms = np.asarray(ms, dtype=float)
    return dict(ms_median=float(np.median(ms)), ms_min=float(ms.min()), ms_max=float(ms.max()), ms=ms.tolist())


def torch_reduce(X, y, view, chunk):
    """(n, mu_mean, mu_M2, ll_mean, ll_M2, logsumexp(ll)) per evaluation row, over view [N][R][D]."""
    N, R, D = view.shape
    per = max(1, chunk // R)
    acc = None
    for c0 in range(0, N, per):
        q = view[c0:c0 + per].reshape(-1, D)
        z = X @ q.T
        mu = torch.exp(z)
        ll = y[:, None] * z - mu
        cnt = float(q.shape[0])
        vm, mm = torch.var_mean(mu, dim=1, unbiased=False)
        vl, ml = torch.var_mean(ll, dim=1, unbiased=False)
        cur = [cnt, mm, vm * cnt, ml, vl * cnt, torch.logsumexp(ll, dim=1)]
        if acc is None:
            acc = cur
            continue
        na, nb = acc[0], cnt
        n = na + nb
        for m_, v_ in ((1, 2), (3, 4)):
            delta = cur[m_] - acc[m_]
            acc[v_] = acc[v_] + cur[v_] + delta * delta * (na * nb / n)
            acc[m_] = acc[m_] + delta * (nb / n)
        acc[5] = torch.logaddexp(acc[5], cur[5])
        acc[0] = n
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1 << 16)
    ap.add_argument("--rows-per-chain", type=int, default=10)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--n-eval", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=1 << 15)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictive_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_predictive.py needs a GPU"
    assert a.repeats >= 5, "at least 5 timed repeats"
    N, R, D, n_eval, K = a.chains, a.rows_per_chain, a.dim, a.n_eval, a.repeats
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(3)
    Xh = 0.3 * rs.standard_normal((n_eval, D))
    beta = 2.0 * rs.standard_normal(D) / np.sqrt(D)
    yh = rs.poisson(np.exp(Xh @ beta)).astype(float)
    X, y = torch.as_tensor(Xh, device=dev), torch.as_tensor(yh, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    samples = torch.as_tensor(beta, device=dev) + 0.5 / np.sqrt(D) * torch.randn(N, R + 1, D, dtype=torch.float64,
                                                                                   device=dev, generator=g)
    view = samples[:, 1:]
    S = N * R
    L = H.lib()
    nbytes = L.hmc_glm_predictive_workspace_size(D, n_eval, S)
    assert nbytes > 0
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    out = torch.zeros((n_eval, H.PRED_STRIDE), dtype=torch.float64, device=dev)
    glm = H.GLM(D, n_eval, D, H.ptr(X), H.ptr(y), None, H.HMC_GLM_POISSON)
    sm = H.Samples(H.ptr(samples), N, samples.stride(0), samples.stride(1), 1, R + 1, 1)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def hip():
        H.check(L.hmc_glm_predictive(ctypes.byref(glm), ctypes.byref(sm), H.ptr(out), H.ptr(ws), nbytes, stream),
                "hmc_glm_predictive")

    # ---- agreement first
    hip()
    ref = torch_reduce(X, y, view, a.chunk)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.all(o[:, 0] == S)
    agree = {}
    for name, got, want in (("mu_mean", o[:, 1], ref[1]), ("mu_M2", o[:, 2], ref[2]), ("ll_mean", o[:, 3], ref[3]),
                            ("ll_M2", o[:, 4], ref[4]), ("logsumexp_ll", o[:, 5] + np.log(o[:, 6]), ref[5])):
        want = want.cpu().numpy()
        agree[name] = float(np.max(np.abs(got - want) / np.abs(want)))
        assert agree[name] <= 1e-9, (name, agree[name])

    # ---- timing: warm-up (above, and once more each), then alternating windows
    times = {"hip": [], "torch": []}
    for k in range(1 + K):
        for name in ("hip", "torch"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if name == "hip":
                for _ in range(a.inner):
                    hip()
            else:
                torch_reduce(X, y, view, a.chunk)
            e1.record()
            torch.cuda.synchronize()
            if k >= 1:
                times[name].append(e0.elapsed_time(e1) / (a.inner if name == "hip" else 1))
    res = dict(config=dict(family="poisson", D=D, n_eval=n_eval, chains=N, rows_per_chain=R, samples=S,
                           torch_chunk=a.chunk, repeats=K, warmup=1, hip_calls_per_window=a.inner,
                           sample_blocks=int(L.hmc_glm_predictive_blocks(D, n_eval, S)), workspace_bytes=int(nbytes),
                           device=torch.cuda.get_device_name(0)),
               max_rel_difference=agree, hip=stats(times["hip"]), torch=stats(times["torch"]))
    res["speedup_at_medians"] = res["torch"]["ms_median"] / res["hip"]["ms_median"]
    # the work the algorithm needs, from the shapes: 2 D flops per entry of Z on the matrix cores, the
    # samples read once per group of 64 evaluation rows
    res["hip"]["mfma_tflops_at_median"] = 2.0 * D * n_eval * S / (res["hip"]["ms_median"] * 1e-3) / 1e12
    res["hip"]["entries_per_s_at_median"] = float(n_eval) * S / (res["hip"]["ms_median"] * 1e-3)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
