"""Throughput of the logistic-regression kernel (csrc/hmc_logit.hip).

    python scripts/dev/bench_logistic.py [--chains 262144] [--iters-per-launch 20] [--launches 20]

Config: D = 32, n = 1024 (X and the true coefficients standard normal, labels drawn from the model,
unit prior variances, RandomState(3)), Philox, L ~ U{5..19}, dt = 1 / sqrt(lambda_max(X^T X / 4 + I)),
every row stored into a circular window of 100 rows (bench.py's storage path).  Warm-up launches
first, then `--launches` timed launches between device events.  Writes profiles/logistic_bench.json:
ms per launch, leapfrog/s and the fraction of the FP64 matrix peak at 4 n D flop per leapfrog (the
two products of one gradient; the peak figure is bench.py's).  Needs a GPU: there is no fallback,
and without one nothing is written.  Not a gate: bench.py is the project's benchmark.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "understanding-hmc_amd")]
from hmc_amd import _lib as H                                   # noqa: E402
from hmc_amd.engine import LogisticEngine                        # noqa: E402
from hmc_amd.target import LogisticTarget                        # noqa: E402

FP64_PEAK_TFLOPS = 78.6      # bench.py's figure: MI355X FP64 vector = FP64 matrix peak (spec)


def logistic(D, n, seed=3):
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((n, D))
    beta = rs.standard_normal(D)
    y = (rs.random_sample(n) < 1 / (1 + np.exp(-X @ beta))).astype(float)
    return LogisticTarget(X, y, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1 << 18)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--iters-per-launch", type=int, default=20)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window-rows", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logistic_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_logistic.py needs a GPU"
    N, S, K, W, R, D, n = a.chains, a.iters_per_launch, a.launches, a.warmup, a.window_rows, a.dim, a.rows
    n_iter = (W + K) * S
    t = logistic(D, n)
    dt = float(1.0 / np.sqrt(np.linalg.eigvalsh(t.X.T @ t.X / 4 + np.diag(t.prior_prec)).max()))
    eng = LogisticEngine(t, N, n_iter, 0, 1, 5, 20, dt, rng="philox", seed=0, fp_mode="fast", store_chain=False)
    window = torch.zeros((N, R, D), dtype=torch.float64, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    q_start = 0.5 * torch.randn(N, D, dtype=torch.float64, device="cuda", generator=g)
    eng.set_chain_window(window, 0)
    eng.init(q_start)
    it = 1
    for _ in range(W):
        eng.run(it, it + S)
        it += S
    torch.cuda.synchronize()
    c0 = eng.read_counters()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(K)]
    for j in range(K):
        ev[j][0].record()
        eng.run(it, it + S)
        ev[j][1].record()
        it += S
    torch.cuda.synchronize()
    ms = np.array([s_.elapsed_time(t_) for s_, t_ in ev])
    c = eng.read_counters() - c0
    lf = int(c[H.CNT_LEAPFROG])
    secs = ms.sum() / 1e3
    # gradients evaluated: one per leapfrog step plus one at each iteration's start point; the tile
    # of 16 chains steps to its longest trajectory, which the leapfrog count does not include
    tflops_leapfrog = 4.0 * n * D * lf / secs / 1e12
    out = dict(config=dict(D=D, n=n, chains=N, iters_per_launch=S, launches=K, warmup_launches=W, window_rows=R,
                           L_low=5, L_high=20, dt=dt, rng="philox", device=torch.cuda.get_device_name(0)),
               ms_per_launch_mean=float(ms.mean()), ms_per_launch_min=float(ms.min()),
               ms_per_launch_max=float(ms.max()), leapfrogs=lf, leapfrog_per_s=lf / secs,
               accept_rate=float(c[H.CNT_ACCEPT] + c[H.CNT_ACCEPT_WU]) / (N * K * S),
               flop_per_leapfrog=4 * n * D, tflops_at_4nD_per_leapfrog=tflops_leapfrog,
               fp64_peak_tflops=FP64_PEAK_TFLOPS, frac_fp64_mfma_peak=tflops_leapfrog / FP64_PEAK_TFLOPS)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
