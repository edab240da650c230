"""Throughput of the Gaussian-mixture kernel (csrc/hmc_mix.hip) next to the general-diagonal MVN
kernel (GEN, non-identity precision) at the same shape, in one process, alternating launches.

    python scripts/dev/bench_mixture.py [--chains 1048576] [--iters-per-launch 20] [--launches 20]

Config: D = 100, K = 4 components (the test recipe's seed 3, sep 4), Philox, L ~ U{5..19}, dt = 0.1,
every row stored into a circular window of 100 rows (one window, shared by the two engines, as
bench.py's storage path).  Warm-up launches first, then `--launches` timed launches of each engine
between device events.  Writes profiles/mixture_bench.json: leapfrog/s of both, their ratio, and the
bytes a launch has to move.  Needs a GPU: there is no fallback, and without one nothing is written.
Not a gate: bench.py is the project's benchmark.
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
from hmc_amd.engine import MixtureEngine, RandomEngine           # noqa: E402
from hmc_amd.target import MixtureTarget, MVNTarget              # noqa: E402


def mixture(D=100, K=4, sep=4.0, seed=3):
    rs = np.random.RandomState(seed)
    w = rs.uniform(0.5, 1.5, K)
    w /= w.sum()
    mu = rs.standard_normal((K, D))
    mu *= sep / np.linalg.norm(mu, axis=1, keepdims=True)
    return MixtureTarget(w, mu, rs.uniform(0.5, 2.0, (K, D)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1 << 20)
    ap.add_argument("--iters-per-launch", type=int, default=20)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window-rows", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixture_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mixture.py needs a GPU"
    N, S, K, W, R, D = a.chains, a.iters_per_launch, a.launches, a.warmup, a.window_rows, 100
    n_iter = (W + K) * S
    mix = mixture(D)
    gen = MVNTarget(np.zeros(D), np.diag(np.random.RandomState(3).uniform(0.5, 2.0, D)))
    kw = dict(rng="philox", seed=0, fp_mode="fast", store_chain=False)
    engines = {"mixture": MixtureEngine(mix, N, n_iter, 0, 1, 5, 20, 0.1, **kw),
               "mvn_gen": RandomEngine(gen, N, n_iter, 0, 1, 5, 20, 0.1, **kw)}
    window = torch.zeros((N, R, D), dtype=torch.float64, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    comp = torch.randint(mix.K, (N,), device="cuda", generator=g)
    q_start = torch.as_tensor(mix.mu).cuda()[comp] + torch.randn(N, D, dtype=torch.float64, device="cuda", generator=g)
    for e in engines.values():
        e.set_chain_window(window, 0)
        e.init(q_start)
    it = 1
    for _ in range(W):
        for e in engines.values():
            e.run(it, it + S)
        it += S
    torch.cuda.synchronize()
    c0 = {k: e.read_counters() for k, e in engines.items()}
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(K)]
          for k in engines}
    for j in range(K):                         # alternating: both see the same clocks and neighbours
        for k, e in engines.items():
            ev[k][j][0].record()
            e.run(it, it + S)
            ev[k][j][1].record()
        it += S
    torch.cuda.synchronize()
    out = dict(config=dict(D=D, K=mix.K, chains=N, iters_per_launch=S, launches=K, warmup_launches=W, window_rows=R,
                           L_low=5, L_high=20, dt=0.1, rng="philox", device=torch.cuda.get_device_name(0)),
               # q in and out, one q_chain row + E + dE per iteration, E_prev in and out
               required_bytes_per_launch=N * (S * (8 * D + 16) + 16 * D + 16))
    for k, e in engines.items():
        ms = np.array([s_.elapsed_time(t_) for s_, t_ in ev[k]])
        c = e.read_counters() - c0[k]
        lf = int(c[H.CNT_LEAPFROG])
        out[k] = dict(ms_per_launch_mean=float(ms.mean()), ms_per_launch_min=float(ms.min()),
                      ms_per_launch_max=float(ms.max()), leapfrogs=lf,
                      leapfrog_per_s=lf / (ms.sum() / 1e3),
                      accept_rate=float(c[H.CNT_ACCEPT] + c[H.CNT_ACCEPT_WU]) / (N * K * S),
                      required_GBps=out["required_bytes_per_launch"] / (ms.mean() / 1e3) / 1e9)
    out["ratio_mixture_over_mvn_gen"] = out["mixture"]["leapfrog_per_s"] / out["mvn_gen"]["leapfrog_per_s"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
