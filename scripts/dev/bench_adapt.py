"""Cost and effect of the per-chain step multiplier of the GLM kernels (the ADAPT forms behind
hmc_glm_random_iters_adapt / hmc_glm_nuts_iters_adapt).

    python scripts/dev/bench_adapt.py [--chains 65536] [--repeats 5]

Config: bench_glm.py's data (D = 32, n = 1024, unit prior variances, RandomState(3)), Philox, Poisson.
  frozen against plain   The _adapt entry with every multiplier 1 and no adapting iteration (bit-identical
                         results) against the plain entry, alternating launch by launch in one session: one
                         warm-up launch each, then `--repeats` timed launches each between device events.
                         Random: launches of `--iters-per-launch` iterations, L ~ U{5..19}.  NUTS: d_max 8,
                         `--nuts-iters` iterations per launch, each from a fresh init.  Reported: medians and
                         ranges, the ratio of the medians, and the plain entry's own range over its median.
  wrong step             NUTS on both families from 4 and 1/4 of the recipe's dt: `--adapt-iters` adapting
                         iterations and `--nuts-iters` more with adapt_step, against the same run without;
                         n_unstable, n_dmax and the lane utilisation of the iterations after warm-up alone
                         (counter differences around the last launch), and the mean adapted multiplier.
Writes profiles/adapt_bench.json.  Needs a GPU: there is no fallback.  Not a gate: bench.py is the
project's benchmark.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "understanding-hmc_amd"), os.path.dirname(os.path.abspath(__file__))]
from bench_glm import data, stats                                               # noqa: E402
from hmc_amd import _lib as H                                                   # noqa: E402
from hmc_amd.engine import GLMEngine, GLMNutsEngine                              # noqa: E402
from hmc_amd.target import GLMTarget                                             # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def compare(plain_ms, frozen_ms):
    p, f = stats(plain_ms), stats(frozen_ms)
    return dict(plain=p, frozen_adapt=f, ratio_of_medians=f["ms_median"] / p["ms_median"],
                plain_range_over_median=(p["ms_max"] - p["ms_min"]) / p["ms_median"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1 << 16)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--iters-per-launch", type=int, default=10)
    ap.add_argument("--nuts-iters", type=int, default=10)
    ap.add_argument("--adapt-iters", type=int, default=40)
    ap.add_argument("--d-max", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adapt_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_adapt.py needs a GPU"
    assert a.repeats >= 5, "at least 5 timed repeats"
    N, S, K, D, n, I = a.chains, a.iters_per_launch, a.repeats, a.dim, a.rows, a.nuts_iters
    g = torch.Generator(device="cuda").manual_seed(0)
    out = dict(config=dict(D=D, n=n, chains=N, iters_per_launch=S, nuts_iters=I, adapt_iters=a.adapt_iters,
                           d_max=a.d_max, repeats=K, warmup_launches=1, L_low=5, L_high=20, rng="philox",
                           device=torch.cuda.get_device_name(0)))
    X, y, dt = data("poisson", D, n)
    target = GLMTarget(X, y, "poisson", 1.0)
    q_start = 0.5 * torch.randn(N, D, dtype=torch.float64, device="cuda", generator=g)

    # ---- Random: plain and frozen engines take turns
    n_iter = (1 + K) * S
    engines = {}
    for name, kw in (("plain", {}), ("frozen", dict(step_scale0=1.0))):
        eng = GLMEngine(target, N, n_iter, 0, 1, 5, 20, dt, rng="philox", seed=0, store_chain=False, **kw)
        eng.init(q_start)
        engines[name] = eng
    ms = {name: [] for name in engines}
    for k in range(1 + K):
        for name, eng in engines.items():
            t = timed(lambda: eng.run(1 + k * S, 1 + (k + 1) * S))
            if k >= 1:
                ms[name].append(t)
    assert torch.equal(engines["plain"].q, engines["frozen"].q)             # the frozen form is the plain kernel's result
    out["random_poisson"] = dict(compare(ms["plain"], ms["frozen"]), dt=dt)
    del engines
    torch.cuda.empty_cache()

    # ---- NUTS: plain and frozen runs take turns, each from a fresh init
    ms, last = {"plain": [], "frozen": []}, {}
    for k in range(1 + K):
        for name, kw in (("plain", {}), ("frozen", dict(step_scale0=1.0))):
            eng = GLMNutsEngine(target, N, I, 0, 1, a.d_max, dt, rng="philox", seed=0, store_chain=False,
                                on_dmax="break", **kw)
            eng.init(q_start)
            t = timed(lambda: eng.run(1, I + 1))
            if k >= 1:
                ms[name].append(t)
            last[name] = eng.q.clone()
    assert torch.equal(last["plain"], last["frozen"])
    out["nuts_poisson"] = dict(compare(ms["plain"], ms["frozen"]), dt=dt)

    # ---- NUTS from a deliberately wrong step, with and without adapt_step
    W = a.adapt_iters + 1                                   # warm_up: iterations 1 .. adapt_iters adapt
    for family in ("poisson", "bernoulli"):
        Xf, yf, dtf = data(family, D, n)
        for label, factor in (("4x", 4.0), ("quarter", 0.25)):
            for adapt in (False, True):
                eng = GLMNutsEngine(GLMTarget(Xf, yf, family, 1.0), N, W - 1 + I, W, 1, a.d_max, factor * dtf,
                                    rng="philox", seed=0, store_chain=False, on_dmax="break", adapt_step=adapt)
                eng.init(q_start)
                eng.run(1, W)
                torch.cuda.synchronize()
                c0 = eng.read_counters()
                t = timed(lambda: eng.run(W, W + I))
                c = eng.read_counters() - c0
                lf, steps = int(c[H.CNT_LEAPFROG]), int(c[H.CNT_LEAPFROG_SQ])
                rec = dict(dt=factor * dtf, ms_after_warm_up=t, leapfrogs=lf, n_unstable=int(c[H.CNT_UNSTABLE]),
                           n_dmax=int(c[H.CNT_DMAX]), trees=N * I, lane_utilisation=lf / (16.0 * steps),
                           finite_chains=int(torch.isfinite(eng.q).all(dim=1).sum()))
                if adapt:
                    s = eng.step_scale
                    st = eng.adapt_state
                    rec.update(step_scale_mean=float(s.mean()), step_scale_min=float(s.min()),
                               step_scale_max=float(s.max()),
                               accept_stat_after_warm_up=float((st[:, 6].sum() / st[:, 7].sum())))
                out["wrong_step_%s_%s_%s" % (family, label, "adaptive" if adapt else "fixed")] = rec
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
