"""Throughput of the GLM kernels: the Random sampler through hmc_glm_random_iters (both families)
against hmc_logit_random_iters, and NUTS (csrc/hmc_glm_nuts.hip) on both families.

    python scripts/dev/bench_glm.py [--chains 262144] [--nuts-chains 65536] [--repeats 5]

Config: D = 32, n = 1024, unit prior variances, RandomState(3), Philox.
  bernoulli: bench_logistic.py's data (X and the coefficients standard normal, labels from the model),
             dt = 1 / sqrt(lambda_max(X^T X / 4 + I))
  poisson:   X = 0.3 N(0, 1), beta = 2 N(0, 1) / sqrt(D), y ~ Poisson(exp(X beta)),
             dt = 1 / sqrt(lambda_max(X^T diag(exp(X beta)) X + I))
Random: L ~ U{5..19}, launches of `--iters-per-launch` iterations, every row into a circular window;
the three engines (logistic entry, GLM entry Bernoulli, GLM entry Poisson) take turns launch by launch
in one session: one warm-up launch each, then `--repeats` timed launches each between device events.
NUTS: d_max = 8, `--nuts-iters` iterations per run in one launch, no q_chain; one warm-up run, then
`--repeats` timed runs (each from a fresh init) per family.  Reported per leg: median and range of
the launch times, leapfrog/s at the median; for NUTS also the lane utilisation LEAPFROG / (16 wave
steps) and the time per wave step of one wave slot (elapsed x wave slots in flight / wave steps, the
slots being min(tiles, CUs x 4 SIMDs x waves per SIMD)), next to the Random kernel's time per gradient
pass estimated the same way (its tile takes max L of its 16 chains + 1 passes per iteration; the
expectation of that maximum for L ~ U{5..19} is used, not a count).
Writes profiles/glm_bench.json.  Needs a GPU: there is no fallback.  Not a gate: bench.py is the
project's benchmark.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "understanding-hmc_amd")]
from hmc_amd import _lib as H                                                   # noqa: E402
from hmc_amd.engine import GLMEngine, GLMNutsEngine, LogisticEngine              # noqa: E402
from hmc_amd.target import GLMTarget, LogisticTarget                             # noqa: E402


def data(family, D, n, seed=3):
    rs = np.random.RandomState(seed)
    if family == "poisson":
        X = 0.3 * rs.standard_normal((n, D))
        beta = 2.0 * rs.standard_normal(D) / np.sqrt(D)
        y = rs.poisson(np.exp(X @ beta)).astype(float)
        W = np.exp(X @ beta)
    else:
        X = rs.standard_normal((n, D))
        beta = rs.standard_normal(D)
        y = (rs.random_sample(n) < 1 / (1 + np.exp(-X @ beta))).astype(float)
        W = np.full(n, 0.25)
    dt = float(1.0 / np.sqrt(np.linalg.eigvalsh(X.T @ (W[:, None] * X) + np.eye(D)).max()))
    return X, y, dt


def stats(ms):
    ms = np.asarray(ms, dtype=float)
    return dict(ms_median=float(np.median(ms)), ms_min=float(ms.min()), ms_max=float(ms.max()), ms=ms.tolist())


def wave_slots(tiles, D):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return min(tiles, cus * 4 * (2 if D <= 32 else 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1 << 18)
    ap.add_argument("--nuts-chains", type=int, default=1 << 16)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--iters-per-launch", type=int, default=10)
    ap.add_argument("--nuts-iters", type=int, default=20)
    ap.add_argument("--d-max", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-rows", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glm_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_glm.py needs a GPU"
    assert a.repeats >= 5, "at least 5 timed repeats"
    N, S, K, R, D, n = a.chains, a.iters_per_launch, a.repeats, a.window_rows, a.dim, a.rows
    g = torch.Generator(device="cuda").manual_seed(0)
    out = dict(config=dict(D=D, n=n, chains=N, iters_per_launch=S, repeats=K, warmup_launches=1, window_rows=R,
                           L_low=5, L_high=20, nuts_chains=a.nuts_chains, nuts_iters=a.nuts_iters, d_max=a.d_max,
                           rng="philox", device=torch.cuda.get_device_name(0)))

    # ---- Random: the three engines interleaved
    Xb, yb, dtb = data("bernoulli", D, n)
    Xp, yp, dtp = data("poisson", D, n)
    n_iter = (1 + K) * S
    legs = [("logit_entry_bernoulli", LogisticEngine, LogisticTarget(Xb, yb, 1.0), dtb),
            ("glm_entry_bernoulli", GLMEngine, GLMTarget(Xb, yb, "bernoulli", 1.0), dtb),
            ("glm_entry_poisson", GLMEngine, GLMTarget(Xp, yp, "poisson", 1.0), dtp)]
    q_start = 0.5 * torch.randn(N, D, dtype=torch.float64, device="cuda", generator=g)
    engines = []
    for name, cls, t, dt in legs:
        eng = cls(t, N, n_iter, 0, 1, 5, 20, dt, rng="philox", seed=0, fp_mode="fast", store_chain=False)
        eng.set_chain_window(torch.zeros((N, R, D), dtype=torch.float64, device="cuda"), 0)
        eng.init(q_start)
        engines.append(eng)
    times = {name: [] for name, *_ in legs}
    c0 = {}
    for k in range(1 + K):
        for (name, *_), eng in zip(legs, engines):
            if k == 1:
                torch.cuda.synchronize()
                c0[name] = eng.read_counters()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.run(1 + k * S, 1 + (k + 1) * S)
            e1.record()
            torch.cuda.synchronize()
            if k >= 1:
                times[name].append(e0.elapsed_time(e1))
    Lmax = np.random.RandomState(0).randint(5, 20, size=(200000, 16)).max(axis=1).mean()   # E[max of 16 L]
    tiles = (N + 15) // 16
    for (name, _, _, dt), eng in zip(legs, engines):
        c = eng.read_counters() - c0[name]
        st = stats(times[name])
        lf = int(c[H.CNT_LEAPFROG])
        passes = tiles * S * (Lmax + 1.0)                                   # per launch, estimated
        out["random_" + name] = dict(st, dt=dt, leapfrogs=lf, leapfrog_per_s=lf / K / (st["ms_median"] / 1e3),
                                     accept_rate=float(c[H.CNT_ACCEPT] + c[H.CNT_ACCEPT_WU]) / (N * K * S),
                                     us_per_gradient_pass_per_wave_slot_estimated=st["ms_median"] * 1e3 *
                                     wave_slots(tiles, D) / passes)
    del engines
    torch.cuda.empty_cache()

    # ---- NUTS, both families
    NN, I = a.nuts_chains, a.nuts_iters
    qn = 0.5 * torch.randn(NN, D, dtype=torch.float64, device="cuda", generator=g)
    for family, X, y, dt in (("bernoulli", Xb, yb, dtb), ("poisson", Xp, yp, dtp)):
        ms, cnt = [], None
        for k in range(1 + K):
            eng = GLMNutsEngine(GLMTarget(X, y, family, 1.0), NN, I, 0, 1, a.d_max, dt, rng="philox", seed=0,
                                store_chain=False, on_dmax="break")
            eng.init(qn)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.run(1, I + 1)
            e1.record()
            torch.cuda.synchronize()
            if k >= 1:
                ms.append(e0.elapsed_time(e1))
            cnt = eng.read_counters()
        st = stats(ms)
        lf, steps = int(cnt[H.CNT_LEAPFROG]), int(cnt[H.CNT_LEAPFROG_SQ])
        tiles_n = (NN + 15) // 16
        out["nuts_" + family] = dict(st, dt=dt, leapfrogs=lf, wave_steps=steps, n_dmax=int(cnt[H.CNT_DMAX]),
                                     n_unstable=int(cnt[H.CNT_UNSTABLE]),
                                     leapfrog_per_s=lf / (st["ms_median"] / 1e3),
                                     lane_utilisation=lf / (16.0 * steps),
                                     leapfrogs_per_chain_iteration=lf / float(NN * I),
                                     us_per_wave_step_per_wave_slot=st["ms_median"] * 1e3 * wave_slots(tiles_n, D) / steps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
