"""Posterior quantiles: hmc_order_stats (csrc/hmc_select.hip) against the best torch does on the same
GPU without a second copy of the window.

    python scripts/dev/bench_quantiles.py [--chains 65536] [--rows-per-chain 100] [--dim 100]

Config: probs (0.05, 0.5, 0.95) on a stored window of 65,536 chains x (1 + 100) rows x D = 100 of
N(0, 1) from a seeded device generator, through the view [:, 1:] (M = 6,553,600 samples per
dimension, 5.24 GB).  The ranks are the ones hmc_amd.quantiles.quantiles asks for: lo and hi of every
probability and M - 1 (the NaN detector), 7 in all, one hmc_order_stats call.
  hip:   one hmc_order_stats call on the strided view; workspace and output allocated before.
  torch: torch.sort of contiguous chunk copies, `--chunk-dims` dimensions at a time
         (view[:, :, d0:d1] transposed to [dims][M], sorted along M, the ranks gathered).
         torch.quantile refuses more than 16 M elements, and a sort of the whole window needs a
         second copy of it.
Before any time is reported the two legs must give identical order statistics (bit for bit).  One
warm-up and `--repeats` timed windows each, alternating hip / torch in one session, between device
events.  Also reported: the hip time per pass against the HBM model, bytes of the view / 8 TB/s per
pass.  `--headline` adds one hip run at 1,048,576 chains (84 GB) if the device holds it.  Writes
profiles/quantiles_bench.json.  Needs a GPU: there is no fallback.  Not a gate: bench.py is the
project's benchmark.
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
from hmc_amd.quantiles import quantile_ranks                                    # noqa: E402

HBM_BYTES_PER_S = 8e12


def stats(ms):
    ms = np.asarray(ms, dtype=float)
    return dict(ms_median=float(np.median(ms)), ms_min=float(ms.min()), ms_max=float(ms.max()), ms=ms.tolist())


def needed_ranks(M, probs):
    lo, hi, _ = quantile_ranks(M, probs)
    return sorted(set(lo.tolist()) | set(hi.tolist()) | {M - 1})


class Hip:
    def __init__(self, samples, ranks):
        N, L, D = samples.shape
        self.L, self.D, self.T = H.lib(), D, len(ranks)
        self.rk = (ctypes.c_int64 * self.T)(*ranks)
        self.nbytes = self.L.hmc_select_workspace_size(D, self.T)
        self.ws = torch.empty(self.nbytes // 8, dtype=torch.int64, device=samples.device)
        self.out = torch.empty((self.T, D), dtype=torch.float64, device=samples.device)
        self.sm = H.Samples(H.ptr(samples), N, samples.stride(0), samples.stride(1), 1, L, 1)
        self.stream = torch.cuda.current_stream(samples.device).cuda_stream

    def __call__(self):
        H.check(self.L.hmc_order_stats(ctypes.byref(self.sm), self.D, self.T, self.rk, H.ptr(self.out),
                                       H.ptr(self.ws), self.nbytes, self.stream), "hmc_order_stats")
        return self.out


def torch_sort(view, ranks, chunk_dims):
    N, R, D = view.shape
    idx = torch.as_tensor(ranks, device=view.device)
    out = torch.empty((len(ranks), D), dtype=torch.float64, device=view.device)
    for d0 in range(0, D, chunk_dims):
        cols = view[:, :, d0:d0 + chunk_dims].permute(2, 0, 1).reshape(-1, N * R)    # the chunk copy
        out[:, d0:d0 + chunk_dims] = torch.sort(cols, dim=1).values[:, idx].T
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1 << 16)
    ap.add_argument("--rows-per-chain", type=int, default=100)
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--chunk-dims", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--headline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantiles_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_quantiles.py needs a GPU"
    assert a.repeats >= 5, "at least 5 timed repeats"
    N, R, D, K = a.chains, a.rows_per_chain, a.dim, a.repeats
    probs = (0.05, 0.5, 0.95)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    samples = torch.randn(N, R + 1, D, dtype=torch.float64, device=dev, generator=g)
    view = samples[:, 1:]
    M = N * R
    ranks = needed_ranks(M, probs)
    hip = Hip(samples, ranks)

    # ---- agreement first: identical order statistics
    got = hip().cpu().numpy()
    ref = torch_sort(view, ranks, a.chunk_dims).cpu().numpy()
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), "the two legs disagree"

    times = {"hip": [], "torch": []}
    for k in range(1 + K):                                # the first window of each leg is the warm-up
        for name in ("hip", "torch"):
            ms = timed(hip if name == "hip" else (lambda: torch_sort(view, ranks, a.chunk_dims)))
            if k >= 1:
                times[name].append(ms)
    view_bytes = M * D * 8
    model_ms = view_bytes / HBM_BYTES_PER_S * 1e3
    res = dict(config=dict(chains=N, rows_per_chain=R, D=D, samples_per_dim=M, view_bytes=view_bytes, probs=probs,
                           ranks=ranks, passes=H.SELECT_PASSES, bits=H.SELECT_BITS,
                           blocks_per_tile=int(hip.L.hmc_select_grid(D, M)), workspace_bytes=int(hip.nbytes),
                           torch_leg="torch.sort of contiguous chunk copies", torch_chunk_dims=a.chunk_dims,
                           repeats=K, warmup=1, device=torch.cuda.get_device_name(0)),
               identical_order_statistics=True, hip=stats(times["hip"]), torch=stats(times["torch"]))
    res["ratio_at_medians"] = res["torch"]["ms_median"] / res["hip"]["ms_median"]
    per_pass = res["hip"]["ms_median"] / H.SELECT_PASSES
    res["hip"].update(ms_per_pass_at_median=per_pass, hbm_model_ms_per_pass=model_ms,
                      hbm_model_ms=model_ms * H.SELECT_PASSES, fraction_of_hbm_model=model_ms / per_pass,
                      read_TBps_at_median=view_bytes / (per_pass * 1e-3) / 1e12)
    if a.headline:
        del samples, view, hip
        torch.cuda.empty_cache()
        Nh = 1 << 20
        try:
            big = torch.empty(Nh, R, D, dtype=torch.float64, device=dev)
            for c0 in range(0, Nh, 1 << 16):              # filled in pieces: no second buffer of its size
                big[c0:c0 + (1 << 16)].normal_(generator=g)
            hb = Hip(big, needed_ranks(Nh * (R - 1), probs))
            hb()
            ms = [timed(hb) for _ in range(2)]
            bytes_h = Nh * (R - 1) * D * 8
            res["headline"] = dict(chains=Nh, rows_in_window=R, rows_read=R - 1, view_bytes=bytes_h, ms=ms,
                                   hbm_model_ms=bytes_h / HBM_BYTES_PER_S * 1e3 * H.SELECT_PASSES)
        except torch.OutOfMemoryError as e:
            res["headline"] = dict(skipped="the device does not hold the window: %s" % str(e).splitlines()[0])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
