"""Write tests/golden/random_routes.json: what the Random sampler's host queries answer over a grid
that crosses every edge of the kernel choice (csrc/hmc_route.cpp), from the library that HMC_AMD_LIB
names (default: the tree's own).  Host-only queries, no GPU; tests/test_layout_query.py compares the
tree's library with the file, entry for entry.  The committed file came from the library built at
the commit before the choice moved into csrc/hmc_route.cpp:

    HMC_AMD_LIB=<that commit's libhmc.so> python scripts/dev/gen_random_routes.py

Per entry: [D, kind, L_low, L_high, fp_mode, rng_mode, variant, dt] and the answers
[layout status, K, lpc, cpw, wave, leapfrog form, workspace bytes at n = 0, 1, 17, 65536].
variant: "none" (no kinetic descriptor: hmc_random_layout and hmc_random_workspace_size), "id"
(identity kinetic), one of q0 / prec / minv / p_scale / dt_vec set on a diagonal target, or "mass"
(a full cov_p on a dense target).  The pointers are never followed on the host.
"""
import ctypes
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "understanding-hmc_amd"))

DIMS = (1, 2, 63, 64, 65, 66, 96, 97, 98, 100, 112, 113, 128, 129, 320, 321, 2047, 2048, 2049, 2050)
RANGES = ((5, 20), (1, 2), (0, 3), (1, 4096), (1, 4097), (4000, 4096), (12, 13))
NS = (0, 1, 17, 65536)
DTS = (9.99e-4, 1e-3, 0.1, 1.4142, 1.4143, 1.99, 1.9999, 2.0, -0.1)
DIAG_VARIANTS = ("none", "id", "q0", "prec", "minv", "p_scale", "dt_vec")
DENSE_VARIANTS = ("none", "id", "mass")
PTR = 0x1000   # a non-null device pointer the host code never follows


def drift_edges(dt):
    """One L_high on either side of the three-term rule's L_high m <= 2e5 dt (1 - dt^2 / 4), m = 2 from
    dt^2 = 2 on; past that, also the pair the rule without m would have as its edge."""
    bound = 2e5 * dt * (1.0 - 0.25 * dt * dt)
    edge = int(math.floor(bound / (2.0 if dt * dt >= 2.0 else 1.0)))
    plain = int(math.floor(bound))
    return (edge, edge + 1) + ((plain, plain + 1) if plain != edge else ())


def cases():
    """The grid, thinned where a factor cannot matter (the full cross product is some 6000 entries):
    - a dense target's answers depend on D and on the mass alone: one range, FAST, Philox;
    - the modes only matter where the wave-per-chain shapes are (64 < D <= 2048): below and above,
      FAST with Philox stands for all four, in between EXACT with replay is left to its two halves;
    - q0, prec, minv, p_scale and dt_vec each only switch the general-diagonal form on: each in
      turn on a short and a long range over the dimensions next to an edge;
    - dt only enters through the three-term rule: the step-size grid runs on one lane-group-free
      shape per wave kernel family (65: wave, 100: four-chain, 129: two pairs per lane)."""
    out = []
    for D in DIMS:
        out += [(D, 1, 5, 20, 1, 1, var, 0.1) for var in DENSE_VARIANTS]
        modes = ((1, 1), (0, 1), (1, 0)) if 64 < D <= 2048 else ((1, 1),)
        out += [(D, 0, lo, hi, fp, rng, var, 0.1)
                for lo, hi in RANGES for fp, rng in modes for var in ("none", "id")]
    for D in (2, 64, 65, 100, 112, 2048, 2049):
        out += [(D, 0, lo, hi, 1, 1, var, 0.1) for lo, hi in ((5, 20), (1, 4096)) for var in DIAG_VARIANTS[2:]]
    for D in (65, 100, 129):
        out += [(D, 0, lo, hi, 1, 1, "id", dt) for lo, hi in ((5, 20), (1, 4096)) for dt in DTS if dt != 0.1]
    # the trajectory-length side of the three-term rule, on the four-chain and the wave shapes
    for D in (100, 129):
        for dt in (1e-3, 1.999):
            for hi in drift_edges(dt):
                out.append((D, 0, 1, hi, 1, 1, "id", dt))
    return out


def answers(H, L, case):
    D, kind, lo, hi, fp, rng, var, dt = case
    T = H.Target(D, kind, PTR if var == "q0" else None, PTR if (var == "prec" or kind == 1) else None, 0.0)
    S = H.Schedule(0, 0, 1, 0, 1, 2, lo, hi, 1, 1, rng, fp, 10, 0, 0)
    K = None
    if var != "none":
        K = H.Kinetic(PTR if var == "minv" else None, PTR if var == "p_scale" else None,
                      PTR if var == "dt_vec" else None, float(dt), *((PTR,) * 3 if var == "mass" else (None,) * 3))
    kp = ctypes.byref(K) if K is not None else None
    out = (ctypes.c_int32 * 4)(-1, -1, -1, -1)
    status = L.hmc_random_layout_ex(ctypes.byref(T), kp, ctypes.byref(S), ctypes.byref(out))
    form = L.hmc_random_leapfrog_form(ctypes.byref(T), kp, ctypes.byref(S))
    sizes = [L.hmc_random_workspace_size_ex(ctypes.byref(T), kp, n) for n in NS]
    return [status] + list(out) + [form] + sizes


def table():
    from hmc_amd import _lib as H
    L = H.lib()
    assert (H.HMC_TARGET_DIAG, H.HMC_TARGET_DENSE) == (0, 1) and (H.HMC_MODE_EXACT, H.HMC_MODE_FAST) == (0, 1)
    assert (H.HMC_RNG_REPLAY, H.HMC_RNG_PHILOX) == (0, 1)
    return [[list(c), answers(H, L, c)] for c in cases()]


def main():
    from hmc_amd import _lib as H
    rows = table()
    out = os.path.join(ROOT, "tests", "golden", "random_routes.json")
    with open(out, "w") as f:
        json.dump({"case_columns": ["D", "kind", "L_low", "L_high", "fp_mode", "rng_mode", "variant", "dt"],
                   "answer_columns": ["status", "K", "lpc", "cpw", "wave", "form"] + ["bytes_n%d" % n for n in NS],
                   "entries": rows}, f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d entries from %s" % (out, len(rows), H.LIB_PATH))


if __name__ == "__main__":
    main()
