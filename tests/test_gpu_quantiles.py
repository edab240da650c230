"""Exact order statistics and quantiles on the GPU (csrc/hmc_select.hip behind hmc_select_* and
hmc_order_stats, hmc_amd.quantiles, HMC_sampler.quantiles / .credible_interval) against np.sort and
np.quantile of the same view materialised on the host.

Order statistics carry no tolerance: bit for bit, except that a zero may come back with either sign
(compared with ==) and that every NaN comes back as the canonical one.

Quantiles carry none either.  hmc_amd.quantiles.lerp restates NumPy's _lerp operation for operation,
its g >= 0.5 branch included, on exact order statistics, so every quantile is asserted equal to
np.quantile's, bit for bit (a zero by ==, for the reason above), wherever x_(lo), x_(lo + 1) and x_(hi)
are finite.  The entries left out, and why: NumPy lerps x_(lo) with x_(lo + 1) even where
g = 0 and hi = ceil(h) = lo, and forms inf - inf or 0 * inf = NaN when one of them is infinite (only
the "mix" column holds infinities); there the two sides are compared for NaN in the same places
only where x_(lo) or x_(hi) itself is infinite, and not at all where x_(lo + 1) alone is (NumPy gives
NaN, the issue's hi = ceil(h) gives x_(lo)).  The order-statistic tests cover those columns exactly.
The probabilities are such that (M - 1) p is either an exact integer or at least 1e-6 away from one
(asserted in check_quantiles, and at import that an interior exact integer occurs among the cases),
so lo and hi cannot differ between two float64 evaluations of it."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 2, 1), (3, 5, 3), (7, 9, 16), (5, 12, 17), (33, 21, 100), (4, 6, 130)]
ROWS = [slice(1, None), slice(2, None, 3)]
PROBS = (0.05, 0.5, 0.95, 0.0, 1.0, 0.3)
DENORM_MIN = 5e-324
# (M - 1) p is an exact integer for an interior p in at least one (shape, rows) case
assert any(M > 2 and 0 < p < 1 and ((M - 1) * np.float64(p)).is_integer()
           for N, L, D in SHAPES for rows in ROWS for p in PROBS
           for M in [N * len(range(*rows.indices(L)))])


# ------------------------------------------------------------------------------------------ inputs
def special_columns(n, rs):
    """Columns that break a radix select, each of n values: name -> column."""
    a = 1.2345678
    b = np.nextafter(a, 2.0)                                        # differs in the last mantissa bit only
    base = np.array([-3.7], dtype=np.float64).view(np.uint64)[0] & ~np.uint64(0xFF)
    low = rs.randint(0, 256, size=n).astype(np.uint64)
    mix = np.array([-np.inf, np.inf, -0.0, 0.0, DENORM_MIN, -DENORM_MIN, 3 * DENORM_MIN, -2.5, -1e-300, 1e300,
                    -1e300, 2.0 ** -1022, 1.0])
    five = np.array([-1.5, -1.5 + 2.0 ** -52, 0.0, 7.25, 7.25 * (1 + 2.0 ** -52)])
    return {
        "equal": np.full(n, -0.4375),
        "last_bit": np.where(rs.random_sample(n) < 0.5, a, b),
        "top56": (base | low).view(np.float64),                     # equal in their top 56 bits
        "mix": mix[rs.randint(0, len(mix), size=n)],
        "ties": five[rs.randint(0, len(five), size=n)],
    }


SPECIAL_AT = {"equal": 1, "last_bit": 3, "top56": 5, "mix": 7, "ties": 9}     # beside N(0, 1) columns


def make_data(N, L, D, seed=0):
    """[N][L][D] of N(0, 1) with every special column whose index exists (D = 1: N(0, 1) alone)."""
    rs = np.random.RandomState(100 * D + 10 * L + N + seed)
    x = rs.standard_normal((N, L, D))
    for name, col in special_columns(N * L, rs).items():
        if SPECIAL_AT[name] < D:
            x[:, :, SPECIAL_AT[name]] = col.reshape(N, L)
    return x


def flat(x, rows):
    return np.ascontiguousarray(x[:, rows, :]).reshape(-1, x.shape[2])


def assert_same_values(got, ref, label=""):
    """Bit for bit; zeros by ==; NaN where the reference has NaN."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (label, got.shape, ref.shape)
    same = (got.view(np.uint64) == ref.view(np.uint64)) | ((got == 0) & (ref == 0)) | (np.isnan(got) & np.isnan(ref))
    assert same.all(), (label, np.argwhere(~same)[:5], got[~same][:5], ref[~same][:5])


def ranks_for(M, extra=()):
    """0, M - 1, a repeated rank, two adjacent ranks (as far as M has them)."""
    mid = M // 2
    r = [0, M - 1, mid, mid, min(mid + 1, M - 1), M // 3]
    return [k for k in list(extra) + r if 0 <= k < M][:8]


def boundary_ranks(col):
    """The two ranks on either side of the boundary between the two values of the last_bit column."""
    n_low = int((col == col.min()).sum())
    return [k for k in (n_low - 1, n_low) if 0 <= k < len(col)]


# ------------------------------------------------------------------------------------------ order statistics
@pytest.mark.parametrize("rows", ROWS, ids=["rows1", "rows2by3"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_order_stats_match_np_sort(shape, rows):
    from hmc_amd.quantiles import order_stats
    N, L, D = shape
    x = make_data(N, L, D)
    x2 = flat(x, rows)
    M = x2.shape[0]
    xd = torch.as_tensor(x, device=DEV)
    if M == 0:
        assert order_stats(xd, [], rows=rows).shape == (0, D)
        with pytest.raises(AssertionError):
            order_stats(xd, [0], rows=rows)
        return
    extra = boundary_ranks(x2[:, SPECIAL_AT["last_bit"]]) if D > SPECIAL_AT["last_bit"] else ()
    ranks = ranks_for(M, extra)
    ref = np.sort(x2, axis=0)[ranks]
    assert_same_values(order_stats(xd, ranks, rows=rows), ref, "device tensor")
    assert_same_values(order_stats(x, ranks, rows=rows), ref, "host array")


@pytest.mark.parametrize("name", list(SPECIAL_AT))
def test_special_columns_every_rank(name):
    """Every rank of every special column (more than 8 ranks: the Python batching), beside N(0, 1)
    columns that must not notice."""
    from hmc_amd.quantiles import order_stats
    N, L, D = 5, 12, 17
    x = make_data(N, L, D, seed=3)
    x2 = flat(x, slice(1, None))
    M = x2.shape[0]
    col = SPECIAL_AT[name]
    if name == "last_bit":
        n_low = int((x2[:, col] == x2[:, col].min()).sum())
        assert 0.25 * M < n_low < 0.75 * M                              # split about 50 / 50
    if name == "top56":
        assert len(set((x2[:, col].view(np.uint64) >> np.uint64(8)).tolist())) == 1
    if name == "mix":
        c = x2[:, col]
        assert np.isinf(c).any() and (c < 0).any() and (np.abs(c) == DENORM_MIN).any() and \
            np.signbit(c[c == 0]).any() and (~np.signbit(c[c == 0])).any()
    ranks = list(range(M))
    got = order_stats(torch.as_tensor(x, device=DEV), ranks)
    assert_same_values(got, np.sort(x2, axis=0), name)


def test_more_than_eight_ranks():
    from hmc_amd.quantiles import order_stats
    x = make_data(33, 21, 100)
    x2 = flat(x, slice(1, None))
    M = x2.shape[0]
    ranks = [0, M - 1, 5, 5, 6, 17, 100, 101, 329, 330, 331, 400, 400, 512, 600, 657, 658, 1, 2]
    assert len(ranks) > 2 * 8
    assert_same_values(order_stats(torch.as_tensor(x, device=DEV), ranks), np.sort(x2, axis=0)[ranks])


def test_non_contiguous_view():
    """A slice of a larger tensor: padded chain stride, row_stride > D, an offset base."""
    from hmc_amd.quantiles import order_stats, quantiles
    big = torch.as_tensor(np.random.RandomState(5).standard_normal((9, 14, 40)), device=DEV)
    v = big[2:7, 1:13, 5:28]
    assert not v.is_contiguous() and v.stride(1) == 40 > v.shape[2] and v.stride(0) == 14 * 40
    for rows in ROWS:
        x2 = flat(v.cpu().numpy(), rows)
        M = x2.shape[0]
        ranks = ranks_for(M)
        assert_same_values(order_stats(v, ranks, rows=rows), np.sort(x2, axis=0)[ranks], str(rows))
        check_quantiles(quantiles(v, PROBS, rows=rows), x2, PROBS)


def test_tile_spanning_three_blocks_with_a_short_last_block():
    """A shape chosen from hmc_select_grid: one tile of dimensions over >= 3 sample blocks, the last
    one short."""
    from hmc_amd import _lib as H
    from hmc_amd.quantiles import order_stats
    grid = H.lib().hmc_select_grid
    D, N, L = 3, 50, 52
    M = N * (L - 1)
    per = next(m for m in range(1, 1 << 16) if grid(D, m + 1) == 2)     # samples of a full block
    blocks = grid(D, M)
    print("samples per block %d, M %d, blocks %d, last block %d" % (per, M, blocks, M - (blocks - 1) * per))
    assert blocks == -(-M // per) and blocks >= 3 and M % per != 0
    x = make_data(N, L, D)
    x2 = flat(x, slice(1, None))
    ranks = [0, M - 1, per - 1, per, 2 * per, M // 2, M // 2, M // 2 + 1]
    assert_same_values(order_stats(torch.as_tensor(x, device=DEV), ranks), np.sort(x2, axis=0)[ranks])


# ------------------------------------------------------------------------------------------ NaN
@pytest.mark.parametrize("nan_bits", [0x7FF8000000000000, 0xFFF8000000000001], ids=["nan", "negative_nan"])
def test_nan_sorts_last_and_stays_in_its_dimension(nan_bits):
    from hmc_amd.quantiles import order_stats, quantiles
    x = make_data(7, 9, 16)
    rows = slice(1, None)
    M = flat(x, rows).shape[0]
    ranks = [0, M // 2, M - 2, M - 1]
    clean_s = order_stats(torch.as_tensor(x, device=DEV), ranks)
    clean_q = quantiles(torch.as_tensor(x, device=DEV), PROBS)
    y = x.copy()
    y[3, 4, 6] = np.array([nan_bits], dtype=np.uint64).view(np.float64)[0]
    assert np.isnan(y[3, 4, 6])
    got_s = order_stats(torch.as_tensor(y, device=DEV), ranks)
    got_q = quantiles(torch.as_tensor(y, device=DEV), PROBS)
    ref = np.sort(flat(y, rows), axis=0)[ranks]                    # NumPy sorts NaN last
    assert np.isnan(ref[3, 6]) and not np.isnan(ref[2, 6])
    assert_same_values(got_s, ref)
    assert np.isnan(got_q[:, 6]).all()
    with np.errstate(invalid="ignore"):
        assert np.isnan(np.quantile(flat(y, rows), PROBS, axis=0)[:, 6]).all()
    others = np.arange(16) != 6
    assert np.array_equal(got_s[:, others].view(np.uint64), clean_s[:, others].view(np.uint64))
    assert np.array_equal(got_q[:, others].view(np.uint64), clean_q[:, others].view(np.uint64))


# ------------------------------------------------------------------------------------------ shards
def staged(parts, ranks, M, D):
    """The staged C entries: count on every part, the tables added on the device, one pick per pass.
    Returns (state, values) as host arrays."""
    from hmc_amd import _lib as H
    from hmc_amd.quantiles import _View
    lib = H.lib()
    T = len(ranks)
    rk = (ctypes.c_int64 * T)(*ranks)
    state = torch.full((D * T * H.SELECT_STATE_STRIDE,), -1, dtype=torch.int64, device=DEV)
    total = torch.empty(D * T * H.SELECT_BINS, dtype=torch.int64, device=DEV)
    counts = torch.full_like(total, 12345)                          # count zeroes it itself
    out = torch.empty((T, D), dtype=torch.float64, device=DEV)
    views = [_View(p, slice(1, None), None) for p in parts]
    assert sum(v.M for v in views) == M
    s = torch.cuda.current_stream().cuda_stream
    H.check(lib.hmc_select_init(H.ptr(state), D, T, rk, M, s), "init")
    for p in range(H.SELECT_PASSES):
        total.zero_()
        for v in views:
            H.check(lib.hmc_select_count(ctypes.byref(v.c), D, T, p, H.ptr(state), H.ptr(counts), s), "count")
            total += counts
        H.check(lib.hmc_select_pick(D, T, p, H.ptr(state), H.ptr(total), s), "pick")
    H.check(lib.hmc_select_values(D, T, H.ptr(state), H.ptr(out), s), "values")
    return state.cpu().numpy(), out.cpu().numpy()


def test_shard_invariance():
    """Chains split into two shards at 16 and at 1 (what a two-rank all-reduce computes), and an empty
    third shard: state and values are bit-identical to the single run."""
    from hmc_amd.quantiles import order_stats
    N, L, D = 33, 21, 100
    x = torch.as_tensor(make_data(N, L, D), device=DEV)
    M = N * (L - 1)
    ranks = [0, M - 1, 33, 330, 330, 331, 500]
    state1, val1 = staged([x], ranks, M, D)
    assert_same_values(val1, np.sort(flat(x.cpu().numpy(), slice(1, None)), axis=0)[ranks])
    assert np.array_equal(order_stats(x, ranks).view(np.uint64), val1.view(np.uint64))
    for cut in (16, 1):
        state2, val2 = staged([x[:cut], x[cut:]], ranks, M, D)
        assert np.array_equal(state2, state1), cut
        assert np.array_equal(val2.view(np.uint64), val1.view(np.uint64)), cut
    state3, val3 = staged([x[:16], x[:0], x[16:]], ranks, M, D)
    assert np.array_equal(state3, state1) and np.array_equal(val3.view(np.uint64), val1.view(np.uint64))


def test_one_rank_process_group(tmp_path):
    """group=: the staged path with an all-reduce between count and pick, on a one-rank gloo group in
    this process; equal to the group-less call."""
    import torch.distributed as dist
    from hmc_amd.quantiles import order_stats, quantiles
    assert not dist.is_initialized()
    x = torch.as_tensor(make_data(7, 9, 16), device=DEV)
    ranks = [0, 55, 20, 20, 21]
    dist.init_process_group("gloo", init_method="file://%s" % (tmp_path / "store"), rank=0, world_size=1)
    try:
        got_s = order_stats(x, ranks, group=dist.group.WORLD)
        got_q = quantiles(x, PROBS, group=dist.group.WORLD)
    finally:
        dist.destroy_process_group()
    assert np.array_equal(got_s.view(np.uint64), order_stats(x, ranks).view(np.uint64))
    assert np.array_equal(got_q.view(np.uint64), quantiles(x, PROBS).view(np.uint64))


# ------------------------------------------------------------------------------------------ quantiles
def check_quantiles(got, x2, probs, label=""):
    """Equality with np.quantile, bit for bit (zeros by ==), wherever x_(lo), x_(lo + 1) and x_(hi) are
    finite; the module docstring says what happens elsewhere."""
    M = x2.shape[0]
    p = np.asarray(probs, dtype=np.float64)
    h = (M - 1) * p
    frac = np.abs(h - np.round(h))
    assert np.all((frac == 0) | (frac >= 1e-6)), (M, h)             # lo / hi are unambiguous
    lo, hi = np.floor(h).astype(int), np.ceil(h).astype(int)
    nxt = np.minimum(lo + 1, M - 1)
    s = np.sort(x2, axis=0)
    with np.errstate(invalid="ignore"):
        ref = np.quantile(x2, p, axis=0)
    assert got.shape == ref.shape == s[lo].shape
    ends = np.isfinite(s[lo]) & np.isfinite(s[hi])
    fin = ends & np.isfinite(s[nxt])
    assert np.isfinite(ref[fin]).all() and fin.any()
    same = (got.view(np.uint64) == ref.view(np.uint64)) | ((got == 0) & (ref == 0))
    print("%s M %d: %d of %d finite entries equal, %d entries beside an infinity" %
          (label, M, int(same[fin].sum()), int(fin.sum()), int((~fin).sum())))
    assert same[fin].all(), (label, np.argwhere(fin & ~same)[:5], got[fin & ~same][:5], ref[fin & ~same][:5])
    assert np.array_equal(np.isnan(got[~ends]), np.isnan(ref[~ends])), label


@pytest.mark.parametrize("rows", ROWS, ids=["rows1", "rows2by3"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_quantiles_match_np_quantile(shape, rows):
    from hmc_amd.quantiles import quantiles
    N, L, D = shape
    x = make_data(N, L, D)
    x2 = flat(x, rows)
    if x2.shape[0] == 0:
        with pytest.raises(AssertionError):
            quantiles(torch.as_tensor(x, device=DEV), PROBS, rows=rows)
        return
    check_quantiles(quantiles(torch.as_tensor(x, device=DEV), PROBS, rows=rows), x2, PROBS, str(shape))


# ------------------------------------------------------------------------------------------ surface
def check_sampler(h, D):
    x2 = h.q_chain[:, 1:].reshape(-1, D)
    check_quantiles(h.quantiles(), x2, (0.05, 0.5, 0.95), "sampler")
    check_quantiles(h.quantiles(PROBS), x2, PROBS, "sampler")
    lo, hi = h.credible_interval(0.9)
    assert lo.shape == hi.shape == (D,) and np.all(lo <= hi)
    tail = (1.0 - 0.9) / 2.0                                         # the interval's own probabilities
    check_quantiles(np.stack([lo, hi]), x2, (tail, 1.0 - tail), "interval")
    lo8, hi8 = h.credible_interval(0.8)
    assert np.all(lo <= lo8) and np.all(hi8 <= hi)


def test_sampler_quantiles_random_mvn():
    from hmc_amd.quantiles import quantiles
    from hmc_amd.samplers import HMC_sampler
    from hmc_amd.target import MVNTarget
    D, N, Niter = 100, 32, 20
    h = HMC_sampler(D, None, None, Nchain=N, Niter=Niter, sampler_type="Random", L_low=5, L_high=20, dt=0.1,
                    warm_up_num=0, target=MVNTarget(np.zeros(D), np.eye(D)), rng="philox", seed=4, fp_mode="fast")
    with pytest.raises(RuntimeError, match="gen_sample"):
        h.quantiles()
    with pytest.raises(RuntimeError, match="gen_sample"):
        h.credible_interval()
    h.gen_sample(np.random.RandomState(2).standard_normal((N, D)), verbose=False)
    check_sampler(h, D)
    # the energies as a D = 1 view with row_stride 1
    E = np.ascontiguousarray(h.E_chain.reshape(N, -1))
    check_quantiles(quantiles(E[..., None], PROBS), E[:, 1:].reshape(-1, 1), PROBS, "E_chain")


def test_sampler_quantiles_glm_nuts():
    """The smallest shape of tests/test_gpu_glm_nuts.py (D1: D = 1, n = 1, 5 chains, d_max 4, 12
    iterations), Philox draws."""
    import glm_cases as G
    from hmc_amd.samplers import HMC_sampler
    c = G.recipe("poisson", 1, 1, 5, 0.8, 1, pvs=1.0)
    h = HMC_sampler(1, None, None, Nchain=5, Niter=12, sampler_type="NUTS", dt=c["dt"], d_max=4,
                    target=G.glm_target(c), rng="philox", seed=5)
    with pytest.raises(RuntimeError, match="gen_sample"):
        h.quantiles()
    h.gen_sample(c["q_start"], verbose=False)
    check_sampler(h, 1)


# ------------------------------------------------------------------------------------------ ABI on the device
def test_count_of_an_empty_shard_zeroes_counts():
    """M == 0: hmc_order_stats launches nothing and leaves out alone; hmc_select_count still zeroes
    counts (an empty shard's share of the sum)."""
    from hmc_amd import _lib as H
    lib = H.lib()
    D, T = 5, 2
    x = torch.zeros((0, 4, D), dtype=torch.float64, device=DEV)
    assert x.numel() == 0 and not x.data_ptr()                      # an empty shard has no storage: q is NULL
    v = H.Samples(H.ptr(x), 0, 0, D, 1, 4, 1)
    rk = (ctypes.c_int64 * T)(0, 0)
    out = torch.full((T, D), 7.0, dtype=torch.float64, device=DEV)
    nbytes = lib.hmc_select_workspace_size(D, T)
    ws = torch.full((nbytes // 8,), 9, dtype=torch.int64, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    assert lib.hmc_order_stats(ctypes.byref(v), D, T, rk, H.ptr(out), H.ptr(ws), nbytes, s) == H.HMC_OK
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (ws == 9).all()
    state = ws[:D * T * H.SELECT_STATE_STRIDE]
    counts = ws[D * T * H.SELECT_STATE_STRIDE:]
    assert lib.hmc_select_count(ctypes.byref(v), D, T, 0, H.ptr(state), H.ptr(counts), s) == H.HMC_OK
    torch.cuda.synchronize()
    assert (counts == 0).all() and (state == 9).all()
