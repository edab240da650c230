"""Host-side choice of the leapfrog form (no GPU): hmc_random_leapfrog_form answers what
hmc_random_iters would launch (hmc_random.hip::leapfrog_three_term)."""
import ctypes


def test_form_query_follows_the_bounds(monkeypatch):
    """hmc_random_leapfrog_form (host only): three-term inside [1e-3, 2), two-FMA outside, in EXACT
    mode, for a general diagonal target and for the lane-group kernels (D <= 64)."""
    from hmc_amd import _lib as H
    monkeypatch.setattr(H, "_lib", None)     # argtypes bound to this module's structure classes
    L = H.lib()

    def form(D, dt, fp=H.HMC_MODE_FAST, prec=None):
        T = H.Target(D, H.HMC_TARGET_DIAG, None, prec, 0.0)
        K = H.Kinetic(None, None, None, dt, None, None, None)
        S = H.Schedule(4, 0, 10, 0, 1, 11, 5, 20, 1, 11, H.HMC_RNG_PHILOX, fp, 10, 0, 0)
        return L.hmc_random_leapfrog_form(ctypes.byref(T), ctypes.byref(K), ctypes.byref(S))

    assert [form(100, dt) for dt in (0.1, 1e-3, 1.99, 9.9e-4, 2.0, 0.0)] == [1, 1, 1, 0, 0, 0]
    assert form(1000, 0.1) == 1 and form(2048, 0.1) == 1
    assert form(100, 0.1, fp=H.HMC_MODE_EXACT) == 0
    assert form(100, 0.1, prec=1) == 0          # any non-NULL diagonal: the general kernels
    assert form(64, 0.1) == 0 and form(4096, 0.1) == 0
