"""Host model of the FAST wave kernels' three-term leapfrog (hmc_wave.hip, TT) on the unit MVN.

`three_term` restates the kernel's operation order in NumPy float64 (each fused multiply-add is
evaluated in extended precision and rounded once, which is what v_fma_f64 does up to the rare
double rounding); `leapfrog_ld` is the reference's kick-drift-kick (samplers.py:831-839) in
np.longdouble.  `run_chains` runs the Random sampler's iteration loop (samplers.py:428-475, warm-up
1, thin 1) on a replay tape with either of them, so that a test can measure how far the
restatement itself sits from the long-double integration on exactly the inputs it uses.
"""
import numpy as np

LD = np.longdouble


def fma(a, b, c):
    """round(a * b + c) once: the product and sum carried in extended precision."""
    return np.asarray(LD(a) * LD(b) + LD(c), dtype=np.float64)


def three_term(q, p, dt, L):
    """L leapfrog steps from (q, p) (arrays (..., D), float64) in the kernel's order.

    Returns (traj, m1, k1): traj[l] = u[l] for l = 0..L, m1 = u[L].u[L] and
    k1 = u[L].u[L] + p[L].p[L] summed over the last axis, the latter as the kernel forms it:
    fma(sum w^2, 1/dt^2, sum u^2) with w = dt p[L] = (c/2) u[L] - u[L-1].
    """
    dt = float(dt)
    h, c = dt * 0.5, 2.0 - dt * dt
    ch, idt2 = 0.5 * c, 1.0 / (dt * dt)
    q = np.asarray(q, dtype=np.float64)
    if L <= 0:
        return [q], (q * q).sum(-1), (q * q).sum(-1) + (p * p).sum(-1)
    odd = L & 1
    t = fma(-h if odd else h, q, p)
    x = fma(-(0.0 if odd else dt), t, q)      # u[0] (odd L) or u[-1]
    u = fma(dt if odd else 0.0, t, q)         # u[1] (odd L) or u[0]
    traj = [q] + ([u] if odd else [])
    for _ in range(odd, L, 2):
        x = fma(c, u, -x)
        u = fma(c, x, -u)
        traj += [x, u]
    w = fma(ch, u, -x)
    m1 = (u * u).sum(-1)
    k1 = fma((w * w).sum(-1), idt2, m1)
    return traj, m1, k1


def leapfrog_ld(q, p, dt, L):
    """The reference's leapfrog (unit precision and mass) in long double: same return as three_term."""
    q, p, dt = LD(q), LD(p), LD(dt)
    traj = [q]
    for _ in range(max(L, 0)):
        p = p - dt * q / 2
        q = q + dt * p
        p = p - dt * q / 2
        traj.append(q)
    m1 = (q * q).sum(-1)
    return traj, m1, m1 + (p * p).sum(-1)


def run_chains(q_start, P, Ls, lnu, dt, logc, form):
    """Random sampler on a replay tape, warm-up 1, thin 1 (row i - 1 holds iteration i).

    q_start (N, D), P (N, Niter, D), Ls (N, Niter), lnu (N, Niter); form "three_term" (float64, the
    kernel's order) or "long_double".  Returns q_chain (N, Niter, D), E_chain (N, Niter),
    accept (N, Niter) bool and traj0: chain 0's trajectory points (L + 1, D) per iteration.
    """
    step, ft = (three_term, np.float64) if form == "three_term" else (leapfrog_ld, LD)
    N, Niter, D = P.shape
    q_chain = np.zeros((N, Niter, D), dtype=ft)
    E_chain = np.zeros((N, Niter), dtype=ft)
    accept = np.zeros((N, Niter), dtype=bool)
    traj0 = []
    for m in range(N):
        q = np.asarray(q_start[m], dtype=ft)
        for i in range(1, Niter + 1):
            p = np.asarray(P[m, i - 1], dtype=ft)
            e0 = (q * q).sum() + (p * p).sum()
            E_chain[m, i - 1] = 0.5 * (ft(logc) + e0)
            traj, _, k1 = step(q, p, dt, int(Ls[m, i - 1]))
            if m == 0:
                traj0.append(np.stack(traj))
            dE = 0.5 * (k1 - e0)
            accept[m, i - 1] = bool(dE < 0 or lnu[m, i - 1] < -dE)
            if accept[m, i - 1]:
                q = traj[-1]
            q_chain[m, i - 1] = q
    return dict(q_chain=q_chain, E_chain=E_chain, accept=accept, traj0=traj0)


def trajectory_deviation(dt, L, D=100, seed=0):
    """dev[l], l = 0..L: max over steps 0..l and the D coordinates of |u_three_term - u_long_double|
    on one trajectory from unit-normal q and p: the figure the host's bound on the trajectory length
    is set from (dev[l] covers every trajectory of at most l steps)."""
    rs = np.random.RandomState(seed)
    q, p = rs.standard_normal(D), rs.standard_normal(D)
    t3, _, _ = three_term(q, p, dt, L)
    tl, _, _ = leapfrog_ld(q, p, dt, L)
    return np.maximum.accumulate([float(np.max(np.abs(LD(a) - b))) for a, b in zip(t3, tl)])


def energy_deviation(dtw, L=19, D=100, n=2000, seed=0):
    """max over n draws from the stationary law of |H_three_term - H_long_double| / H after L steps
    at dt * omega = dtw (H = (q.q + p.p) / 2): the figure the host's lower bound on dt is set from."""
    rs = np.random.RandomState(seed)
    q, p = rs.standard_normal((n, D)), rs.standard_normal((n, D))
    _, _, k3 = three_term(q, p, dtw, L)
    _, _, kl = leapfrog_ld(q, p, dtw, L)
    return float(np.max(np.abs(LD(k3) - kl) / kl))
