"""Target and kinetic descriptors, stated once for the engines and for HMC_sampler's row-wise calls.

Host layer (NumPy only): `host_mvn` and `host_kinetic` turn (target, cov_p, dt, dense) into the
arrays of hmc_target / hmc_kinetic (include/hmc.h), None where the kernels take NULL.  Upload layer:
`upload_mvn` / `upload_kinetic` turn those arrays into the ctypes structs plus the device tensors
that must stay alive as long as the struct is used.  `KernelTarget` is one row of the table of
targets with kernels of their own (engine.KERNEL_TARGETS)."""
import hashlib
from collections import namedtuple

import numpy as np

from . import _lib as H

# hmc_target's MVN half and hmc_kinetic as host arrays (None = NULL); dt is the scalar step
HostMVN = namedtuple("HostMVN", "kind q0 prec")
HostKinetic = namedtuple("HostKinetic", "minv p_scale dt_vec dt minv_full p_chol_t kick")


def host_cov_p(cov_p, D):
    """cov_p as the engines keep and fingerprint it: float64, identity by default (samplers.py:352-354)."""
    return np.diag(np.ones(D)) if cov_p is None else np.asarray(cov_p, dtype=np.float64)


def full_mass(cov_p):
    """Q3 with a full cov_p: any off-diagonal entry."""
    return bool(np.any(cov_p - np.diag(np.diag(cov_p))))


def host_mvn(target, cov_p=None, dense=False):
    """The MVN target arrays: a diagonal target stays diagonal (prec (D,), None for the identity)
    unless `dense` or a full cov_p asks for the dense kernels (prec (D, D)); q0 None for a zero mean."""
    diag = target.diagonal and not dense and not full_mass(host_cov_p(cov_p, target.D))
    q0 = None if target.zero_mean else target.q0
    if diag:
        return HostMVN(H.HMC_TARGET_DIAG, q0, None if target.identity else np.diag(target.prec))
    return HostMVN(H.HMC_TARGET_DENSE, q0, target.prec)


def host_kinetic(D, cov_p, dt, prec=None, chol=False):
    """The kinetic arrays of a run with momenta p ~ N(0, cov_p) and step dt (scalar, or (D,) with
    the scalar 0.0).  Identity mass: all None.  Diagonal cov_p: minv = diag(inv(cov_p)) and
    p_scale = sqrt(diag(cov_p)).  Full cov_p (samplers.py:356 inv_cov_p, :829 p = C z, :835-837 kick
    by inv_cov_p . dVdq; `prec` is the target's precision): minv_full, kick = minv_full @ prec and,
    only with `chol`, p_chol_t = cholesky(cov_p).T, which the Philox draws of the engines need and
    the row-wise leapfrog / energy calls do not."""
    cov_p = host_cov_p(cov_p, D)
    minv = p_scale = minv_full = p_chol_t = kick = None
    if full_mass(cov_p):
        minv_full = np.linalg.inv(cov_p)
        if chol:
            p_chol_t = np.linalg.cholesky(cov_p).T
        kick = minv_full @ np.asarray(prec, dtype=np.float64)
    else:
        minv_d = np.diag(np.linalg.inv(cov_p)).astype(np.float64)      # samplers.py:356
        if not (np.all(np.diag(cov_p) == 1.0) and np.all(minv_d == 1.0)):
            minv, p_scale = minv_d, np.sqrt(np.diag(cov_p))
    dt = np.asarray(dt, dtype=np.float64)
    if dt.ndim == 0:
        dt_vec, dts = None, float(dt)
    else:
        assert dt.size == D
        dt_vec, dts = dt.reshape(-1), 0.0
    return HostKinetic(minv, p_scale, dt_vec, dts, minv_full, p_chol_t, kick)


def host_descriptors(target, cov_p, dt, dense=False, chol=False):
    """(HostMVN, HostKinetic) of an MVN target."""
    return host_mvn(target, cov_p, dense), host_kinetic(target.D, cov_p, dt, target.prec, chol)


def fingerprint(arrays):
    """sha256 over the float64 bytes of `arrays` in order: a checkpoint's target_sha256."""
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------- upload layer
def dev_tensor(a, device, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64).to(device)


def _upload(arrays, device):
    return [None if a is None else dev_tensor(a, device) for a in arrays]


def upload_mvn(target, mvn, device):
    """(H.Target, device tensors to keep alive)."""
    keep = _upload((mvn.q0, mvn.prec), device)
    return H.Target(target.D, mvn.kind, H.ptr(keep[0]), H.ptr(keep[1]), target.logdet_const), keep


def upload_kinetic(kin, device):
    """(H.Kinetic, device tensors to keep alive)."""
    keep = _upload((kin.minv, kin.p_scale, kin.dt_vec, kin.minv_full, kin.p_chol_t, kin.kick), device)
    minv, p_scale, dt_vec, minv_full, p_chol_t, kick = [H.ptr(x) for x in keep]
    return H.Kinetic(minv, p_scale, dt_vec, kin.dt, minv_full, p_chol_t, kick), keep


# ---------------------------------------------------------------- targets with kernels of their own
class KernelTarget(namedtuple("KernelTarget", "name fields scalars struct head limits init iters leapfrog "
                                              "energy engine nuts_engine")):
    """One target that is not MVN and has kernels of its own.  name: how messages call it.  fields:
    the target's arrays in the order of the device descriptor; scalars: what follows them in the
    struct (attribute names both).  struct, head: the ctypes struct and the target's sizes it starts
    with.  limits: (attribute, largest value) pairs the kernels take.  init, iters, leapfrog, energy:
    the C entries.  engine, nuts_engine: the engine classes (nuts_engine None: no NUTS kernel).
    A diagonal cov_p only."""
    __slots__ = ()

    def arrays(self, t):
        return tuple(getattr(t, f) for f in self.fields)

    def fingerprint_arrays(self, t):
        """What a checkpoint fingerprints: the descriptor's arrays, then its scalars."""
        return self.arrays(t) + tuple(np.float64(getattr(t, s)) for s in self.scalars)

    def check(self, t):
        """NotImplementedError for sizes the kernels do not take."""
        if any(getattr(t, a) > most for a, most in self.limits):
            raise NotImplementedError("%s kernels: %s (%s)" % (
                self.name, ", ".join("%s=%d" % (a, getattr(t, a)) for a, _ in self.limits),
                ", ".join("%s <= %d" % lim for lim in self.limits)))

    def upload(self, t, device):
        """(device descriptor, device tensors to keep alive).  X goes as it is, row-major with
        ldx = D: the kernels clamp their reads to [n][D]."""
        keep = _upload(self.arrays(t), device)
        return self.struct(*self.head(t), *[H.ptr(x) for x in keep], *[getattr(t, s) for s in self.scalars]), keep
