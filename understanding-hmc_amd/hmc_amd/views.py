"""Stored samples as the device sees them: the hmc_samples view (include/hmc.h) that the predictive
and the quantile reductions read in place."""
import numpy as np

from . import _lib as H


class SamplesView:
    """samples[:, rows, :] as an hmc_samples view on the device.

    samples: an [N][L][D] float64 torch tensor or NumPy array; a device tensor is read in place, a
    non-contiguous view by its strides (the last dimension must be contiguous), never copied.  rows: a
    slice with a positive step.  device: where a host `samples` goes (default: the current device).
    min_D: the smallest D the caller takes."""

    def __init__(self, samples, rows, device, min_D=0):
        import torch
        if not isinstance(samples, torch.Tensor):
            samples = torch.as_tensor(np.asarray(samples, dtype=np.float64))
        if samples.dim() != 3:
            raise AssertionError("samples must be [N][L][D]")
        if samples.dtype != torch.float64:
            raise AssertionError("samples must be float64")
        if device is None:
            device = samples.device if samples.is_cuda else torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if not samples.is_cuda:
            samples = samples.to(self.device)
        N, L, D = samples.shape
        if D < min_D:
            raise AssertionError("samples must have D >= %d" % min_D)
        if D > 1 and samples.stride(2) != 1:
            raise AssertionError("samples: the last dimension must be contiguous")
        if not isinstance(rows, slice):
            raise AssertionError("rows must be a slice")
        begin, end, step = rows.indices(L)
        if step < 1:
            raise AssertionError("rows must have a positive step")
        end = max(end, begin)
        self.samples = samples                      # keeps the storage alive
        self.D = D
        self.M = N * len(range(begin, end, step))   # samples in the view
        cs = samples.stride(0) if N > 1 else 0
        rs = samples.stride(1) if L > 1 else D
        self.c = H.Samples(H.ptr(samples), N, cs, rs, begin, end, step)
