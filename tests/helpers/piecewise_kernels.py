"""
Builds the ``markovflow_amd.PiecewiseKernel`` that a ``(segments, change_points)`` description of
tests/helpers/piecewise_closed_forms.py stands for - TEST INFRASTRUCTURE, NOT PRODUCT CODE.
"""
import torch

import markovflow_amd as mfa

MATERN = {1: mfa.Matern12, 3: mfa.Matern32, 5: mfa.Matern52}
HO_VAR = 0.8          # the oscillator's share of a product's variance


def component_kernel(c, device="cpu", dtype=torch.float64, leaves=None):
    """One component description as a kernel.  With ``leaves`` (a list), the hyper-parameters become leaf tensors that require a
    gradient and are appended to it."""
    def hyper(v):
        x = torch.as_tensor(v, dtype=dtype, device=device)
        if leaves is not None:
            x = x.clone().requires_grad_(True)
            leaves.append(x)
        return x

    if c["order"] == 0:
        return (mfa.HarmonicOscillator(hyper(c["var"]), hyper(c["period"]), device=device, dtype=dtype) if c["osc"]
                else mfa.Constant(hyper(c["var"]), device=device, dtype=dtype))
    if not c["osc"]:
        return MATERN[c["order"]](hyper(c["ls"]), hyper(c["var"]), device=device, dtype=dtype)
    pair = [MATERN[c["order"]](hyper(c["ls"]), hyper(torch.as_tensor(c["var"], dtype=torch.float64) / HO_VAR), device=device, dtype=dtype),
            mfa.HarmonicOscillator(hyper(HO_VAR), hyper(c["period"]), device=device, dtype=dtype)]
    return mfa.Product(pair if c["osc"] == 1 else pair[::-1])


def segment_kernel(comps, device="cpu", dtype=torch.float64, leaves=None):
    parts = [component_kernel(c, device, dtype, leaves) for c in comps]
    return parts[0] if len(parts) == 1 else mfa.Sum(parts)


def build(segments, change_points, jitter=0.0, device="cpu", dtype=torch.float64, leaves=None):
    kernels = [segment_kernel(comps, device, dtype, leaves) for comps in segments]
    return mfa.PiecewiseKernel(kernels, torch.as_tensor(change_points, dtype=dtype, device=device).reshape(-1), jitter=jitter)
