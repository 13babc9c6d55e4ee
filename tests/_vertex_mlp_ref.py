"""Torch restatement of the generators' score head (reference pygcn/models.py:368-370, :391-393, the MLPs :195-241)
in any dtype — the float64 arbiter of tests/test_vertex_mlp_gpu.py and what tests/test_vertex_mlp_cpu.py holds against
the fixture g8_generators.npz.  Nothing here imports the native library.

  head(h, x, d, params, batch_norm, skip_last, masks)   scores [N, 1]
  pre_activations(h, x, d, params, batch_norm, skip_last)   (z1, z2) of the restatement's own ReLU
  unpack(bits, width, dtype)                            int64 [N] bit masks -> 0/1 [N, width]
  assert_masks_near(bits, z, what)                      the device's mask differs from (z > 0) only at the boundary
"""
import numpy as np
import torch
import torch.nn.functional as F


def _lin(params, i, t):
    return F.linear(t, params[f"linear{i}.weight"], params.get(f"linear{i}.bias"))


def _act(z, mask, batch_norm):
    """ReLU (with `mask` given: z * mask, the device's derivative convention), then the fork's fresh BatchNorm1d."""
    r = z * mask if mask is not None else F.relu(z)
    return F.batch_norm(r, None, None, None, None, True, 0.0, 1e-5) if batch_norm else r


def head(h, x, d, params, batch_norm, skip_last=0, masks=None):
    """linear3(act(linear2(act(linear1(cat(h, x[:, d : F - skip_last])))))): `params` maps linear{1,2,3}.weight /
    .bias (a bias may be missing or None) to tensors of h's dtype; `masks` = (m1 [N, H1], m2 [N, H2]) of 0/1."""
    a = torch.cat((h, x[:, d:x.shape[1] - skip_last]), dim=1)
    m1, m2 = masks if masks is not None else (None, None)
    y1 = _act(_lin(params, 1, a), m1, batch_norm)
    y2 = _act(_lin(params, 2, y1), m2, batch_norm)
    return _lin(params, 3, y2)


def pre_activations(h, x, d, params, batch_norm, skip_last=0):
    with torch.no_grad():
        a = torch.cat((h, x[:, d:x.shape[1] - skip_last]), dim=1)
        z1 = _lin(params, 1, a)
        z2 = _lin(params, 2, _act(z1, None, batch_norm))
    return z1, z2


def unpack(bits, width, dtype):
    bits = torch.as_tensor(bits, dtype=torch.int64).cpu()
    return ((bits.unsqueeze(1) >> torch.arange(width)) & 1).to(dtype)


def assert_masks_near(bits, z, what="", tol=1e-5, cap=1e-4):
    """The conditions of tests/_sampling.py::device_relu_mask: the device's mask may differ from the float64
    (z > 0) only where float64's |z| <= tol * max|z|, and on fewer than `cap` of the elements.  Returns the mask
    as z's dtype and the number of differing elements."""
    if z.shape[1] < 64:
        assert int((torch.as_tensor(bits).cpu() >> z.shape[1]).abs().max()) == 0, f"{what}: bits past the layer's width"
    mask = unpack(bits, z.shape[1], z.dtype)
    flips = (mask != 0) != (z > 0)
    if bool(flips.any()):
        assert float(z[flips].abs().max()) <= tol * float(z.abs().max()), f"{what}: masks differ away from the ReLU boundary"
    assert float(flips.double().mean()) < cap, what
    return mask, int(flips.sum())


def to_numpy(t):
    return np.asarray(t.detach().cpu().numpy())
