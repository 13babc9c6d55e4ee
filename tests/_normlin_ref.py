"""`functional.relu_batch_norm_linear` restated with torch operators, in any dtype, without the native library:
per column window, training-mode BatchNorm (biased variance, gamma = 1, beta = 0) of relu(z) times W — the fork's
`apply_bn(F.relu(.))` (reference pygcn/models.py:41-45, :49, :53) followed by the next layer's
`torch.mm(input, self.weight)` (pygcn/layers.py:33) — and the quantities its backward sweeps accumulate."""
import torch


def xhat_of(z, eps=1e-5, relu=True):
    """(xhat, rstd) of one window z [n, F]."""
    x = torch.relu(z) if relu else z
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x - mean) * rstd, rstd


def relu_batch_norm_linear(z, weight, eps=1e-5, relu=True, batch=1):
    """s [n, batch·Fout]: window j is xhat(z[:, j·Fin:(j+1)·Fin]) @ weight."""
    fin = weight.shape[0]
    assert z.shape[1] == batch * fin
    return torch.cat([xhat_of(z[:, j * fin:(j + 1) * fin], eps, relu)[0] @ weight for j in range(batch)], dim=1)


def step(z, weight, ds, dtype, eps=1e-5, relu=True, batch=1):
    """(s, dz, grad_W) as numpy arrays, evaluated in `dtype` on the CPU through autograd."""
    zz = z.detach().cpu().to(dtype).requires_grad_()
    ww = weight.detach().cpu().to(dtype).requires_grad_()
    s = relu_batch_norm_linear(zz, ww, eps, relu, batch)
    s.backward(ds.detach().cpu().to(dtype))
    return s.detach().numpy(), zz.grad.numpy(), ww.grad.numpy()


def backward_sums(z, weight, ds, eps=1e-5, relu=True):
    """What backward sweep 1 needs of ONE window, each formed two ways: (sum_r dy, sum_r dy * xhat) directly from
    dy = ds @ weight.T, and from colsum(ds) and P = xhat.T @ ds through
        sum_r dy[r][i]              = sum_j W[i][j] * colsum(ds)[j]
        sum_r dy[r][i] * xhat[r][i] = sum_j W[i][j] * P[i][j]."""
    xhat, _ = xhat_of(z, eps, relu)
    dy = ds @ weight.T
    P = xhat.T @ ds
    direct = (dy.sum(0), (dy * xhat).sum(0))
    folded = (weight @ ds.sum(0), (weight * P).sum(1))
    return direct, folded, P
