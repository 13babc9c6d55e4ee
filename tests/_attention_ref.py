"""Torch restatement of the head of the fork's SoftGenerator (reference pygcn/models.py:289-329, 412-433) on
the CPU, in float32 (the reference's arithmetic) and float64 (the arbiter): what tests/test_attention_cpu.py
pins against the fixture g7_soft_generator.npz, and what tests/test_attention_gpu.py holds the HIP sweeps
against.  Nothing here imports the native library.

  head(h, key)                          softmax over the vertices of torch.mul(key, h).sum(dim=1)   :326-327
  pool_mlp(params, h)                   the key: mean over the vertices -> linear1..3               :303-312
  soft_generator(params, x, adj, d)     the whole model                                             :427-433
  reinforce_step(state, x, adj, d, picked, reward, dtype)   (attn, {name: grad}) of -reward * sum log attn[picked]
  attention_step(h, key, g, dtype)      (attn, dh, dkey) of the head alone, 2-D or [k, N, C] with key [k, C]
  recipe(n, c, scale, k=None)           the seeded inputs of the parity cases: h = relu(N(0,1)),
                                        key = scale * N(0,1), g = N(0,1) from default_rng(5), in that order
"""
import numpy as np
import torch
import torch.nn.functional as F


def head(h, key):
    if h.dim() == 3:                                       # one key per sample
        return torch.softmax(torch.mul(key.unsqueeze(1), h).sum(dim=2), dim=1)
    return torch.softmax(torch.mul(key, h).sum(dim=1), dim=0)


def pool_mlp(params, h):
    x = torch.mean(h, dim=0).unsqueeze(0)
    x = F.relu(F.linear(x, params["PoolMLP.linear1.weight"], params["PoolMLP.linear1.bias"]))
    x = F.relu(F.linear(x, params["PoolMLP.linear2.weight"], params["PoolMLP.linear2.bias"]))
    return F.linear(x, params["PoolMLP.linear3.weight"], params["PoolMLP.linear3.bias"])


def soft_generator(params, x, adj, dim_touched):
    h = x[:, :dim_touched]
    for i in (1, 2, 3):
        h = F.relu(torch.sparse.mm(adj, h @ params[f"GCN.gc{i}.weight"]) + params[f"GCN.gc{i}.bias"])
    return head(h, pool_mlp(params, h))


def reinforce_step(state, x, adj, dim_touched, picked, reward, dtype):
    params = {k: v.detach().clone().to(dtype).requires_grad_() for k, v in state.items()}
    attn = soft_generator(params, x.to(dtype), adj.to(dtype), dim_touched)
    loss = -reward * torch.log(attn[picked]).sum()
    loss.backward()
    return attn.detach().numpy(), {k: p.grad.numpy() for k, p in params.items()}


def attention_step(h, key, g, dtype):
    h = h.detach().clone().to(dtype).requires_grad_()
    key = key.detach().clone().to(dtype).requires_grad_()
    attn = head(h, key)
    attn.backward(g.to(dtype))
    return attn.detach(), h.grad, key.grad


def recipe(n, c, scale, k=None):
    rng = np.random.default_rng(5)
    lead = () if k is None else (k,)
    h = np.maximum(rng.standard_normal(lead + (n, c)), 0.0).astype(np.float32)
    key = (scale * rng.standard_normal(lead + (c,))).astype(np.float32)
    g = rng.standard_normal(lead + (n,)).astype(np.float32)
    return torch.from_numpy(h), torch.from_numpy(key), torch.from_numpy(g)


def fixture_case(g7):
    """(state, x, adj sparse CSR float32, dim_touched, picked, reward) of g7_soft_generator.npz."""
    state = {name[len("param_"):]: torch.from_numpy(g7[name]) for name in g7.files if name.startswith("param_")}
    n = g7["x"].shape[0]
    adj = torch.sparse_csr_tensor(torch.from_numpy(g7["rowptr"]), torch.from_numpy(g7["col"]).long(),
                                  torch.from_numpy(g7["val"]), (n, n))
    return (state, torch.from_numpy(g7["x"]), adj, int(g7["dim_touched"]), torch.from_numpy(g7["picked"]),
            float(g7["reward"]))
