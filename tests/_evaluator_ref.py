"""The fork's evaluator restated on the CPU in a given dtype: GCN_OVER_MLP.forward (reference
pygcn/models.py:341-355) over PoolLayer.forward (:272, :279) and MLPLayers.forward (:212-217), with the
fork's live GCN as tests/test_norm_gpu.py restates it (`fork_forward`, whose ReLU can take the device's
derivative masks: `check_relu_masks` there says why and on what condition).

`params` uses the state_dict keys of GCN_OVER_MLP: GCNLayer.gc1..3.{weight,bias}, MLPLayers.linear1..3.{weight,bias}.
"""
import torch
import torch.nn.functional as F

from test_norm_gpu import fork_forward


def pool_layer(x):
    """reference pygcn/models.py:272,279: x [k, N, C + 1], the last feature the vertex flag; every sample is
    divided by the number of non-zero flags of sample 0."""
    x = (x.permute(2, 1, 0) * x[:, :, -1].T).permute(2, 1, 0)                                      # :272
    return torch.sum(x[:, :, :-1], axis=1) / len(torch.nonzero(x[0, :, -1], as_tuple=True)[0])     # :279


def mlp_layers(params, x):
    """reference pygcn/models.py:212-217."""
    x = F.relu(F.linear(x, params["MLPLayers.linear1.weight"], params.get("MLPLayers.linear1.bias")))
    x = F.relu(F.linear(x, params["MLPLayers.linear2.weight"], params.get("MLPLayers.linear2.bias")))
    return F.linear(x, params["MLPLayers.linear3.weight"], params.get("MLPLayers.linear3.bias"))


def evaluator_forward(params, x, adj, dim_touched, masks=None):
    """reference pygcn/models.py:341-355: the GCN once per sample on x[i, :, :dim_touched] (:343-349), the
    untouched columns and the flag concatenated behind its output (:351), PoolLayer (:353), MLPLayers (:354).
    `masks[i]`: the three ReLU derivative masks of sample i, or None for torch's own."""
    gcn = {name[len("GCNLayer."):]: v for name, v in params.items() if name.startswith("GCNLayer.")}
    outs = [fork_forward(gcn, x[i, :, :dim_touched], adj, None if masks is None else masks[i])[0]
            for i in range(x.shape[0])]
    all_gcn_output = torch.cat((torch.stack(outs), x[:, :, dim_touched:]), dim=2)
    return mlp_layers(params, pool_layer(all_gcn_output))


def evaluator_step(state, x, adj, dim_touched, dtype, loss_fn, masks=None, flag=None):
    """One training step in `dtype`: out = evaluator(x), loss_fn(out).backward().  Returns (out, parameter
    gradients by name, the gradient of the flag [k, N]).  `flag` [k, N]: the last column of x is replaced by it,
    as `torch.cat((data, flag), 2)` (reference pygcn/policy-generator.py:398), and the gradient is the flag's."""
    params = {name: v.detach().clone().to(dtype).requires_grad_() for name, v in state.items()}
    x = x.detach().clone().to(dtype)
    if flag is not None:
        flag = flag.detach().clone().to(dtype).requires_grad_()
        x_in = torch.cat((x[:, :, :-1], flag.unsqueeze(2)), dim=2)
    else:
        x_in = x.requires_grad_()
    out = evaluator_forward(params, x_in, adj.to(dtype), dim_touched, masks)
    loss_fn(out).backward()
    dflag = flag.grad if flag is not None else x_in.grad[:, :, -1]
    return (out.detach().numpy(), {name: p.grad.numpy() for name, p in params.items()}, dflag.numpy())
