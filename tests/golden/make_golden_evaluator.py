#!/usr/bin/env python3
"""Generate tests/golden/g9_evaluator.npz by IMPORTING the reference's evaluator GCN_OVER_MLP on the CPU.

Run once where the reference tree exists (PYGCN_REFERENCE, default /root/reference):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_evaluator.py

What is executed from the reference (never copied): `models.get_model(config, 'GNN_OVER_MLP')`, i.e.
`models.GCN_OVER_MLP` (pygcn/models.py:333-355) with its GCN, PoolLayer and MLPLayers, built from a SimpleNamespace
config.  The GCN's BatchNorm line calls `.cuda()` (:41-45): `nn.Module.cuda` is patched to return `self` for the
run, so everything stays on the CPU.

The output is data only, on the 64-vertex row-normalised adjacency of g7 / g8 (stored again as CSR arrays), three
cases with dim_touched = 8:

    a_   k = 3, F = 17      b_   k = 3, F = 9      c_   k = 1, F = 17 (the parameters of a_)

x [k, 64, F] is standard normal with a Bernoulli(0.3) 0/1 flag as its last column, and requires grad.  Per case:
the seed-42 state_dict ("param_", a_ and b_ only), the output [k, 1], every parameter gradient of out.sum()
("grad_") and x.grad[:, :, -1] ("dflag").

ReLU sits in the model five times, and a pre-activation within rounding of zero would make the fixture depend on
the precision it was made in.  So the script restates the model (tests/_evaluator_ref.py) in float32 and in
float64 and REFUSES to write a fixture unless the two agree to 1e-6 normwise on the output, every parameter
gradient and the flag's gradient, and unless the float32 restatement reproduces the imported model's results
to 1e-6 as well; the seeds below pass (checked on the CPU when the fixture was made).
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import inputs as gin  # noqa: E402
from make_golden_soft_generator import adjacency, ref_models  # noqa: E402
import _evaluator_ref as R  # noqa: E402

torch.set_num_threads(1)   # fixed summation order for a reproducible fixture

N, DIM_TOUCHED, NHID, NCLASS, NHID1, NHID2, NN, SEED = 64, 8, 32, 32, 16, 8, 5, 42
CASES = (("a_", 3, 17, 941), ("b_", 3, 9, 909), ("c_", 1, 17, 929))      # tag, k, F, seed of x


def config(nfeat_x):
    return SimpleNamespace(gcn_nfeat=DIM_TOUCHED, gcn_nhid=NHID, gcn_nclass=NCLASS, gcn_dropout=0.0, NN=NN,
                           linear_nin=NCLASS + nfeat_x - 1 - DIM_TOUCHED, linear_nhid1=NHID1, linear_nhid2=NHID2,
                           linear_nout=1, linear_activation="relu", linear_bias=True, dim_touched=DIM_TOUCHED,
                           replay_buffer_capacity=8)


def features(k, nfeat_x, seed):
    x = gin.dense((k, N, nfeat_x), seed)
    x[:, :, -1] = (np.random.default_rng(seed + 1).random((k, N)) < 0.3).astype(np.float32)
    return torch.from_numpy(x)


def close(a, b, what, rel=1e-6):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err, scale = np.abs(a - b).max(), np.abs(b).max()
    assert err <= rel * scale, f"{what}: {err:.3e} > {rel:g} * {scale:.3e}"
    return err / scale if scale > 0 else 0.0


def run(k, nfeat_x, seed, adj):
    torch.manual_seed(SEED)
    model = ref_models.get_model(config(nfeat_x), "GNN_OVER_MLP")
    assert type(model).__name__ == "GCN_OVER_MLP"
    state = {name: v.detach().clone() for name, v in model.state_dict().items()}
    x = features(k, nfeat_x, seed).requires_grad_()
    out = model(x, adj)
    out.sum().backward()
    grads = {name: p.grad.clone() for name, p in model.named_parameters()}
    dflag = x.grad[:, :, -1].clone()
    # the restatement in float32 and float64: the fixture must not hinge on a rounding
    r32 = R.evaluator_step(state, x, adj, DIM_TOUCHED, torch.float32, lambda o: o.sum())
    r64 = R.evaluator_step(state, x, adj, DIM_TOUCHED, torch.float64, lambda o: o.sum())
    worst = 0.0
    for what, got, a32, a64 in ([("out", out.detach().numpy(), r32[0], r64[0]), ("dflag", dflag.numpy(), r32[2], r64[2])]
                                + [("grad " + name, grads[name].numpy(), r32[1][name], r64[1][name]) for name in grads]):
        worst = max(worst, close(a32, a64, f"float32 vs float64 restatement, {what}"),
                    close(got, a32, f"imported model vs float32 restatement, {what}"))
    return state, x.detach(), out.detach(), grads, dflag, worst


def main():
    a = adjacency()
    coo = a.tocoo()
    adj = torch.sparse_coo_tensor(np.vstack([coo.row, coo.col]).astype(np.int64), coo.data, (N, N)).coalesce()
    out = {"rowptr": a.indptr.astype(np.int64), "col": a.indices.astype(np.int32), "val": a.data.astype(np.float32),
           "dims": np.array([DIM_TOUCHED, NHID, NCLASS, NHID1, NHID2, NN], np.int64)}
    real_cuda = torch.nn.Module.cuda
    torch.nn.Module.cuda = lambda self, device=None: self
    try:
        for tag, k, nfeat_x, seed in CASES:
            state, x, y, grads, dflag, worst = run(k, nfeat_x, seed, adj)
            print(tag, "k", k, "F", nfeat_x, "out", y.view(-1).tolist(), "worst float32 / float64 gap", worst)
            out[tag + "x"], out[tag + "out"], out[tag + "dflag"] = x.numpy(), y.numpy(), dflag.numpy()
            if tag != "c_":
                for name, v in state.items():
                    out[tag + "param_" + name] = v.numpy()
            else:
                assert all(np.array_equal(v.numpy(), out["a_param_" + name]) for name, v in state.items())
            for name, g in grads.items():
                out[tag + "grad_" + name] = g.numpy()
    finally:
        torch.nn.Module.cuda = real_cuda
    path = os.path.join(HERE, "g9_evaluator.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
