#!/usr/bin/env python3
"""Generate tests/golden/g7_soft_generator.npz by IMPORTING the reference's SoftGenerator on the CPU.

Run once where the reference tree exists (PYGCN_REFERENCE, default /root/reference):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_soft_generator.py

What is executed from the reference (never copied): `models.SoftGenerator` (pygcn/models.py:412-433) with
its SoftGeneratorGCN, SoftGeneratorPoolMLP and SoftGeneratorAttention, built from a SimpleNamespace config.
The loss is the REINFORCE shape of rl-policy-generator.py:335,387: -reward * sum of log attn[picked].

The output is data only: the seed-42 state_dict, a 64-vertex row-normalised adjacency as CSR arrays,
x [64, 10] (dim_touched = 8), the reference's attn [64] and every parameter gradient.
"""
import os
import sys
import warnings
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PYGCN_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
sys.path.insert(0, HERE)
import inputs as gin  # noqa: E402

_cwd = os.getcwd()
os.chdir(os.path.join(REF, "pygcn"))          # the reference imports flat, relative to cwd
sys.path.insert(0, os.getcwd())
import models as ref_models  # noqa: E402
os.chdir(_cwd)

torch.set_num_threads(1)   # fixed summation order for a reproducible fixture

N, NFEAT_X, DIM_TOUCHED, NHID, NCLASS, NHID1, NHID2, NN = 64, 10, 8, 32, 32, 16, 16, 5
PICKED = np.array([3, 17, 42], np.int64)
REWARD = 0.7


def adjacency():
    """D^-1 (A + I) of a seeded random graph, duplicates summed: CSR float32."""
    rows, cols, vals = gin.random_coo(N, N, 400, seed=700)
    a = sp.coo_matrix((vals.astype(np.float64), (rows, cols)), shape=(N, N)).tocsr() + sp.eye(N, format="csr")
    a = sp.diags(1.0 / np.asarray(a.sum(1)).ravel()) @ a
    a = a.tocsr().astype(np.float32)
    a.sort_indices()
    return a


def main():
    config = SimpleNamespace(gcn_nfeat=DIM_TOUCHED, gcn_nhid=NHID, gcn_nclass=NCLASS, gcn_dropout=0.0, NN=NN,
                             linear_nin=NCLASS, linear_nhid1=NHID1, linear_nhid2=NHID2, linear_nout=1,
                             linear_activation="relu", linear_bias=True, dim_touched=DIM_TOUCHED,
                             replay_buffer_capacity=8)
    torch.manual_seed(42)
    model = ref_models.SoftGenerator(config)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    a = adjacency()
    coo = a.tocoo()
    adj = torch.sparse_coo_tensor(np.vstack([coo.row, coo.col]).astype(np.int64), coo.data, (N, N)).coalesce()
    x = torch.from_numpy(gin.dense((N, NFEAT_X), 701))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")       # (the reference calls F.softmax without dim)
        attn = model(x, adj)
    loss = -REWARD * torch.log(attn[torch.from_numpy(PICKED)]).sum()
    loss.backward()
    out = {"rowptr": a.indptr.astype(np.int64), "col": a.indices.astype(np.int32), "val": a.data.astype(np.float32),
           "x": x.numpy(), "dim_touched": np.int64(DIM_TOUCHED), "picked": PICKED, "reward": np.float64(REWARD),
           "dims": np.array([DIM_TOUCHED, NHID, NCLASS, NHID1, NHID2, NN], np.int64),
           "attn": attn.detach().numpy(), "loss": loss.detach().numpy()}
    for name, v in state.items():
        out["param_" + name] = v.numpy()
    for name, p in model.named_parameters():
        out["grad_" + name] = p.grad.numpy()
    path = os.path.join(HERE, "g7_soft_generator.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes; attn sum", float(attn.sum()), "loss", float(loss))


if __name__ == "__main__":
    main()
