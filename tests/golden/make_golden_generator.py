#!/usr/bin/env python3
"""Generate tests/golden/g8_generators.npz by IMPORTING the reference's Generator and Hierarchical_Generator on
the CPU.

Run once where the reference tree exists (PYGCN_REFERENCE, default /root/reference):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_generator.py

What is executed from the reference (never copied): `models.Generator` (pygcn/models.py:358-379) and
`models.Hierarchical_Generator` (:382-408) with their GeneratorGCN, GeneratorMLPLayers and MLPLayers, built from
a SimpleNamespace config, and `models.SoftGenerator` with the config and seed of g7_soft_generator.npz for the
log-probability of three fixed picks.  GeneratorMLPLayers' BatchNorm line calls `.cuda()` (:231):
`nn.Module.cuda` is patched to return `self` for the run, so everything stays on the CPU.  Generator's forward
prints four statistics of its scores (:371); the print is swallowed.

The output is data only: per model ("gen_" / "hier_") the seed-42 state_dict, the per-vertex scores before the
flag (captured from the model's MLPLayers), vac_flag [64, 1] and every parameter gradient of vac_flag.sum();
the shared 64-vertex row-normalised adjacency as CSR arrays and x [64, 10] (dim_touched = 8; the last column
is Hierarchical_Generator's group label, 0 = the masked group); and `g7_log_prob`, the sum of
Categorical(attn).log_prob over `g7_picked` under g7's SoftGenerator.

The script refuses a fixture whose NN-th and (NN+1)-th largest scores are closer than 1e-3 * max|score| —
100 times the parity contract — so that rounding cannot change the chosen set.
"""
import contextlib
import io
import os
import sys
import warnings
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PYGCN_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
sys.path.insert(0, HERE)
import inputs as gin  # noqa: E402
from make_golden_soft_generator import NHID1 as G7_NHID1, NHID2 as G7_NHID2, adjacency, ref_models  # noqa: E402

torch.set_num_threads(1)   # fixed summation order for a reproducible fixture

N, NFEAT_X, DIM_TOUCHED, NHID, NCLASS, NHID1, NHID2, NN, SEED = 64, 10, 8, 32, 32, 16, 8, 5, 42
G7_PICKED = np.array([3, 17, 42], np.int64)


def config(linear_nin, nhid1=NHID1, nhid2=NHID2):
    return SimpleNamespace(gcn_nfeat=DIM_TOUCHED, gcn_nhid=NHID, gcn_nclass=NCLASS, gcn_dropout=0.0, NN=NN,
                           linear_nin=linear_nin, linear_nhid1=nhid1, linear_nhid2=nhid2, linear_nout=1,
                           linear_activation="relu", linear_bias=True, dim_touched=DIM_TOUCHED,
                           replay_buffer_capacity=8)


def features():
    """x [64, 10]: eight touched columns, one untouched feature, and a group label in {0, 1, 2}."""
    x = gin.dense((N, NFEAT_X), 801)
    x[:, -1] = np.random.default_rng(802).integers(0, 3, N).astype(np.float32)
    return torch.from_numpy(x)


def run(cls, linear_nin, x, adj, hierarchical):
    torch.manual_seed(SEED)
    model = cls(config(linear_nin))
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    seen = {}
    mlp_forward = model.MLPLayers.forward          # (the models call `.forward` themselves: hooks do not fire)

    def recording(h):
        seen["mlp"] = mlp_forward(h)
        return seen["mlp"]
    model.MLPLayers.forward = recording
    with contextlib.redirect_stdout(io.StringIO()):
        vac_flag = model(x, adj)
    del model.MLPLayers.forward
    scores = seen["mlp"].detach().clone()
    if hierarchical:      # the masking lines (:395-397) on the captured output: data, recomputed with torch
        scores = torch.where(x[:, -1:] == 0, scores.min(), scores)
    top = torch.sort(scores.squeeze(1), descending=True).values
    gap, scale = float(top[NN - 1] - top[NN]), float(scores.abs().max())
    assert gap >= 1e-3 * scale, f"{cls.__name__}: the scores at ranks NN, NN+1 differ by {gap:.3e} < 1e-3 * {scale:.3e}"
    assert int((vac_flag != 0).sum()) == NN
    vac_flag.sum().backward()
    return state, scores, vac_flag.detach(), {n: p.grad.clone() for n, p in model.named_parameters()}, gap / scale


def main():
    a = adjacency()
    coo = a.tocoo()
    adj = torch.sparse_coo_tensor(np.vstack([coo.row, coo.col]).astype(np.int64), coo.data, (N, N)).coalesce()
    x = features()
    out = {"rowptr": a.indptr.astype(np.int64), "col": a.indices.astype(np.int32), "val": a.data.astype(np.float32),
           "x": x.numpy(), "dims": np.array([DIM_TOUCHED, NHID, NCLASS, NHID1, NHID2, NN], np.int64)}
    real_cuda = torch.nn.Module.cuda
    torch.nn.Module.cuda = lambda self, device=None: self
    try:
        for tag, cls, nin, hier in (("gen_", ref_models.Generator, NCLASS + NFEAT_X - DIM_TOUCHED, False),
                                    ("hier_", ref_models.Hierarchical_Generator, NCLASS + NFEAT_X - DIM_TOUCHED - 1,
                                     True)):
            state, scores, flag, grads, margin = run(cls, nin, x, adj, hier)
            print(tag, "rank margin", margin, "flag ones at", torch.nonzero(flag.squeeze(1)).squeeze(1).tolist())
            out[tag + "scores"], out[tag + "vac_flag"] = scores.numpy(), flag.numpy()
            for name, v in state.items():
                out[tag + "param_" + name] = v.numpy()
            for name, g in grads.items():
                out[tag + "grad_" + name] = g.numpy()
    finally:
        torch.nn.Module.cuda = real_cuda
    # the log-probability of three picks under g7's model (its config, its seed, its inputs)
    g7 = np.load(os.path.join(HERE, "g7_soft_generator.npz"))
    torch.manual_seed(42)
    soft = ref_models.SoftGenerator(config(NCLASS, G7_NHID1, G7_NHID2))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        attn = soft(torch.from_numpy(g7["x"]), adj)
    assert np.array_equal(attn.detach().numpy(), g7["attn"]), "this is not g7's model"
    sampler = torch.distributions.Categorical(attn.squeeze())
    total = 0
    for action in G7_PICKED.tolist():
        total = total + sampler.log_prob(torch.tensor([action]))
    out["g7_picked"], out["g7_log_prob"] = G7_PICKED, total.detach().numpy()
    path = os.path.join(HERE, "g8_generators.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes; g7 log-prob", float(total.detach()))


if __name__ == "__main__":
    main()
