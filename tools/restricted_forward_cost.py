#!/usr/bin/env python3
"""What the forward pass restricted to the loss rows' receptive field costs: forward + backward
step of the 256 -> 256 -> 256 fp32 model, dropout 1/2, on bench.py's C3 and C4 graphs and its share of labelled
rows (the first 140 / 2708 of the vertices), for

    (a) model(x, g, rows=idx)                          today's route: backward restricted, forward full height
    (b) model(x, g, rows=idx, restrict_forward=True)   forward restricted too
    (c), (d) the same two with fused.set_input_product_cache(True)

HIP events around each step, 3 warm-up rounds, median of --steps (>= 20) rounds, the four cases ALTERNATING
inside every round of one process (they share clocks and box).  Beside it: the per-kernel split of (b)'s forward
pass, n2 / N and the share of stored entries in the rows R2, the one-off construction of the two row blocks
through CSRGraph.take_rows next to the same blocks cut with the torch-op recipe of RowSets.__init__, and the
peak allocation above the live tensors of one step of (a) and (b).  Writes profiles/restricted_forward_cost.json
(--out)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pygcn_amd import GCN, CSRGraph, fused                      # noqa: E402
from pygcn_amd import gemm as G, spmm as S                      # noqa: E402
from pygcn_amd.utils import rmat_graph                          # noqa: E402

CONFIGS = {"c3": (1_000_000, 10_000_000), "c4": (10_000_000, 100_000_000)}     # bench.py's CONFIGS
FEAT, DROPOUT = 256, 0.5


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
            "n": len(ts)}


def torch_rows_block(graph, rows, rows2=None):
    """Rows `rows` of the graph cut with the torch-op recipe of RowSets.__init__ (repeat_interleave over int64
    temporaries); with `rows2` the columns are renumbered by searchsorted, as its at_block does."""
    dev = graph.device
    rp = graph.rowptr.to(torch.int64)
    starts, lens = rp[rows], rp[rows + 1] - rp[rows]
    total = int(lens.sum())
    idx = torch.repeat_interleave(starts - torch.cumsum(lens, 0) + lens, lens) + torch.arange(total, device=dev)
    cols = graph.col[idx]
    if rows2 is not None:
        cols = torch.searchsorted(rows2, cols.to(torch.int64)).to(torch.int32)
    out_rp = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=out_rp[1:])
    return CSRGraph(out_rp.to(torch.int32 if total < 2 ** 31 - 1 else torch.int64), cols.contiguous(),
                    graph.val[idx].contiguous(), (rows.numel(), graph.shape[1] if rows2 is None else rows2.numel()),
                    validate=False)


def measure(name, steps, dev):
    n, e = CONFIGS[name]
    rowptr, col, val = rmat_graph(n, e, seed=42, perm_seed=43, device=dev)
    g = CSRGraph(rowptr, col, val, (n, n))
    g.plan(), g.t().plan()
    x = torch.randn(n, FEAT, generator=torch.Generator(device=dev).manual_seed(44), device=dev)
    labels = torch.randint(0, FEAT, (n,), device=dev, generator=torch.Generator(device=dev).manual_seed(45))
    idx = torch.arange(max(1, int(n * 140 / 2708)), device=dev)
    y = labels[idx]
    torch.manual_seed(42)
    model = GCN(FEAT, FEAT, FEAT, dropout=DROPOUT).to(dev)
    model.train()
    rs = fused.row_sets(g, idx)
    # ---- one-off construction of Â[R2,:] and Â[R,R2]: device cut vs the torch-op recipe (host clock: both end in
    # host reads), each three times
    build = {"take_rows_ms": [], "torch_recipe_ms": []}
    for _ in range(3):
        rs._restricted = None
        build["take_rows_ms"].append(round(wall_ms(lambda: rs.restricted(g))[0], 3))
        build["torch_recipe_ms"].append(round(wall_ms(
            lambda: (torch_rows_block(g, rs.rows2), torch_rows_block(g, rs.rows_u, rs.rows2)))[0], 3))
        torch.cuda.empty_cache()
    a_rows2, a_block = rs.restricted(g)
    res = {"n": n, "nnz": g.nnz, "loss_rows": int(idx.numel()), "n2": rs.n2, "n2_over_n": round(rs.n2 / n, 4),
           "entries_in_rows_r2": a_rows2.nnz, "entries_in_rows_r2_share": round(a_rows2.nnz / g.nnz, 4),
           "block_entries": a_block.nnz, "construction": build}

    def step(restrict, cache):
        fused.set_input_product_cache(cache)
        model.zero_grad(set_to_none=True)
        out = model(x, g, rows=idx, restrict_forward=restrict)
        torch.nn.functional.nll_loss(out, y).backward()
    cases = {"a_rows": (False, False), "b_restricted": (True, False), "c_rows_cached": (False, True),
             "d_restricted_cached": (True, True)}
    times = {k: [] for k in cases}
    try:
        for rnd in range(3 + steps):
            for k, (restrict, cache) in cases.items():
                t = event_ms(lambda: step(restrict, cache))
                if rnd >= 3:
                    times[k].append(t)
        res["step"] = {k: summary(v) for k, v in times.items()}
        med = {k: res["step"][k]["median_ms"] for k in cases}
        res["ratio_b_over_a"] = round(med["b_restricted"] / med["a_rows"], 4)
        res["ratio_d_over_c"] = round(med["d_restricted_cached"] / med["c_rows_cached"], 4)
        # ---- peak allocation of one step above what is live before it
        fused.set_input_product_cache(False)
        peaks = {}
        for k in ("a_rows", "b_restricted"):
            model.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            live = torch.cuda.memory_allocated(dev)
            step(cases[k][0], False)
            torch.cuda.synchronize()
            peaks[k + "_bytes"] = int(torch.cuda.max_memory_allocated(dev) - live)
        peaks["one_full_height_tensor_bytes"] = n * FEAT * 4
        res["peak_above_live"] = peaks
    finally:
        fused.set_input_product_cache(False)
    # ---- the forward kernels of (b), one by one (same calls as fused._gcn2_forward with the row sets)
    w1, b1, w2, b2 = (t.detach() for t in (model.gc1.weight, model.gc1.bias, model.gc2.weight, model.gc2.bias))
    z = S.spmm_csr(a_rows2, x)
    h1 = G.layer_gemm(z, w1, bias=b1, relu=True)
    sup2 = G._dense_forward(h1, w2)
    split = {"spmm_rows2_x": lambda: S.spmm_csr(a_rows2, x),
             "gemm_layer1_bias_relu": lambda: G.layer_gemm(z, w1, bias=b1, relu=True),
             "dropout_rows": lambda: S.dropout_rows(h1, rs.rows2, DROPOUT, 12345),
             "gemm_layer2": lambda: G._dense_forward(h1, w2),
             "spmm_block_log_softmax": lambda: S.spmm_csr(a_block, sup2, bias=b2, log_softmax=True)}
    kernel = {}
    for k, fn in split.items():
        for _ in range(3):
            fn()
        kernel[k] = summary([event_ms(fn) for _ in range(steps)])
    fwd = sum(v["median_ms"] for v in kernel.values())
    kernel["forward_sum_ms"] = round(fwd, 4)
    kernel["backward_and_host_ms"] = round(res["step"]["b_restricted"]["median_ms"] - fwd, 4)   # (derived)
    res["split_of_b"] = kernel
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--configs", default="c3,c4")
    ap.add_argument("--steps", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "restricted_forward_cost.json"))
    args = ap.parse_args()
    if args.steps < 20:
        raise SystemExit("--steps: at least 20")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "model": "GCN 256 -> 256 -> 256 fp32, dropout 0.5",
           "gemm_scheme": S.gemm_scheme(), "steps": args.steps, "warmup_rounds": 3, "configs": {}}
    for name in args.configs.split(","):
        out["configs"][name] = measure(name, args.steps, dev)
        print(name, json.dumps(out["configs"][name]), flush=True)
        torch.cuda.empty_cache()
        with open(args.out, "w") as f:          # (after every config: a later one that runs out of time loses nothing)
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
