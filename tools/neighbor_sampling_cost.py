#!/usr/bin/env python3
"""What a fan-out costs and what it saves, on bench.py's C3 and C4 graphs and its share of labelled
rows (the first 140 / 2708 of the vertices), K in {5, 10, 25}:

    sampler     g.sample_neighbors(K, by=..., stream=i, rescale="sum") for the three modes (the training call: square,
                so the diagonal is looked for, and rescaled, so every value is read), and the bare uniform draw
                (keep_diagonal=False, rescale=None: no source array is read but for the kept entries), next to
                g.take_rows(all rows) — a plain copy of the same arrays — in the same rounds.  Host clock around a
                call that ends in a synchronise (both calls read their entry count).  The rate is the ALGORITHMIC
                bytes over that time: source entries x 4 B for `col` where it is read, x 4 B for `val` where it is
                read, kept entries x 8 B, both row pointers.
    field       n2, the rows layer 1 runs on, of the labelled rows with and without the fan-out.
    step        the restricted forward + backward step of the 256 -> 256 -> 256 fp32 model, dropout 1/2, with a FRESH
                uniform sample every step — sampler, rebuilt row sets and row blocks included — next to the same step
                on the full graph with its row sets cached (profiles/restricted_forward_cost.json's b_restricted).
    memory      peak allocation of one such step above what is live before it.

3 warm-up rounds, then --rounds rounds; every case runs once per round, so the cases ALTERNATE inside one process and
share clocks and machine; medians with min / max.  Writes profiles/neighbor_sampling_cost.json (--out)."""
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
from pygcn_amd import spmm as S                                 # noqa: E402
from pygcn_amd.utils import rmat_graph                          # noqa: E402

CONFIGS = {"c3": (1_000_000, 10_000_000), "c4": (10_000_000, 100_000_000)}     # bench.py's CONFIGS
FANOUTS = (5, 10, 25)
MODES = ("uniform", "weight", "strongest")
FEAT, DROPOUT, WARMUP = 256, 0.5, 3


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
            "n": len(ts)}


def peak_above_live(fn, dev):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    live = torch.cuda.memory_allocated(dev)
    out = fn()
    torch.cuda.synchronize()
    peak = int(torch.cuda.max_memory_allocated(dev) - live)
    del out
    return peak


def measure(name, rounds, dev):
    n, e = CONFIGS[name]
    rowptr, col, val = rmat_graph(n, e, seed=42, perm_seed=43, device=dev)
    g = CSRGraph(rowptr, col, val, (n, n))
    g.plan()
    deg = (g.rowptr[1:] - g.rowptr[:-1]).to(torch.int64)
    res = {"n": n, "nnz": g.nnz, "max_degree": int(deg.max()),
           "p99_degree": int(torch.quantile(deg[:: max(1, n // 1_000_000)].double(), 0.99))}
    all_rows = torch.arange(n, device=dev)
    rowptr_bytes = 2 * (n + 1) * 4

    # ---- the sampler next to take_rows over all rows
    cases = {"take_rows_all": lambda i: g.take_rows(all_rows)}
    for K in FANOUTS:
        for by in MODES:
            cases[f"K{K}_{by}"] = lambda i, K=K, by=by: g.sample_neighbors(K, by=by, seed=1, stream=i, rescale="sum")
        cases[f"K{K}_uniform_bare"] = lambda i, K=K: g.sample_neighbors(K, seed=1, stream=i, keep_diagonal=False)
    times, kept = {k: [] for k in cases}, {}
    for rnd in range(WARMUP + rounds):
        for k, fn in cases.items():
            t, out = wall_ms(lambda: fn(rnd))
            kept[k] = out.nnz
            del out
            if rnd >= WARMUP:
                times[k].append(t)
    sampler = {}
    copy_ms = statistics.median(times["take_rows_all"])
    for k, ts in times.items():
        row = summary(ts)
        row["kept_entries"] = kept[k]
        if k == "take_rows_all":
            nbytes = g.nnz * 16 + rowptr_bytes
        else:
            source = 0 if k.endswith("_bare") else 8                     # col for the diagonal, val for the sums / keys
            nbytes = g.nnz * source + kept[k] * 8 + rowptr_bytes
            row["over_take_rows"] = round(row["median_ms"] / copy_ms, 3)
        row["algorithmic_bytes"] = nbytes
        row["gb_per_s"] = round(nbytes / row["median_ms"] / 1e6, 1)
        sampler[k] = row
    res["sampler"] = sampler

    # ---- the receptive field and the step
    x = torch.randn(n, FEAT, generator=torch.Generator(device=dev).manual_seed(44), device=dev)
    labels = torch.randint(0, FEAT, (n,), device=dev, generator=torch.Generator(device=dev).manual_seed(45))
    idx = torch.arange(max(1, int(n * 140 / 2708)), device=dev)
    y = labels[idx]
    torch.manual_seed(42)
    model = GCN(FEAT, FEAT, FEAT, dropout=DROPOUT).to(dev)
    model.train()
    field = {"loss_rows": int(idx.numel()), "full_n2": fused.row_sets(g, idx).n2}
    for K in FANOUTS:
        field[f"K{K}_n2"] = fused.row_sets(g.sample_neighbors(K, seed=1, rescale="sum"), idx).n2
    field.update({k + "_over_n": round(v / n, 4) for k, v in list(field.items()) if k.endswith("n2")})
    res["field"] = field

    def step(K, i):
        graph = g if K is None else g.sample_neighbors(K, seed=1, stream=i, rescale="sum")
        model.zero_grad(set_to_none=True)
        out = model(x, graph, rows=idx, restrict_forward=True)
        torch.nn.functional.nll_loss(out, y).backward()
    steps = {"full_graph_cached_row_sets": None, **{f"K{K}_fresh_sample": K for K in FANOUTS}}
    times = {k: [] for k in steps}
    for rnd in range(WARMUP + rounds):
        for k, K in steps.items():
            t, _ = wall_ms(lambda: step(K, rnd))
            if rnd >= WARMUP:
                times[k].append(t)
    res["step"] = {k: summary(v) for k, v in times.items()}
    full = res["step"]["full_graph_cached_row_sets"]["median_ms"]
    for k in steps:
        if steps[k] is not None:
            res["step"][k]["over_full_graph"] = round(res["step"][k]["median_ms"] / full, 3)
    model.zero_grad(set_to_none=True)
    res["peak_above_live_bytes"] = {k: peak_above_live(lambda: step(K, 99), dev) for k, K in steps.items()}
    res["peak_above_live_bytes"]["one_full_height_tensor"] = n * FEAT * 4
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--configs", default="c3,c4")
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbor_sampling_cost.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "model": "GCN 256 -> 256 -> 256 fp32, dropout 0.5",
           "gemm_scheme": S.gemm_scheme(), "rounds": args.rounds, "warmup_rounds": WARMUP, "clock": "host, synchronised",
           "configs": {}}
    for name in args.configs.split(","):
        out["configs"][name] = measure(name, args.rounds, dev)
        print(name, json.dumps(out["configs"][name]), flush=True)
        torch.cuda.empty_cache()
        with open(args.out, "w") as f:          # (after every config: a later one that runs out of time loses nothing)
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
