#!/usr/bin/env python3
"""Time of the fork's evaluator up to its MLP — GCNBatchNorm on k samples over one graph, then the masked
mean pool (reference pygcn/models.py:341-353) — forward + backward, in two forms on the same GPU:

    loop     for j: model(x[j], adj), stacked, then (h * mask[..., None]).sum(1) / count   (the fork's loop)
    batched  model(x, adj) on x [k, N, F] and functional.masked_mean_pool                  (one pass)

on the bench's C3 graph (10^6 vertices, 10^7 sampled edges, R-MAT seeds 42 / 43), GCNBatchNorm(32, 32, 32)
(the fork's hidden = gcn_nclass = 32), fp32, k = 20 (its batch_size), 8 and 32; the loss is the mean over
the pooled [k, C] result.  Per k: median step time of each form (device events), and — with --profile —
per-kernel times of one `rocprofv3 --kernel-trace --stats` run of each form, with bytes / time of the
batched BatchNorm and pool sweeps.  Each measurement runs in a child process of its own under a timeout;
the first failure stops the run.

    python tools/batched_model_cost.py [--out results.json] [--profile] [--timeout 300]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCHES = [20, 8, 32]
NODES, EDGES, WIDTH = 1_000_000, 10_000_000, 32
# activation-sized streams ([N, k*F] reads + writes) of the sweeps that have a bytes / time figure
STREAMS = {"bn_stats_kernel": 1, "bn_apply_kernel": 2, "bn_bwd_sums_kernel": 2, "bn_bwd_apply_kernel": 3,
           "pool_colsum_kernel": 1, "pool_broadcast_kernel": 1}


def build(k, nodes, edges):
    import torch
    from pygcn_amd import CSRGraph, GCNBatchNorm
    from pygcn_amd.utils import rmat_graph
    dev = torch.device("cuda:0")
    rowptr, col, val = rmat_graph(nodes, edges, seed=42, perm_seed=43, device=dev)
    graph = CSRGraph(rowptr, col, val, (nodes, nodes))
    torch.manual_seed(42)
    model = GCNBatchNorm(WIDTH, WIDTH, WIDTH, dropout=0.5).to(dev).train()
    gen = torch.Generator(device=dev).manual_seed(44)
    x = torch.randn(k, nodes, WIDTH, generator=gen, device=dev)
    mask = (torch.rand(k, nodes, generator=gen, device=dev) < 0.3).float()
    return model, graph, x, mask, (mask[0] != 0).sum()


def step_fn(form, model, graph, x, mask, count):
    import torch
    from pygcn_amd.functional import masked_mean_pool

    def loop():
        model.zero_grad(set_to_none=True)
        h = torch.stack([model(x[j], graph) for j in range(x.shape[0])])
        ((h * mask[..., None]).sum(1) / count).mean().backward()

    def batched():
        model.zero_grad(set_to_none=True)
        masked_mean_pool(model(x, graph), mask, count).mean().backward()
    return {"loop": loop, "batched": batched}[form]


def run_child(form, k, nodes, edges, reps, warmup):
    import torch
    step = step_fn(form, *build(k, nodes, edges))
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record(); step(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"form": form, "k": k, "nodes": nodes, "edges": edges, "width": WIDTH, "reps": reps, "warmup": warmup,
            "device": torch.cuda.get_device_name(0), "median_ms": sorted(ts)[reps // 2], "min_ms": min(ts),
            "max_ms": max(ts), "peak_GB": torch.cuda.max_memory_allocated() / 1e9}


def child(cmd, timeout, what):
    """A fresh process per measurement: its memory is gone when it ends, a hang ends with its timeout."""
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        print(f"{what}: no result within {timeout} s; stopping", file=sys.stderr)
        return None
    if out.returncode != 0:
        print(out.stderr[-4000:], file=sys.stderr)
        print(f"{what}: exit status {out.returncode}; stopping", file=sys.stderr)
        return None
    return out.stdout


def kernel_table(form, k, args, steps=3):
    """Per-kernel totals of `steps` profiled steps (after the warm-up steps, which are profiled too and
    counted: calls and times are per (warmup + steps) steps)."""
    with tempfile.TemporaryDirectory() as tmp:
        me = [sys.executable, os.path.abspath(__file__), "--run", form, str(k), "--nodes", str(args.nodes),
              "--edges", str(args.edges), "--reps", str(steps), "--warmup", "1"]
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "trace", "--output-format", "csv", "--"] + me
        if child(cmd, args.timeout, f"rocprofv3 {form} k={k}") is None:
            return None
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            print(f"rocprofv3 {form} k={k}: no kernel_stats.csv written; stopping", file=sys.stderr)
            return None
        rows = list(csv.DictReader(open(found[0])))
    n_steps = steps + 1
    act_bytes = args.nodes * k * WIDTH * 4
    table = []
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        name = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        row = {"kernel": name[:90], "calls_per_step": int(r["Calls"]) / n_steps,
               "ms_per_step": float(r["TotalDurationNs"]) / 1e6 / n_steps, "avg_ms": float(r["AverageNs"]) / 1e6}
        for key, streams in STREAMS.items():
            if form == "batched" and name.startswith(key):
                row["streams"] = streams
                row["TB_per_s"] = streams * act_bytes / (row["avg_ms"] * 1e-3) / 1e12
        table.append(row)
    return table


def show(r):
    print(f"k = {r['k']:3d}  {r['form']:8s} {r['median_ms']:9.2f} ms  (min {r['min_ms']:.2f}, max {r['max_ms']:.2f}; "
          f"peak {r['peak_GB']:.1f} GB)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="write the results as JSON")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--profile", action="store_true", help="add one rocprofv3 kernel-trace run per form at k = 20")
    ap.add_argument("--batches", type=int, nargs="+", default=BATCHES)
    ap.add_argument("--nodes", type=int, default=NODES)
    ap.add_argument("--edges", type=int, default=EDGES)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--run", nargs=2, metavar=("FORM", "K"), help="(child) one measurement, JSON on the last line")
    args = ap.parse_args()
    if args.run:
        print(json.dumps(run_child(args.run[0], int(args.run[1]), args.nodes, args.edges, args.reps, args.warmup)))
        return 0
    results = {"steps": [], "kernels": {}}

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(results, f, indent=1)
    for k in args.batches:
        for form in ("loop", "batched"):
            out = child([sys.executable, os.path.abspath(__file__), "--run", form, str(k), "--nodes", str(args.nodes),
                         "--edges", str(args.edges), "--reps", str(args.reps), "--warmup", str(args.warmup)],
                        args.timeout, f"{form} k={k}")
            if out is None:
                save()
                return 1
            results["steps"].append(json.loads(out.strip().splitlines()[-1]))
            show(results["steps"][-1])
        a, b = results["steps"][-2:]
        print(f"k = {k:3d}  batched / loop = {b['median_ms'] / a['median_ms']:.3f}", flush=True)
    save()
    if args.profile:
        k = args.batches[0]
        for form in ("loop", "batched"):
            table = kernel_table(form, k, args)
            if table is None:
                save()
                return 1
            results["kernels"][f"{form}_k{k}"] = table
            print(f"{form}, k = {k}: kernels per step")
            for row in table[:14]:
                rate = f"  {row['TB_per_s']:5.2f} TB/s" if "TB_per_s" in row else ""
                print(f"  {row['ms_per_step']:9.3f} ms  {row['calls_per_step']:6.1f} calls  {row['kernel'][:70]}{rate}",
                      flush=True)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
