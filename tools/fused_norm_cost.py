#!/usr/bin/env python3
"""Cost of `fused_norm=True` — ReLU + BatchNorm folded into the next layer's X·W (functional.relu_batch_norm_linear,
pygcn_amd/csrc/gcn_normlin.hip) — against the default route of the same models, forward + backward, on the bench's
C3 graph (10^6 vertices, 10^7 sampled edges, R-MAT seeds 42 / 43), fp32, width 32:

    batched    GCNBatchNorm(32, 32, 32) on x [k, N, 32], functional.masked_mean_pool, mean   (tools/batched_model_cost.py)
    evaluator  GCN_OVER_MLP(8, 32, 32, ...) on x [k, N, 17], F.mse_loss                      (tools/evaluator_cost.py)

for k = 1, 8 and 20.  Step time: the flag off and on alternating, `--rounds` rounds, every measurement a child
process of its own under a timeout (median of `--reps` device-event times after a warm-up; the peak of
torch.cuda.max_memory_allocated with it); per (workload, k, flag) the median and the spread (max - min) of the rounds'
medians, and the verdict `fused_over_default`.  The flag counts as FASTER at a k when the fused median lies below the
default's by more than twice the default's own spread.  `--parent-tree DIR` (a built checkout of the commit before
the flag existed) adds the default route of that tree at k = 20 to every round.  `--profile`: one
`rocprofv3 --kernel-trace --stats` run per flag setting at k = 20 (batched), bytes / time of every new sweep.
`--agree`: output and parameter gradients of the two routes side by side at the full size, max|d| / max|ref|
(recorded, not gated).  The first failure stops the run.

    python tools/fused_norm_cost.py [--out profiles/fused_norm_cost.json] [--profile] [--agree] [--parent-tree DIR]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("FUSED_NORM_COST_ROOT") or HERE          # (the child of --parent-tree imports that tree)
sys.path.insert(0, ROOT)

BATCHES = [20, 8, 1]
NODES, EDGES, WIDTH, EVAL_F, DIM_TOUCHED = 1_000_000, 10_000_000, 32, 17, 8
# activation-sized streams ([N, k*32] reads + writes) of the sweeps that have a bytes / time figure
STREAMS = {"nl_forward_kernel": 2, "nl_bwd_sums_kernel": 2, "nl_bwd_apply_kernel": 3, "bn_stats_kernel": 1,
           "bn_apply_kernel": 2, "bn_bwd_sums_kernel": 2, "bn_bwd_apply_kernel": 3}


def build(workload, k, nodes, edges, fused):
    """(model, step): fused None = a tree without the flag."""
    import torch
    import torch.nn.functional as F
    from pygcn_amd import GCN_OVER_MLP, CSRGraph, GCNBatchNorm
    from pygcn_amd.functional import masked_mean_pool
    from pygcn_amd.utils import rmat_graph
    dev = torch.device("cuda:0")
    rowptr, col, val = rmat_graph(nodes, edges, seed=42, perm_seed=43, device=dev)
    graph = CSRGraph(rowptr, col, val, (nodes, nodes))
    flag = {} if fused is None else {"fused_norm": fused}
    torch.manual_seed(42)
    gen = torch.Generator(device=dev).manual_seed(44)
    if workload == "batched":
        model = GCNBatchNorm(WIDTH, WIDTH, WIDTH, dropout=0.5, **flag).to(dev).train()
        x = torch.randn(k, nodes, WIDTH, generator=gen, device=dev)
        mask = (torch.rand(k, nodes, generator=gen, device=dev) < 0.3).float()
        count = (mask[0] != 0).sum()

        def forward():
            return masked_mean_pool(model(x, graph), mask, count)

        def loss(out):
            return out.mean()
    else:
        model = GCN_OVER_MLP(DIM_TOUCHED, WIDTH, WIDTH, 0.5, 5, WIDTH + EVAL_F - 1 - DIM_TOUCHED, 16, 8,
                             dim_touched=DIM_TOUCHED, **flag).to(dev).train()
        x = torch.randn(k, nodes, EVAL_F, generator=gen, device=dev)
        x[:, :, -1] = (torch.rand(k, nodes, generator=gen, device=dev) < 0.3).float()
        y = torch.randn(k, 1, generator=gen, device=dev)

        def forward():
            return model(x, graph)

        def loss(out):
            return F.mse_loss(out, y)

    def step():
        model.zero_grad(set_to_none=True)
        out = forward()
        loss(out).backward()
        return out
    return model, step


def run_child(workload, k, fused, nodes, edges, reps, warmup):
    import torch
    _, step = build(workload, k, nodes, edges, fused)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record(); step(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"workload": workload, "k": k, "fused_norm": fused, "nodes": nodes, "edges": edges, "reps": reps,
            "warmup": warmup, "device": torch.cuda.get_device_name(0), "median_ms": sorted(ts)[reps // 2],
            "min_ms": min(ts), "max_ms": max(ts), "peak_GB": torch.cuda.max_memory_allocated() / 1e9}


def agree_child(workload, k, nodes, edges):
    """One step of each route from the same parameters: max|fused - default| / max|default| of the output and of
    every parameter gradient."""
    import torch
    results = {}
    state = None
    for fused in (False, True):
        model, step = build(workload, k, nodes, edges, fused)
        if state is None:
            state = {name: v.detach().clone() for name, v in model.state_dict().items()}
        model.load_state_dict(state)
        out = step().detach().double()
        torch.cuda.synchronize()
        results[fused] = {"output": out, **{name: p.grad.double() for name, p in model.named_parameters()}}
        del model, step
    rel = {name: float((results[True][name] - ref).abs().max() / ref.abs().max()) for name, ref in results[False].items()}
    return {"workload": workload, "k": k, "nodes": nodes, "max_abs_diff_over_max_abs_default": rel}


def child(cmd, timeout, what, env=None):
    """A fresh process per measurement: its memory is gone when it ends, a hang ends with its timeout."""
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    except subprocess.TimeoutExpired:
        print(f"{what}: no result within {timeout} s; stopping", file=sys.stderr)
        return None
    if out.returncode != 0:
        print(out.stderr[-4000:], file=sys.stderr)
        print(f"{what}: exit status {out.returncode}; stopping", file=sys.stderr)
        return None
    return out.stdout


def me(args, *run):
    return [sys.executable, os.path.abspath(__file__), "--run", *run, "--nodes", str(args.nodes), "--edges",
            str(args.edges), "--reps", str(args.reps), "--warmup", str(args.warmup)]


def kernel_table(fused, k, args, steps=3):
    """Per-kernel totals of one profiled run (1 warm-up + `steps` steps, all counted)."""
    with tempfile.TemporaryDirectory() as tmp:
        run = [sys.executable, os.path.abspath(__file__), "--run", "batched", str(k), "on" if fused else "off",
               "--nodes", str(args.nodes), "--edges", str(args.edges), "--reps", str(steps), "--warmup", "1"]
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "trace", "--output-format", "csv", "--"] + run
        if child(cmd, args.timeout, f"rocprofv3 fused_norm={fused} k={k}") is None:
            return None
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            print(f"rocprofv3 fused_norm={fused} k={k}: no kernel_stats.csv written; stopping", file=sys.stderr)
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
            if name.startswith(key):
                row["streams"] = streams
                row["TB_per_s"] = streams * act_bytes / (row["avg_ms"] * 1e-3) / 1e12
        table.append(row)
    return table


def summarise(steps):
    """Per (workload, k): median and spread of the rounds' medians for every route, and the verdict."""
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    groups = {}
    for r in steps:
        groups.setdefault((r["workload"], r["k"]), {}).setdefault(r["route"], []).append(r)
    out = []
    for (workload, k), routes in groups.items():
        row = {"workload": workload, "k": k}
        for route, rs in routes.items():
            ms = [r["median_ms"] for r in rs]
            row[route] = {"median_ms": med(ms), "spread_ms": max(ms) - min(ms), "rounds_ms": ms,
                          "peak_GB": max(r["peak_GB"] for r in rs)}
        if "default" in row and "fused" in row:
            d, f = row["default"], row["fused"]
            row["fused_over_default"] = f["median_ms"] / d["median_ms"]
            row["fused_is_faster"] = bool(f["median_ms"] < d["median_ms"] - 2 * d["spread_ms"])
            row["peak_fused_over_default"] = f["peak_GB"] / d["peak_GB"]
        if "default" in row and "parent" in row:
            d, p = row["default"], row["parent"]
            row["default_within_parent_spread"] = bool(abs(d["median_ms"] - p["median_ms"])
                                                       <= max(p["spread_ms"], d["spread_ms"]))
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="write the results as JSON")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--profile", action="store_true", help="one rocprofv3 kernel-trace run per flag setting at k = 20")
    ap.add_argument("--agree", action="store_true", help="output and gradients of the two routes side by side")
    ap.add_argument("--no-steps", action="store_true", help="skip the step times")
    ap.add_argument("--parent-tree", help="a built checkout of the commit before the flag: its default route at k = 20")
    ap.add_argument("--workloads", nargs="+", default=["batched", "evaluator"])
    ap.add_argument("--batches", type=int, nargs="+", default=BATCHES)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=NODES)
    ap.add_argument("--edges", type=int, default=EDGES)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--run", nargs=3, metavar=("WORKLOAD", "K", "off|on|none|agree"),
                    help="(child) one measurement, JSON on the last line")
    args = ap.parse_args()
    if args.run:
        workload, k, mode = args.run[0], int(args.run[1]), args.run[2]
        if mode == "agree":
            print(json.dumps(agree_child(workload, k, args.nodes, args.edges)))
        else:
            fused = {"off": False, "on": True, "none": None}[mode]
            print(json.dumps(run_child(workload, k, fused, args.nodes, args.edges, args.reps, args.warmup)))
        return 0
    results = {}
    if args.out and os.path.exists(args.out):
        results = json.load(open(args.out))                      # (the parts of a run may come from several calls)
    results.setdefault("steps", [])

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(results, f, indent=1)

    if not args.no_steps:
        results["steps"] = []
        for workload in args.workloads:
            for k in args.batches:
                for rnd in range(args.rounds):
                    routes = [("default", "off", None), ("fused", "on", None)]
                    if args.parent_tree and k == 20:
                        routes.append(("parent", "none", dict(os.environ, FUSED_NORM_COST_ROOT=args.parent_tree)))
                    for route, mode, env in routes:
                        out = child(me(args, workload, str(k), mode), args.timeout, f"{workload} k={k} {route}", env)
                        if out is None:
                            save()
                            return 1
                        r = dict(json.loads(out.strip().splitlines()[-1]), route=route, round=rnd)
                        results["steps"].append(r)
                        print(f"{workload:9s} k = {k:2d}  round {rnd}  {route:8s} {r['median_ms']:9.2f} ms  (min "
                              f"{r['min_ms']:.2f}, max {r['max_ms']:.2f}; peak {r['peak_GB']:.2f} GB)", flush=True)
        results["verdict"] = summarise(results["steps"])
        for row in results["verdict"]:
            print(json.dumps({key: v for key, v in row.items() if not isinstance(v, dict)}), flush=True)
        save()
    if args.agree:
        results["agreement"] = []
        for workload in args.workloads:
            out = child(me(args, workload, str(args.batches[0]), "agree"), args.timeout, f"agreement {workload}")
            if out is None:
                save()
                return 1
            results["agreement"].append(json.loads(out.strip().splitlines()[-1]))
            print(json.dumps(results["agreement"][-1]), flush=True)
        save()
    if args.profile:
        k = args.batches[0]
        results["kernels"] = {}
        for fused in (False, True):
            table = kernel_table(fused, k, args)
            if table is None:
                save()
                return 1
            results["kernels"][f"{'fused' if fused else 'default'}_k{k}"] = table
            print(f"fused_norm = {fused}, k = {k}: kernels per step")
            for row in table[:16]:
                rate = f"  {row['TB_per_s']:5.2f} TB/s" if "TB_per_s" in row else ""
                print(f"  {row['ms_per_step']:9.3f} ms  {row['calls_per_step']:6.1f} calls  {row['kernel'][:70]}{rate}",
                      flush=True)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
