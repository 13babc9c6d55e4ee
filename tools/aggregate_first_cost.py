#!/usr/bin/env python3
"""Cost of `aggregate_first=True` — layer 1 as (Â·X)·W + b (functional.aggregate_linear,
pygcn_amd/csrc/gcn_agglin.hip) — against the default route of the same models, forward + backward, on the bench's
C3 graph (10^6 vertices, 10^7 sampled edges, R-MAT seeds 42 / 43), fp32, hidden width 32:

    evaluator9   GCN_OVER_MLP(8, 32, 32, ...) on x [k, N, 9]  (d = 8), F.mse_loss            (tools/evaluator_cost.py)
    evaluator17  GCN_OVER_MLP(16, 32, 32, ...) on x [k, N, 17] (d = 16), F.mse_loss
    batched      GCNBatchNorm(32, 32, 32) on x [k, N, 32], functional.masked_mean_pool, mean  (d = 32: equal bytes)
    generator    Generator(16, 32, 32, ...) on x [N, 18], flag.sum(), with fused.set_input_product_cache(True): the
                 features are constants of the run, so layer 1 has no sparse product at all after the first step

for k = 1, 8 and 20 (the generator: one sample), each with `fused_norm` off and on (not the generator, which has no
BatchNorm in its GCN).  Step time: the flag off and on alternating, `--rounds` rounds, every measurement a child
process of its own under a timeout (median of `--reps` device-event times after a warm-up; the peak of
torch.cuda.max_memory_allocated with it); per (workload, k, fused_norm, flag) the median and the spread (max - min)
of the rounds' medians, and the verdict `on_over_default`.  The flag counts as FASTER at a configuration when its
median lies below the default's by more than twice the default's own spread.  `--parent-tree DIR` (a built checkout
of the commit before the flag existed) adds the default route of that tree at k = 20 to every round.  `--profile`: one
`rocprofv3 --kernel-trace --stats` run per flag setting at the first workload and batch, bytes / time of the two
sweeps.  `--agree`: output and parameter gradients of the two routes side by side at the full size,
max|d| / max|ref| (recorded, not gated).  The first failure stops the run.

    python tools/aggregate_first_cost.py [--out profiles/aggregate_first_cost.json] [--profile] [--agree]
                                         [--parent-tree DIR] [--workloads ...] [--batches ...] [--fused-norm off on]
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
ROOT = os.environ.get("AGGREGATE_FIRST_COST_ROOT") or HERE     # (the child of --parent-tree imports that tree)
sys.path.insert(0, ROOT)

BATCHES = [20, 8, 1]
NODES, EDGES, WIDTH = 1_000_000, 10_000_000, 32
WORKLOADS = {"evaluator9": 8, "evaluator17": 16, "batched": 32, "generator": 16}     # name -> columns into layer 1
# floats per (vertex, sample) that a sweep reads + writes, given the input width d (layer 1 has no ReLU inside the
# evaluator's sweep: y is not read back)
STREAMS = {"al_forward_kernel": lambda d, relu: d + WIDTH, "al_backward_kernel": lambda d, relu: d + WIDTH * (1 + relu)}


def build(workload, k, nodes, edges, agg, fused_norm):
    """(model, step): agg None = a tree without the flag."""
    import torch
    import torch.nn.functional as F
    from pygcn_amd import GCN_OVER_MLP, CSRGraph, GCNBatchNorm, Generator, fused
    from pygcn_amd.functional import masked_mean_pool
    from pygcn_amd.utils import rmat_graph
    dev = torch.device("cuda:0")
    rowptr, col, val = rmat_graph(nodes, edges, seed=42, perm_seed=43, device=dev)
    graph = CSRGraph(rowptr, col, val, (nodes, nodes))
    flag = {} if agg is None else {"aggregate_first": agg}
    d = WORKLOADS[workload]
    torch.manual_seed(42)
    gen = torch.Generator(device=dev).manual_seed(44)
    if workload == "batched":
        model = GCNBatchNorm(WIDTH, WIDTH, WIDTH, dropout=0.5, fused_norm=fused_norm, **flag).to(dev).train()
        x = torch.randn(k, nodes, WIDTH, generator=gen, device=dev)
        mask = (torch.rand(k, nodes, generator=gen, device=dev) < 0.3).float()
        count = (mask[0] != 0).sum()

        def forward():
            return masked_mean_pool(model(x, graph), mask, count)

        def loss(out):
            return out.mean()
    elif workload == "generator":
        fused.set_input_product_cache(True)
        model = Generator(d, WIDTH, WIDTH, 0.0, 1000, WIDTH + 2, 16, 8, dim_touched=d, **flag).to(dev).train()
        features = torch.randn(nodes, d, generator=gen, device=dev)      # a constant of the run, sliced once
        tail = torch.randn(nodes, 2, generator=gen, device=dev)
        target = torch.randn(nodes, 1, generator=gen, device=dev)

        def forward():
            h = model.GCNLayer(features, graph)
            return model.MLPLayers(torch.cat((h, tail), dim=1))

        def loss(out):          # (not out.sum(): behind the head's BatchNorm its gradient is zero up to rounding)
            return F.mse_loss(out, target)
    else:
        f = d + 1
        model = GCN_OVER_MLP(d, WIDTH, WIDTH, 0.5, 5, WIDTH + f - 1 - d, 16, 8, dim_touched=d, fused_norm=fused_norm,
                             **flag).to(dev).train()
        x = torch.randn(k, nodes, f, generator=gen, device=dev)
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


def run_child(workload, k, agg, fused_norm, nodes, edges, reps, warmup):
    import torch
    _, step = build(workload, k, nodes, edges, agg, fused_norm)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record(); step(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"workload": workload, "k": k, "aggregate_first": agg, "fused_norm": fused_norm, "nodes": nodes,
            "edges": edges, "reps": reps, "warmup": warmup, "device": torch.cuda.get_device_name(0),
            "median_ms": sorted(ts)[reps // 2], "min_ms": min(ts), "max_ms": max(ts),
            "peak_GB": torch.cuda.max_memory_allocated() / 1e9}


def agree_child(workload, k, fused_norm, nodes, edges):
    """One step of each route from the same parameters: max|on - default| / max|default| of the output and of every
    parameter gradient."""
    import torch
    results = {}
    state = None
    for agg in (False, True):
        model, step = build(workload, k, nodes, edges, agg, fused_norm)
        if state is None:
            state = {name: v.detach().clone() for name, v in model.state_dict().items()}
        model.load_state_dict(state)
        out = step().detach().double()
        torch.cuda.synchronize()
        results[agg] = {"output": out, **{name: p.grad.double() for name, p in model.named_parameters()}}
        del model, step
    rel = {name: float((results[True][name] - ref).abs().max() / ref.abs().max()) for name, ref in results[False].items()}
    return {"workload": workload, "k": k, "fused_norm": fused_norm, "nodes": nodes,
            "max_abs_diff_over_max_abs_default": rel}


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


def me(args, *run, reps=None, warmup=None):
    return [sys.executable, os.path.abspath(__file__), "--run", *run, "--nodes", str(args.nodes), "--edges",
            str(args.edges), "--reps", str(reps or args.reps), "--warmup", str(warmup or args.warmup)]


def kernel_table(workload, k, agg, fused_norm, args, steps=3):
    """Per-kernel totals of one profiled run (1 warm-up + `steps` steps, all counted)."""
    with tempfile.TemporaryDirectory() as tmp:
        run = me(args, workload, str(k), "on" if agg else "off", "on" if fused_norm else "off", reps=steps, warmup=1)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "trace", "--output-format", "csv", "--"] + run
        if child(cmd, args.timeout, f"rocprofv3 {workload} aggregate_first={agg} k={k}") is None:
            return None
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            print(f"rocprofv3 {workload} aggregate_first={agg} k={k}: no kernel_stats.csv written; stopping",
                  file=sys.stderr)
            return None
        rows = list(csv.DictReader(open(found[0])))
    n_steps = steps + 1
    d = WORKLOADS[workload]
    relu = workload == "generator"
    table = []
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        name = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        row = {"kernel": name[:90], "calls_per_step": int(r["Calls"]) / n_steps,
               "ms_per_step": float(r["TotalDurationNs"]) / 1e6 / n_steps, "avg_ms": float(r["AverageNs"]) / 1e6}
        for key, floats in STREAMS.items():
            if name.startswith(key):
                row["bytes"] = args.nodes * k * floats(d, relu) * 4
                row["TB_per_s"] = row["bytes"] / (row["avg_ms"] * 1e-3) / 1e12
        table.append(row)
    return table


def summarise(steps):
    """Per (workload, k, fused_norm): median and spread of the rounds' medians for every route, and the verdict."""
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    groups = {}
    for r in steps:
        groups.setdefault((r["workload"], r["k"], r["fused_norm"]), {}).setdefault(r["route"], []).append(r)
    out = []
    for (workload, k, fused_norm), routes in groups.items():
        row = {"workload": workload, "k": k, "fused_norm": fused_norm}
        for route, rs in routes.items():
            ms = [r["median_ms"] for r in rs]
            row[route] = {"median_ms": med(ms), "spread_ms": max(ms) - min(ms), "rounds_ms": ms,
                          "peak_GB": max(r["peak_GB"] for r in rs)}
        if "default" in row and "on" in row:
            d, f = row["default"], row["on"]
            row["on_over_default"] = f["median_ms"] / d["median_ms"]
            row["on_is_faster"] = bool(f["median_ms"] < d["median_ms"] - 2 * d["spread_ms"])
            row["peak_on_over_default"] = f["peak_GB"] / d["peak_GB"]
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
    ap.add_argument("--profile", action="store_true", help="one rocprofv3 kernel-trace run per flag setting")
    ap.add_argument("--agree", action="store_true", help="output and gradients of the two routes side by side")
    ap.add_argument("--no-steps", action="store_true", help="skip the step times")
    ap.add_argument("--parent-tree", help="a built checkout of the commit before the flag: its default route at k = 20")
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS), choices=list(WORKLOADS))
    ap.add_argument("--batches", type=int, nargs="+", default=BATCHES)
    ap.add_argument("--fused-norm", nargs="+", default=["off", "on"], choices=["off", "on"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=NODES)
    ap.add_argument("--edges", type=int, default=EDGES)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--run", nargs=4, metavar=("WORKLOAD", "K", "off|on|none|agree", "FUSED_NORM"),
                    help="(child) one measurement, JSON on the last line")
    args = ap.parse_args()
    if args.run:
        workload, k, mode, fused_norm = args.run[0], int(args.run[1]), args.run[2], args.run[3] == "on"
        if mode == "agree":
            print(json.dumps(agree_child(workload, k, fused_norm, args.nodes, args.edges)))
        else:
            agg = {"off": False, "on": True, "none": None}[mode]
            print(json.dumps(run_child(workload, k, agg, fused_norm, args.nodes, args.edges, args.reps, args.warmup)))
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

    def configurations():
        for workload in args.workloads:
            for k in ([1] if workload == "generator" else args.batches):
                for fn in (["off"] if workload == "generator" else args.fused_norm):
                    yield workload, k, fn

    if not args.no_steps:
        done = {(r["workload"], r["k"], r["fused_norm"]) for r in results["steps"]}
        for workload, k, fn in configurations():
            if (workload, k, fn == "on") in done:                # (measured by an earlier call into the same file)
                results["steps"] = [r for r in results["steps"]
                                    if (r["workload"], r["k"], r["fused_norm"]) != (workload, k, fn == "on")]
            for rnd in range(args.rounds):
                routes = [("default", "off", None), ("on", "on", None)]
                if args.parent_tree and k == 20:
                    routes.append(("parent", "none", dict(os.environ, AGGREGATE_FIRST_COST_ROOT=args.parent_tree)))
                for route, mode, env in routes:
                    what = f"{workload} k={k} fused_norm={fn} {route}"
                    out = child(me(args, workload, str(k), mode, fn), args.timeout, what, env)
                    if out is None:
                        save()
                        return 1
                    r = dict(json.loads(out.strip().splitlines()[-1]), route=route, round=rnd)
                    results["steps"].append(r)
                    print(f"{workload:11s} k = {k:2d}  fused_norm {fn:3s}  round {rnd}  {route:8s} "
                          f"{r['median_ms']:9.2f} ms  (min {r['min_ms']:.2f}, max {r['max_ms']:.2f}; peak "
                          f"{r['peak_GB']:.2f} GB)", flush=True)
            save()
        results["verdict"] = summarise(results["steps"])
        for row in results["verdict"]:
            print(json.dumps({key: v for key, v in row.items() if not isinstance(v, dict)}), flush=True)
        save()
    if args.agree:
        results.setdefault("agreement", [])
        for workload in args.workloads:
            k = 1 if workload == "generator" else args.batches[0]
            out = child(me(args, workload, str(k), "agree", "off"), args.timeout, f"agreement {workload}")
            if out is None:
                save()
                return 1
            results["agreement"] = [a for a in results["agreement"] if a["workload"] != workload]
            results["agreement"].append(json.loads(out.strip().splitlines()[-1]))
            print(json.dumps(results["agreement"][-1]), flush=True)
        save()
    if args.profile:
        workload = args.workloads[0]
        k = 1 if workload == "generator" else args.batches[0]
        results.setdefault("kernels", {})
        for agg in (False, True):
            table = kernel_table(workload, k, agg, args.fused_norm[0] == "on", args)
            if table is None:
                save()
                return 1
            results["kernels"][f"{workload}_{'on' if agg else 'default'}_k{k}"] = table
            print(f"{workload}: aggregate_first = {agg}, k = {k}: kernels per step")
            for row in table[:16]:
                rate = f"  {row['TB_per_s']:5.2f} TB/s" if "TB_per_s" in row else ""
                print(f"  {row['ms_per_step']:9.3f} ms  {row['calls_per_step']:6.1f} calls  {row['kernel'][:70]}{rate}",
                      flush=True)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
