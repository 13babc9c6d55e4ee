#!/usr/bin/env python3
"""Time of one training step of the fork's evaluator GCN_OVER_MLP (reference pygcn/gnn-over-mlp.py:303-314:
`F.mse_loss(model(x, adj), y)`, forward + backward) in two forms on the same GPU:

    new      pygcn_amd.GCN_OVER_MLP: evaluator_ingest -> GCNBatchNorm.forward_wide -> masked_mean_pool -> MLPLayers
    parent   the same step written only with what existed before GCN_OVER_MLP did: GCNBatchNorm on x[:, :, :d],
             torch.cat with the untouched columns, the fork's pool lines (reference pygcn/models.py:351, :272,
             :279, the count read by the host as the fork reads it) and MLPLayers

on the bench's C3 graph (10^6 vertices, 10^7 sampled edges, R-MAT seeds 42 / 43) with GCN_OVER_MLP(8, 32, 32, ...),
x [k, N, F] for F = 9 and 17 (dim_touched = 8) and k = 1 and 20 (the fork's batch size), fp32.  Medians from device
events after a warm-up, with the minimum and maximum of the runs: the new form counts as "not slower" when its
median is within the parent form's own spread (max - min) of the parent's median.  The two ingest sweeps are timed
alone too, with the bytes they move per time.  Each figure runs in a child process of its own under a timeout; a
figure that fails or hangs ends the run.

    python tools/evaluator_cost.py [--out profiles/evaluator_cost.json] [--timeout 300]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NODES, EDGES, DIM_TOUCHED, WIDTH = 1_000_000, 10_000_000, 8, 32
SHAPES = [(f, k) for f in (9, 17) for k in (1, 20)]


def times(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"median_ms": sorted(ts)[reps // 2], "min_ms": min(ts), "max_ms": max(ts)}


def build(f, k, nodes, edges):
    import torch
    from pygcn_amd import CSRGraph
    from pygcn_amd.utils import rmat_graph
    dev = torch.device("cuda:0")
    rowptr, col, val = rmat_graph(nodes, edges, seed=42, perm_seed=43, device=dev)
    graph = CSRGraph(rowptr, col, val, (nodes, nodes))
    gen = torch.Generator(device=dev).manual_seed(44)
    x = torch.randn(k, nodes, f, generator=gen, device=dev)
    x[:, :, -1] = (torch.rand(k, nodes, generator=gen, device=dev) < 0.3).float()
    y = torch.randn(k, 1, generator=gen, device=dev)
    return graph, x, y


def step_fn(form, f, graph, x, y):
    import torch
    import torch.nn.functional as F
    d = DIM_TOUCHED
    nin = WIDTH + f - 1 - d
    torch.manual_seed(42)
    if form == "new":
        from pygcn_amd import GCN_OVER_MLP
        model = GCN_OVER_MLP(d, WIDTH, WIDTH, 0.5, 5, nin, 16, 8, dim_touched=d).to(x.device).train()

        def step():
            model.zero_grad(set_to_none=True)
            F.mse_loss(model(x, graph), y).backward()
        return step
    # the parent route: nothing below is newer than GCNBatchNorm's batched pass
    from pygcn_amd import GCNBatchNorm
    from pygcn_amd.models import MLPLayers
    gcn = GCNBatchNorm(d, WIDTH, WIDTH, 0.5, 5).to(x.device).train()
    mlp = MLPLayers(nin, 16, 8).to(x.device).train()

    def step():
        gcn.zero_grad(set_to_none=True)
        mlp.zero_grad(set_to_none=True)
        h = gcn(x[:, :, :d].contiguous(), graph)
        a = torch.cat((h, x[:, :, d:]), dim=2)                                               # :351
        a = (a.permute(2, 1, 0) * a[:, :, -1].T).permute(2, 1, 0)                            # :272
        pooled = torch.sum(a[:, :, :-1], axis=1) / len(torch.nonzero(a[0, :, -1], as_tuple=True)[0])     # :279
        F.mse_loss(mlp(pooled), y).backward()
    return step


def run_step(form, f, k, args):
    import torch
    graph, x, y = build(f, k, args.nodes, args.edges)
    res = times(step_fn(form, f, graph, x, y), args.reps, args.warmup)
    res.update(form=form, F=f, k=k, nodes=args.nodes, edges=args.edges, reps=args.reps, warmup=args.warmup,
               device=torch.cuda.get_device_name(0), peak_GB=torch.cuda.max_memory_allocated() / 1e9)
    return res


def run_sweeps(f, k, args):
    """The two ingest sweeps alone: x with a gradient (the flag inside x) and the flag on its own, dflag only."""
    import torch
    from pygcn_amd import evaluator as E
    n, d = args.nodes, DIM_TOUCHED
    e = f - 1 - d
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(44)
    x = torch.randn(k, n, f, generator=gen, device=dev)
    flag = (torch.rand(k, n, generator=gen, device=dev) < 0.3).float()
    x[:, :, -1] = flag
    d_wide, d_mask = torch.randn(n, k * d, generator=gen, device=dev), torch.randn(k, n, generator=gen, device=dev)
    d_esum = torch.randn(k, e, generator=gen, device=dev)
    xb, wb, mb = 4 * k * n * f, 4 * k * n * d, 4 * k * n
    rows = {"ingest": (lambda: E.ingest(x, d), xb + wb + mb),
            "ingest_backward": (lambda: E.ingest_backward(x, d, None, d_wide, d_mask, d_esum), 2 * xb + wb + mb),
            "ingest_backward_dflag_only": (lambda: E.ingest_backward(x, d, flag, None, d_mask, d_esum, False, True),
                                           (xb if e else 0) + 3 * mb)}
    out = {"F": f, "k": k, "nodes": n, "device": torch.cuda.get_device_name(0), "sweeps": {}}
    for name, (fn, nbytes) in rows.items():
        t = times(fn, args.reps, args.warmup)
        t.update(MB=nbytes / 1e6, TB_per_s=nbytes / (t["median_ms"] * 1e-3) / 1e12)
        out["sweeps"][name] = t
    return out


def child(cmd, timeout, what):
    """A fresh process per figure: its memory is gone when it ends, a hang ends with its timeout."""
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        print(f"{what}: no result within {timeout} s; stopping", file=sys.stderr)
        return None
    if out.returncode != 0:
        print(out.stderr[-4000:], file=sys.stderr)
        print(f"{what}: exit status {out.returncode}; stopping", file=sys.stderr)
        return None
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="write the results as JSON")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--nodes", type=int, default=NODES)
    ap.add_argument("--edges", type=int, default=EDGES)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--run", nargs=3, metavar=("FORM", "F", "K"),
                    help="(child) one figure (FORM: new, parent or sweeps), JSON on the last line")
    args = ap.parse_args()
    if args.run:
        form, f, k = args.run[0], int(args.run[1]), int(args.run[2])
        print(json.dumps(run_sweeps(f, k, args) if form == "sweeps" else run_step(form, f, k, args)))
        return 0
    results = {"steps": [], "verdicts": [], "sweeps": []}

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(results, fh, indent=1)

    def figure(form, f, k):
        cmd = [sys.executable, os.path.abspath(__file__), "--run", form, str(f), str(k), "--nodes", str(args.nodes),
               "--edges", str(args.edges), "--reps", str(args.reps), "--warmup", str(args.warmup)]
        return child(cmd, args.timeout, f"{form} F={f} k={k}")
    for f, k in SHAPES:
        pair = {}
        for form in ("parent", "new"):
            r = figure(form, f, k)
            save()
            if r is None:
                return 1
            pair[form] = r
            results["steps"].append(r)
            print(f"F = {f:2d}  k = {k:2d}  {form:6s} {r['median_ms']:9.3f} ms  (min {r['min_ms']:.3f}, max "
                  f"{r['max_ms']:.3f}; peak {r['peak_GB']:.1f} GB)", flush=True)
        spread = pair["parent"]["max_ms"] - pair["parent"]["min_ms"]
        verdict = {"F": f, "k": k, "new_over_parent": pair["new"]["median_ms"] / pair["parent"]["median_ms"],
                   "parent_spread_ms": spread,
                   "not_slower": pair["new"]["median_ms"] <= pair["parent"]["median_ms"] + spread}
        results["verdicts"].append(verdict)
        print(f"F = {f:2d}  k = {k:2d}  new / parent = {verdict['new_over_parent']:.3f}  (parent's spread "
              f"{spread:.3f} ms; not slower: {verdict['not_slower']})", flush=True)
        save()
    for f, k in SHAPES:
        r = figure("sweeps", f, k)
        if r is None:
            save()
            return 1
        results["sweeps"].append(r)
        print(f"F = {f:2d}  k = {k:2d}  " + "  ".join(f"{name} {t['median_ms']:.3f} ms = {t['TB_per_s']:.2f} TB/s"
                                                       for name, t in r["sweeps"].items()), flush=True)
        save()
    return 0 if all(v["not_slower"] for v in results["verdicts"]) else 2


if __name__ == "__main__":
    sys.exit(main())
