#!/usr/bin/env python3
"""Cost of CSRGraph.t() by its three routes — the radix sort, the "pattern" share (mirror search + gather, on this
graph's rowptr / col) and the "self" share (mirror search only) — in time and in device memory, on the bench's C3
graph (`rmat_graph(10**6, 10**7)`, R-MAT seeds 42 / 43).

That graph is DIRECTED, so three matrices are measured:

    directed   the C3 graph as the bench builds it: the sort, and share_transpose() on it, which answers "sort"
               (the price of asking: one mirror search, then the sort anyway)
    row        its symmetrization max(A, A^T) (the diagonal is already there), row-normalised: sort and "pattern"
    sym        the same, D^-1/2 · D^-1/2 normalised: sort and "self"

Every measurement is a child process of its own under a timeout: the graph is built, t() runs once as a warm-up, then
`--reps` times from a dropped cache between two device events (median, min, max).  Memory: bytes allocated beyond the
graph itself at the peak of one t() (workspace included) and resident after it with the transpose's schedule built
(torch.cuda.max_memory_allocated / memory_allocated).  `--parent-tree DIR` (a built checkout of the commit before
share_transpose existed) adds the sort of that tree on the same matrices.  The first failure stops the run.

    python tools/shared_transpose_cost.py [--out profiles/shared_transpose_cost.json] [--parent-tree DIR]
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("SHARED_TRANSPOSE_COST_ROOT") or HERE        # (the child of --parent-tree imports that tree)
sys.path.insert(0, ROOT)

NODES, EDGES = 1_000_000, 10_000_000
ROUTES = (("directed", "sort"), ("directed", "share"), ("row", "sort"), ("row", "share"), ("sym", "sort"),
          ("sym", "share"))


def build(matrix, nodes, edges):
    """The matrix as a CSRGraph.  "row" uses only what the parent commit has too."""
    import torch
    from pygcn_amd import CSRGraph
    from pygcn_amd.utils import rmat_graph
    dev = torch.device("cuda:0")
    rowptr, col, val = rmat_graph(nodes, edges, seed=42, perm_seed=43, device=dev)
    g = CSRGraph(rowptr, col, val, (nodes, nodes))
    if matrix == "directed":
        return g
    r, c, _ = g.coo()
    del g, rowptr, col, val
    g = CSRGraph.from_edge_list(torch.stack([r, c], 1), nodes, device=dev, self_loops=False, normalize=False)
    return g.sym_normalize_() if matrix == "sym" else g.row_normalize_()


def run_child(matrix, route, nodes, edges, reps):
    import torch
    g = build(matrix, nodes, edges)
    word = g.share_transpose() if route == "share" else "sort"

    def drop():
        g._t = None
        if route == "share":               # (an answer of "sort" stops the asking: ask again, that is the price)
            g._share, g._share_wanted = None, True

    g.t()
    drop()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    gt = g.t()
    gt.plan()
    torch.cuda.synchronize()
    peak, resident = torch.cuda.max_memory_allocated() - base, torch.cuda.memory_allocated() - base
    shares = bool(gt.col.data_ptr() == g.col.data_ptr())
    del gt
    ts = []
    for _ in range(reps):
        drop()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record(); g.t(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"matrix": matrix, "route": route, "answer": word, "t_is_graph": g.t() is g, "t_shares_col": shares,
            "nodes": nodes, "nnz": g.nnz, "reps": reps, "device": torch.cuda.get_device_name(0),
            "median_ms": sorted(ts)[reps // 2], "min_ms": min(ts), "max_ms": max(ts), "spread_ms": max(ts) - min(ts),
            "peak_extra_MB": peak / 1e6, "resident_extra_MB": resident / 1e6, "graph_MB": base / 1e6}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="write the results as JSON")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--parent-tree", help="a built checkout of the commit before share_transpose: its sort")
    ap.add_argument("--nodes", type=int, default=NODES)
    ap.add_argument("--edges", type=int, default=EDGES)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--run", nargs=2, metavar=("MATRIX", "sort|share"), help="(child) one measurement, JSON on the last line")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps: at least 5")
    if args.run:
        print(json.dumps(run_child(args.run[0], args.run[1], args.nodes, args.edges, args.reps)))
        return 0
    jobs = [(m, r, "this", None) for m, r in ROUTES]
    if args.parent_tree:
        env = dict(os.environ, SHARED_TRANSPOSE_COST_ROOT=os.path.abspath(args.parent_tree))
        jobs += [(m, "sort", "parent", env) for m in ("directed", "row")]
    results = {"nodes": args.nodes, "edges": args.edges, "reps": args.reps, "measurements": []}
    status = 0
    for matrix, route, tree, env in jobs:
        cmd = [sys.executable, os.path.abspath(__file__), "--run", matrix, route, "--nodes", str(args.nodes),
               "--edges", str(args.edges), "--reps", str(args.reps)]
        out = child(cmd, args.timeout, f"{matrix} {route} ({tree})", env)
        if out is None:
            status = 1
            break
        r = dict(json.loads(out.strip().splitlines()[-1]), tree=tree)
        results["measurements"].append(r)
        print(f"{matrix:8s} {route:5s} {tree:6s} -> {r['answer']:7s} {r['median_ms']:8.3f} ms (min {r['min_ms']:.3f}, "
              f"max {r['max_ms']:.3f})  peak +{r['peak_extra_MB']:.1f} MB, resident +{r['resident_extra_MB']:.1f} MB, "
              f"nnz {r['nnz']}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return status


if __name__ == "__main__":
    sys.exit(main())
