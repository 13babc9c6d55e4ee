#!/usr/bin/env python3
"""Cost of `CSRGraph.from_dense` (pygcn_amd/csrc/gcn_dense.hip) and the density below which converting a dense
adjacency pays, on random symmetric non-negative [N, N] fp32 matrices (N = 8192 and 32768 by default).

  conversion   `from_dense(A)` and `from_dense(A, keep_per_row=32)` against the route there was before,
               `CSRGraph.from_torch(A.to_sparse())` (int64 COO indices, then from_coo's radix sort): host clock around
               the call, which ends in its own host read, then a device synchronise; the peak of
               torch.cuda.max_memory_allocated above what was allocated before the call (the input included in
               "before"); and the two sweeps alone between device events, as bytes of A read per second.
  crossover    forward + backward of one GraphConvolution(32, 32) on a [20, N, 32] input (the fork's k = 20):
               `from_dense(A, normalize=True)` against the same row-normalised matrix passed as a dense tensor (the
               layer's torch.mm branch), alternating, `--rounds` rounds of `--reps` device-event times each; per
               density the median and the spread (max - min) of the rounds' medians.  The crossover is where the two
               medians meet, interpolated on log(density) / log(time ratio) between the two densities that bracket it.

Every (N, density) is a child process of its own under a timeout; the first failure stops the run.  No GPU: an error.

    python tools/dense_ingest_cost.py [--out profiles/dense_ingest_cost.json] [--sizes 8192 32768]
                                      [--densities 0.01 0.1 1.0] [--crossover-densities 0.03 0.3]
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, WIDTH, KEEP = 20, 32, 32


def matrix(n, density, seed):
    """Random symmetric non-negative [n, n]: the upper triangle drawn at `density`, values in (0, 1], mirrored."""
    import torch
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(seed)
    a = torch.rand(n, n, generator=gen, device=dev).mul_(0.999).add_(0.001)
    if density < 1.0:
        a.mul_(torch.rand(n, n, generator=gen, device=dev) < density)
    a = torch.triu(a)
    return torch.maximum(a, a.t()).contiguous()


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1], "n": len(ts)}


def time_call(fn, reps, warmup=1):
    """Host clock around fn() + synchronise, and the peak memory above what was allocated before it."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts, peak = [], 0
    for _ in range(reps):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        peak = max(peak, torch.cuda.max_memory_allocated() - before)
        del out
    return dict(stats(ts), peak_above_input_GB=peak / 1e9)


def time_events(fn, reps, warmup=1):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return stats(ts)


def sweeps(a, g, reps):
    """The count and the fill launch alone, on the arrays of the finished conversion `g`."""
    import torch
    from pygcn_amd import _native
    n = a.shape[0]
    head = (a.data_ptr(), a.stride(0), n, n, _native.GCN_DENSE_NONZERO, 0.0, None, None, 0)
    row_count = torch.empty(n, dtype=torch.int32, device=a.device)
    col, val = torch.empty_like(g.col), torch.empty_like(g.val)
    out = {}
    for name, tail, extra in (("count", (row_count.data_ptr(),), 4 * n),
                              ("fill", (g.rowptr.data_ptr(), int(g.rowptr.dtype == torch.int64), col.data_ptr(),
                                        val.data_ptr()), 8 * g.nnz + 4 * n)):
        if name == "fill" and not g.nnz:
            continue
        t = time_events(lambda: _native.launch("gcn_dense_to_csr_" + name, a.device, *head, *tail), reps)
        out[name] = dict(t, matrix_bytes=4 * n * n, other_bytes=extra,
                         matrix_read_TB_per_s=4 * n * n / (t["median_ms"] * 1e-3) / 1e12)
    assert torch.equal(col, g.col) and torch.equal(val.view(torch.int32), g.val.view(torch.int32))
    return out


def layer_step(adj, n, seed):
    import torch
    from pygcn_amd.layers import GraphConvolution
    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    gc = GraphConvolution(WIDTH, WIDTH).to(dev)
    gen = torch.Generator(device=dev).manual_seed(seed + 1)
    x = torch.randn(K, n, WIDTH, generator=gen, device=dev)
    cot = torch.randn(K, n, WIDTH, generator=gen, device=dev)

    def step():
        gc.zero_grad(set_to_none=True)
        out = gc(x, adj)
        out.backward(cot)
        return out
    return gc, step


def run_child(n, density, reps, rounds, convert, crossover):
    import torch
    from pygcn_amd import CSRGraph
    assert torch.cuda.is_available(), "dense_ingest_cost needs an MI355X"
    a = matrix(n, density, 1000 + n)
    res = {"n": n, "density_asked": density, "device": torch.cuda.get_device_name(0), "reps": reps, "rounds": rounds,
           "input_GB": a.numel() * 4 / 1e9}
    g = CSRGraph.from_dense(a)
    res["nnz"], res["density"] = g.nnz, g.density
    heavy = n * n * density > 2e8          # (10^9 COO entries: fewer repeats of the routes that sort them)
    if convert:
        res["from_dense"] = time_call(lambda: CSRGraph.from_dense(a), reps)
        res["from_dense_keep32"] = time_call(lambda: CSRGraph.from_dense(a, keep_per_row=KEEP), reps)
        res["to_sparse_from_torch"] = time_call(lambda: CSRGraph.from_torch(a.to_sparse()), 2 if heavy else reps)
        res["sweeps"] = sweeps(a, g, reps)
        b = CSRGraph.from_torch(a.to_sparse())
        res["equal_to_baseline"] = bool(torch.equal(b.rowptr, g.rowptr) and torch.equal(b.col, g.col)
                                        and torch.equal(b.val, g.val))
        del b
    if crossover:
        del g
        g = CSRGraph.from_dense(a, normalize=True)
        del a
        dense = g.to_dense()
        routes = {"csr": layer_step(g, n, 5), "dense": layer_step(dense, n, 5)}
        a_out = routes["csr"][1]().detach()
        b_out = routes["dense"][1]().detach()
        res["layer_max_abs_diff_over_max_abs"] = float((a_out - b_out).abs().max() / b_out.abs().max())
        del a_out, b_out
        r = 2 if heavy else reps
        meds = {"csr": [], "dense": []}
        for _ in range(rounds):
            for name in ("csr", "dense"):
                meds[name].append(time_events(routes[name][1], r)["median_ms"])
        for name, ms in meds.items():
            res["layer_" + name] = {"median_ms": sorted(ms)[len(ms) // 2], "spread_ms": max(ms) - min(ms),
                                    "rounds_ms": ms}
        res["csr_over_dense"] = res["layer_csr"]["median_ms"] / res["layer_dense"]["median_ms"]
    return res


def crossover_of(rows):
    """Density at which csr_over_dense = 1, by interpolation in log-log between the bracketing measurements."""
    pts = sorted((r["density"], r["csr_over_dense"]) for r in rows if "csr_over_dense" in r)
    for (d0, r0), (d1, r1) in zip(pts, pts[1:]):
        if (r0 - 1) * (r1 - 1) <= 0 and r0 != r1:
            t = (0 - math.log(r0)) / (math.log(r1) - math.log(r0))
            return {"density": math.exp(math.log(d0) + t * (math.log(d1) - math.log(d0))), "between": [d0, d1],
                    "ratios": [r0, r1]}
    if pts:
        return {"density": None, "note": "csr_over_dense stays %s 1 over the measured densities"
                % ("below" if pts[0][1] < 1 else "above"), "densities": [p[0] for p in pts],
                "ratios": [p[1] for p in pts]}
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="write the results as JSON")
    ap.add_argument("--sizes", type=int, nargs="+", default=[8192, 32768])
    ap.add_argument("--densities", type=float, nargs="+", default=[0.01, 0.1, 1.0], help="conversion + crossover")
    ap.add_argument("--crossover-densities", type=float, nargs="+", default=[0.03, 0.3], help="crossover only")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--run", nargs=3, metavar=("N", "DENSITY", "both|crossover"), help="(child) one measurement")
    args = ap.parse_args()
    if args.run:
        n, density, mode = int(args.run[0]), float(args.run[1]), args.run[2]
        print(json.dumps(run_child(n, density, args.reps, args.rounds, mode == "both", True)))
        return 0
    results = {"k": K, "width": WIDTH, "keep_per_row": KEEP, "measurements": [], "crossover": {}}

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(results, f, indent=1)

    for n in args.sizes:
        todo = [(d, "both") for d in args.densities] + [(d, "crossover") for d in args.crossover_densities
                                                         if d not in args.densities]
        for density, mode in sorted(todo):
            cmd = [sys.executable, os.path.abspath(__file__), "--run", str(n), str(density), mode, "--reps",
                   str(args.reps), "--rounds", str(args.rounds)]
            what = f"N = {n} density {density}"
            try:
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            except subprocess.TimeoutExpired:
                print(f"{what}: no result within {args.timeout} s; stopping", file=sys.stderr)
                save()
                return 1
            if out.returncode != 0:
                print(out.stderr[-4000:], file=sys.stderr)
                print(f"{what}: exit status {out.returncode}; stopping", file=sys.stderr)
                save()
                return 1
            r = json.loads(out.stdout.strip().splitlines()[-1])
            results["measurements"].append(r)
            line = f"{what:28s} nnz {r['nnz']:11d}"
            if "from_dense" in r:
                line += (f"  from_dense {r['from_dense']['median_ms']:8.2f} ms  keep32 "
                         f"{r['from_dense_keep32']['median_ms']:8.2f} ms  to_sparse route "
                         f"{r['to_sparse_from_torch']['median_ms']:9.2f} ms")
            line += (f"  layer csr {r['layer_csr']['median_ms']:9.2f} ms  dense {r['layer_dense']['median_ms']:9.2f} ms"
                     f"  ratio {r['csr_over_dense']:.3f}")
            print(line, flush=True)
            save()
        results["crossover"][str(n)] = crossover_of([r for r in results["measurements"] if r["n"] == n])
        print(f"N = {n}: crossover {json.dumps(results['crossover'][str(n)])}", flush=True)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
