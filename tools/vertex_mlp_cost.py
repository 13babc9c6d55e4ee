#!/usr/bin/env python3
"""Time and peak memory of the generators' score head as fused sweeps (functional.vertex_mlp over gcn_vmlp_forward
/ gcn_vmlp_backward, pygcn_amd/csrc/gcn_head.hip) beside the torch route on the same tensors — what
`Generator.scores` runs without `fused_head`: the [N, C + T] concatenation, three Linear layers, two
relu_batch_norm nodes (or two ReLUs):

    N = 10^6 and 10^7, C = 32, H1 = H2 = 32, T = 1 and 9, batch_norm on and off
    forward, and forward + backward of (scores * ds).sum() with a dense ds

Both routes run in the same process, alternating call by call; device events, the median of 7 after 2 warm-up
calls, min and max kept.  The verdict per shape is `not_slower`: the fused forward + backward median is within
the torch route's own spread (max - min) of the torch route's median.  `torch.cuda.max_memory_allocated` above the
live bytes is recorded for both.  Per sweep: the algorithmic bytes and FLOPs from the shapes, the kernel's time
(torch.profiler, the mean of 3 calls; null when the profiler gives no device times), the time either bound alone
would take (HBM at the 6.29 TB/s a float4 copy reaches, the fp32 vector peak of 157.3 TFLOP/s) and which is nearer.
Each shape runs in a child process of its own under a timeout; a shape that fails or hangs ends the run.

    python tools/vertex_mlp_cost.py [--out profiles/vertex_mlp_cost.json] [--timeout 300]
"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, H1, H2, D = 32, 32, 32, 8
SHAPES = [(n, t, bn) for n in (1_000_000, 10_000_000) for t in (1, 9) for bn in (1, 0)]
HBM_BYTES_PER_S, FP32_FLOP_PER_S = 6.29e12, 157.3e12
SWEEP_OF_MODE = {0: "forward", 1: "forward 1: statistics of layer 1", 2: "forward 2: statistics of layer 2",
                 3: "forward 3: score", 10: "backward", 11: "backward 1: sums, grad W3",
                 12: "backward 2: grad W2", 13: "backward 3: grad W1, dh"}


def sweeps(n, t, bn):
    """{mode: (algorithmic bytes, FLOPs)} of the sweeps of one forward + backward, from the shapes."""
    k = C + t
    l1, l2, l3 = k * H1, H1 * H2, H2
    fw = {1: (k, l1), 2: (k, l1 + l2), 3: (k + 1, l1 + l2 + l3)} if bn else {0: (k + 1, l1 + l2 + l3)}
    bw = ({11: (k + 1, l1 + l2 + l3), 12: (k + 1, l1 + 2 * l2), 13: (k + 1 + C, 2 * l1 + 2 * l2 + C * H1)} if bn
          else {10: (k + 1 + C, 2 * l1 + 3 * l2 + l3 + C * H1)})
    return {m: (4 * n * words, 2 * n * fma) for m, (words, fma) in {**fw, **bw}.items()}


def alternate(fused, torch_route, reps=7, warm=2):
    """Both callables timed in turn with device events: {route: {median_ms, min_ms, max_ms}}."""
    import torch
    ts = {"fused": [], "torch": []}
    for i in range(warm + reps):
        for name, fn in (("fused", fused), ("torch", torch_route)):
            e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            if i >= warm:
                ts[name].append(e0.elapsed_time(e1))
    return {name: {"median_ms": sorted(v)[len(v) // 2], "min_ms": min(v), "max_ms": max(v)} for name, v in ts.items()}


def peak_of(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def kernel_times(fn, calls=3):
    """{mode: mean ms per call} of the vmlp sweep kernels under torch.profiler, or None."""
    try:
        import torch
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            m = re.search(r"vmlp_(fwd|bwd)_kernel<\s*\d+,\s*(\d+)", ev.key)
            us = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0)
            if m and us:
                out[int(m.group(2))] = out.get(int(m.group(2)), 0.0) + us / 1e3 / calls
        return out or None
    except Exception as e:                                       # noqa: BLE001  (the times are then "not measured")
        print(f"profiler: {e}", file=sys.stderr)
        return None


def one_shape(n, t, bn):
    import torch
    from pygcn_amd import _native
    from pygcn_amd.functional import vertex_mlp
    from pygcn_amd.models import GeneratorMLPLayers, MLPLayers
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    mlp = (GeneratorMLPLayers if bn else MLPLayers)(C + t, H1, H2, 1).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    h = torch.relu(torch.randn(n, C, generator=gen, device=dev)).requires_grad_()
    x = torch.randn(n, D + t, generator=gen, device=dev)
    ds = torch.randn(n, 1, generator=gen, device=dev)

    fused_fw = lambda: vertex_mlp(h, x, D, mlp, bool(bn))                       # noqa: E731
    torch_fw = lambda: mlp(torch.cat((h, x[:, D:]), dim=1))                     # noqa: E731

    def step(forward):
        h.grad = None
        mlp.zero_grad(set_to_none=True)
        (forward() * ds).sum().backward()
    res = {"n": n, "C": C, "T": t, "H1": H1, "H2": H2, "batch_norm": bool(bn),
           "device": torch.cuda.get_device_name(0), "activation_MB": 4e-6 * n * H1,
           "workspace_bytes": _native.lib().gcn_vmlp_workspace_bytes(n, C, t, H1, H2)}
    with torch.no_grad():
        res["forward_ms"] = alternate(fused_fw, torch_fw)
    res["forward_backward_ms"] = alternate(lambda: step(fused_fw), lambda: step(torch_fw))
    res["peak_bytes"] = {"fused": peak_of(lambda: step(fused_fw)), "torch": peak_of(lambda: step(torch_fw))}
    times = kernel_times(lambda: step(fused_fw))
    res["sweeps"] = []
    for mode, (nbytes, flops) in sweeps(n, t, bn).items():
        mem_ms, alu_ms = 1e3 * nbytes / HBM_BYTES_PER_S, 1e3 * flops / FP32_FLOP_PER_S
        ms = times.get(mode) if times else None
        res["sweeps"].append({"sweep": SWEEP_OF_MODE[mode], "bytes": nbytes, "flop": flops, "ms": ms,
                              "memory_bound_ms": mem_ms, "fp32_bound_ms": alu_ms,
                              "nearer_bound": "fp32 arithmetic" if alu_ms > mem_ms else "memory",
                              "ms_over_nearer_bound": ms / max(mem_ms, alu_ms) if ms else None})
    fb = res["forward_backward_ms"]
    spread = fb["torch"]["max_ms"] - fb["torch"]["min_ms"]
    res["verdict"] = {"fused_over_torch": fb["fused"]["median_ms"] / fb["torch"]["median_ms"],
                      "torch_spread_ms": spread,
                      "not_slower": fb["fused"]["median_ms"] <= fb["torch"]["median_ms"] + spread}
    return res


def show(r):
    f, fb, v = r["forward_ms"], r["forward_backward_ms"], r["verdict"]
    print(f"N = {r['n']}, T = {r['T']}, batch_norm = {r['batch_norm']} on {r['device']}")
    print(f"  forward            fused {f['fused']['median_ms']:.3f} ms   torch {f['torch']['median_ms']:.3f} ms")
    print(f"  forward + backward fused {fb['fused']['median_ms']:.3f} ms   torch {fb['torch']['median_ms']:.3f} ms "
          f"(spread {v['torch_spread_ms']:.3f})   fused / torch = {v['fused_over_torch']:.3f}   "
          f"not slower: {v['not_slower']}")
    print(f"  peak bytes         fused {r['peak_bytes']['fused'] / 1e6:.1f} MB   torch {r['peak_bytes']['torch'] / 1e6:.1f} MB")
    for s in r["sweeps"]:
        ms = f"{s['ms']:.3f} ms" if s["ms"] else "not measured"
        print(f"    {s['sweep']:34s} {ms:>12s}   {s['bytes'] / 1e6:8.1f} MB  {s['flop'] / 1e9:7.2f} GFLOP   nearer bound: "
              f"{s['nearer_bound']} ({max(s['memory_bound_ms'], s['fp32_bound_ms']):.3f} ms)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="write the results as JSON")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per shape")
    ap.add_argument("--shape", nargs=3, metavar=("N", "T", "BN"), help="(child) one shape, JSON on the last line")
    args = ap.parse_args()
    if args.shape:
        print(json.dumps(one_shape(*(int(v) for v in args.shape))))
        return 0
    results = []
    for n, t, bn in SHAPES:
        # a fresh child per shape: its memory is gone when it ends, and a step that hangs ends with its timeout
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", str(n), str(t), str(bn)],
                                 capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(f"N = {n}, T = {t}, batch_norm = {bn}: no result within {args.timeout} s; stopping", file=sys.stderr)
            return 1
        if out.returncode != 0:
            print(out.stderr, file=sys.stderr)
            print(f"N = {n}, T = {t}, batch_norm = {bn}: exit status {out.returncode}; stopping", file=sys.stderr)
            return 1
        results.append(json.loads(out.stdout.strip().splitlines()[-1]))
        show(results[-1])
        if args.out:                  # (after every shape: a later one that fails keeps the earlier results)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(results, f, indent=1)
    accepted = [r["verdict"]["not_slower"] for r in results if r["n"] == 1_000_000]
    return 0 if all(accepted) else 2


if __name__ == "__main__":
    sys.exit(main())
