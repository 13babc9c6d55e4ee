#!/usr/bin/env python3
"""Time of the four ReLU + BatchNorm sweeps (gcn_bn_stats / gcn_bn_apply / gcn_bn_backward_sums /
gcn_bn_backward_apply, pygcn_amd/norm.py) and of the torch composition they replace — torch.relu +
F.batch_norm in training mode, forward and backward — on the same GPU, at 10^6 x 256 and 10^7 x 256
fp32 and 5*10^7 x 128 bf16.  Per sweep: median time, bytes moved / time, and the ratio to torch's pass
of the same direction.  Each shape runs in a child process of its own under a timeout.

    python tools/bn_pass_cost.py [--out results.json] [--timeout 300]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1_000_000, 256, "float32"), (10_000_000, 256, "float32"), (50_000_000, 128, "bfloat16")]
# activation-sized streams (reads + writes of [n, F]) per sweep
STREAMS = {"stats": 1, "apply": 2, "backward_sums": 2, "backward_apply": 3}


def t_of(fn, reps=7):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[reps // 2]


def one_shape(n, nf, dtype_name):
    import torch
    import torch.nn.functional as F
    from pygcn_amd import norm
    dev = torch.device("cuda:0")
    dtype = getattr(torch, dtype_name)
    gen = torch.Generator(device=dev).manual_seed(1)
    z = torch.randn(n, nf, generator=gen, device=dev, dtype=dtype)
    g = torch.randn(n, nf, generator=gen, device=dev, dtype=dtype)
    w = torch.rand(nf, generator=gen, device=dev) + 0.5
    b = torch.randn(nf, generator=gen, device=dev)
    tensor_bytes = z.numel() * z.element_size()

    mean, _, rstd = norm.bn_stats(z)
    _, _, coef = norm.bn_backward_sums(g, z, mean)
    ms = {
        "stats": t_of(lambda: norm.bn_stats(z)),
        "apply": t_of(lambda: norm.bn_apply(z, mean, rstd, w, b)),
        "backward_sums": t_of(lambda: norm.bn_backward_sums(g, z, mean)),
        "backward_apply": t_of(lambda: norm.bn_backward_apply(g, z, coef, w)),
    }
    torch.cuda.empty_cache()

    zt, wt, bt = z.requires_grad_(), w.requires_grad_(), b.requires_grad_()
    compose = lambda: F.batch_norm(torch.relu(zt), None, None, wt, bt, True, 0.0, 1e-5)   # noqa: E731
    torch_fwd = t_of(compose)
    y = compose()
    torch_bwd = t_of(lambda: torch.autograd.grad(y, (zt, wt, bt), g, retain_graph=True))

    res = {"n": n, "F": nf, "dtype": dtype_name, "device": torch.cuda.get_device_name(0),
           "tensor_GB": tensor_bytes / 1e9, "torch_forward_ms": torch_fwd, "torch_backward_ms": torch_bwd,
           "hip_forward_ms": ms["stats"] + ms["apply"], "hip_backward_ms": ms["backward_sums"] + ms["backward_apply"],
           "sweeps": {}}
    for name, t in ms.items():
        ref = torch_bwd if name.startswith("backward") else torch_fwd
        res["sweeps"][name] = {"ms": t, "streams": STREAMS[name],
                               "TB_per_s": STREAMS[name] * tensor_bytes / (t * 1e-3) / 1e12,
                               "share_of_torch_pass": t / ref}
    res["forward_hip_over_torch"] = res["hip_forward_ms"] / torch_fwd
    res["backward_hip_over_torch"] = res["hip_backward_ms"] / torch_bwd
    return res


def show(r):
    print(f"{r['n']} x {r['F']} {r['dtype']} ({r['tensor_GB']:.2f} GB per tensor) on {r['device']}")
    for name, s in r["sweeps"].items():
        print(f"  {name:15s} {s['ms']:8.3f} ms  {s['streams']} streams  {s['TB_per_s']:5.2f} TB/s  "
              f"{s['share_of_torch_pass']:5.2f} of torch's pass")
    print(f"  forward   HIP {r['hip_forward_ms']:8.3f} ms  torch {r['torch_forward_ms']:8.3f} ms  "
          f"ratio {r['forward_hip_over_torch']:.2f}")
    print(f"  backward  HIP {r['hip_backward_ms']:8.3f} ms  torch {r['torch_backward_ms']:8.3f} ms  "
          f"ratio {r['backward_hip_over_torch']:.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="write the results as JSON")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per shape")
    ap.add_argument("--shape", nargs=3, metavar=("N", "F", "DTYPE"), help="(child) one shape, JSON on the last line")
    args = ap.parse_args()
    if args.shape:
        print(json.dumps(one_shape(int(args.shape[0]), int(args.shape[1]), args.shape[2])))
        return 0
    results = []
    for n, nf, dtype_name in SHAPES:
        # a fresh child per shape: its memory is gone when it ends, and a step that hangs ends with its timeout
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", str(n), str(nf), dtype_name],
                                 capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(f"{n} x {nf} {dtype_name}: no result within {args.timeout} s; stopping", file=sys.stderr)
            return 1
        if out.returncode != 0:
            print(out.stderr, file=sys.stderr)
            print(f"{n} x {nf} {dtype_name}: exit status {out.returncode}; stopping", file=sys.stderr)
            return 1
        results.append(json.loads(out.stdout.strip().splitlines()[-1]))
        show(results[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
