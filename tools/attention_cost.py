#!/usr/bin/env python3
"""Time of the vertex-attention sweeps (gcn_attn_scores / gcn_attn_normalize / gcn_attn_backward,
pygcn_amd/attention.py) and of the autograd node around them, beside two torch forms of the same head on the
same tensors:

    literal   softmax(torch.mul(key, x).sum(1), 0)      the fork's lines, reference pygcn/models.py:326-327
    mv        softmax(torch.mv(x, key), 0)              the best plain torch form (bmm for the batched shape)

at 10^6 x 32 (the fork's width), 10^6 x 256 and 10^7 x 256 fp32, and 10^6 x (20 x 32) batched.  Per sweep:
median time and h-sized bytes moved / time; per form: forward and backward (gradients to h and key) medians
from device events after a warm-up.  Each shape runs in a child process of its own under a timeout; a shape
that fails or hangs ends the run.

    python tools/attention_cost.py [--out profiles/attention_cost.json] [--timeout 300]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1_000_000, 32, 1), (1_000_000, 256, 1), (10_000_000, 256, 1), (1_000_000, 32, 20)]
# h-sized streams (reads + writes of [n, k*C]) per sweep; the [k, n] vectors are 1/C of one
STREAMS = {"scores": 1, "normalize": 0, "backward": 2, "backward_without_dh": 1}


def t_of(fn, reps=9):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[reps // 2]


def one_shape(n, c, k):
    import torch
    from pygcn_amd import attention as A
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    store = torch.relu(torch.randn(n, k * c, generator=gen, device=dev))
    key = torch.randn(k, c, generator=gen, device=dev) * (2.0 / c ** 0.5)
    g = torch.randn(k, n, generator=gen, device=dev)
    h_bytes = store.numel() * store.element_size()
    h = store if k == 1 else store.view(n, k, c).permute(1, 0, 2)
    key_in = key[0] if k == 1 else key
    g_in = g[0] if k == 1 else g

    key32 = key.contiguous().view(k * c)
    scores, stats = A.attn_scores(store, key32, n, k, c)
    attn = A.attn_normalize(scores.clone(), stats)
    ds = (attn * (g - (g * attn).sum(1, keepdim=True))).contiguous()
    ms = {
        "scores": t_of(lambda: A.attn_scores(store, key32, n, k, c)),
        "normalize": t_of(lambda: A.attn_normalize(scores, stats, out=attn)),
        "backward": t_of(lambda: A.attn_backward(store, ds, key32, n, k, c)),
        "backward_without_dh": t_of(lambda: A.attn_backward(store, ds, key32, n, k, c, need_dh=False)),
    }
    del scores, attn, ds
    torch.cuda.empty_cache()

    if k == 1:
        forms = {"hip": lambda x, q: A.vertex_attention(x, q),
                 "literal": lambda x, q: torch.softmax(torch.mul(q, x).sum(1), 0),
                 "mv": lambda x, q: torch.softmax(torch.mv(x, q), 0)}
    else:
        forms = {"hip": lambda x, q: A.vertex_attention(x, q),
                 "literal": lambda x, q: torch.softmax(torch.mul(q.unsqueeze(1), x).sum(2), 1),
                 "mv": lambda x, q: torch.softmax(torch.bmm(x, q.unsqueeze(2)).squeeze(2), 1)}
    res = {"n": n, "C": c, "batch": k, "dtype": "float32", "device": torch.cuda.get_device_name(0),
           "h_GB": h_bytes / 1e9, "sweeps": {}, "forms": {}}
    for name, t in ms.items():
        res["sweeps"][name] = {"ms": t, "h_streams": STREAMS[name],
                               "TB_per_s": STREAMS[name] * h_bytes / (t * 1e-3) / 1e12 if STREAMS[name] else None}
    want = None
    for name, form in forms.items():
        x, q = h.detach().requires_grad_(), key_in.detach().clone().requires_grad_()
        fwd = t_of(lambda: form(x, q))
        out = form(x, q)
        bwd = t_of(lambda: torch.autograd.grad(out, (x, q), g_in, retain_graph=True))
        if want is None:
            want = out.detach()
        else:                                   # the same head: faster and different is not faster
            res["forms"].setdefault("max_abs_diff_to_hip", {})[name] = float((out.detach() - want).abs().max())
        res["forms"][name] = {"forward_ms": fwd, "backward_ms": bwd, "total_ms": fwd + bwd}
        del out, x, q
        torch.cuda.empty_cache()
    res["attn_max"] = float(want.max())
    for name in ("literal", "mv"):
        res["forms"][name]["hip_over_this"] = res["forms"]["hip"]["total_ms"] / res["forms"][name]["total_ms"]
    return res


def show(r):
    print(f"{r['n']} x ({r['batch']} x {r['C']}) {r['dtype']} ({r['h_GB']:.2f} GB) on {r['device']}")
    for name, s in r["sweeps"].items():
        rate = f"{s['TB_per_s']:5.2f} TB/s" if s["TB_per_s"] is not None else "   [k, n] floats only"
        print(f"  {name:20s} {s['ms']:8.3f} ms  {s['h_streams']} h-sized streams  {rate}")
    for name in ("hip", "literal", "mv"):
        f = r["forms"][name]
        tail = f"  HIP / this = {f['hip_over_this']:.2f}" if "hip_over_this" in f else ""
        print(f"  {name:8s} forward {f['forward_ms']:8.3f} ms  backward {f['backward_ms']:8.3f} ms  "
              f"total {f['total_ms']:8.3f} ms{tail}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="write the results as JSON")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per shape")
    ap.add_argument("--shape", nargs=3, metavar=("N", "C", "BATCH"), help="(child) one shape, JSON on the last line")
    args = ap.parse_args()
    if args.shape:
        print(json.dumps(one_shape(*(int(v) for v in args.shape))))
        return 0
    results = []
    for n, c, k in SHAPES:
        # a fresh child per shape: its memory is gone when it ends, and a step that hangs ends with its timeout
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", str(n), str(c), str(k)],
                                 capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(f"{n} x ({k} x {c}): no result within {args.timeout} s; stopping", file=sys.stderr)
            return 1
        if out.returncode != 0:
            print(out.stderr, file=sys.stderr)
            print(f"{n} x ({k} x {c}): exit status {out.returncode}; stopping", file=sys.stderr)
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
