#!/usr/bin/env python3
"""Time of vertex selection (pygcn_amd/select.py over gcn_select_kth / gcn_select_indices / gcn_topk_flag /
gcn_race_keys) beside the fork's literal lines on the same tensors:

    topk_flag                     vs  argsort + where               reference pygcn/models.py:373-377
    sample_without_replacement    vs  multinomial + .tolist()       reference pygcn/rl-policy-generator.py:332

at n = 10^6 and 10^7 vertices, k = 1 and 20 windows, NN = 100 and 10^4.  Medians from device events after a
warm-up; the fork's draw ends in a host read, so its time is taken on the host clock around a synchronised call
as well.  The kernels alone (the radix select, the index pass, the flag sweep, the race keys) are timed too.
Each shape runs in a child process of its own under a timeout; a shape that fails or hangs ends the run.

    python tools/select_cost.py [--out profiles/select_cost.json] [--timeout 300]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(n, k, nn) for n in (1_000_000, 10_000_000) for k in (1, 20) for nn in (100, 10_000)]


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


def wall_of(fn, reps=9):
    import torch
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[reps // 2]


def one_shape(n, k, nn):
    import torch
    from pygcn_amd import select as S
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    scores = torch.randn(k, n, generator=gen, device=dev)
    probs = torch.softmax(torch.randn(k, n, generator=gen, device=dev), dim=1)

    def literal_flag(s):          # the fork's lines, one window after the other (its models are not batched)
        out = []
        for j in range(s.shape[0]):
            col = s[j].view(-1, 1)
            sorted_indices = torch.argsort(col, dim=0, descending=True)
            topk_mask = torch.where(col > col[sorted_indices[nn]], torch.reciprocal(col), torch.zeros_like(col))
            out.append(col * topk_mask)
        return out

    def literal_draw(p):
        return [torch.multinomial(p[j], nn, replacement=False).tolist() for j in range(p.shape[0])]

    keys = S.race_keys(probs, 7)
    thr, cnt = S.kth_largest(keys, nn)
    res = {"n": n, "batch": k, "NN": nn, "device": torch.cuda.get_device_name(0),
           "vector_MB": 4e-6 * n * k,
           "kernels_ms": {
               "select_kth": t_of(lambda: S.kth_largest(scores, nn + 1)),
               "select_indices": t_of(lambda: S.topk_indices(keys, nn, thr, cnt)),
               "topk_flag_sweep": t_of(lambda: S.flag_above(scores, thr)),
               "race_keys": t_of(lambda: S.race_keys(probs, 7))},
           "topk_flag_ms": {"hip": t_of(lambda: S.topk_flag(scores, nn)), "literal": t_of(lambda: literal_flag(scores))},
           "sample_ms": {"hip": t_of(lambda: S.sample_without_replacement(probs, nn, seed=7)),
                         "hip_wall": wall_of(lambda: S.sample_without_replacement(probs, nn, seed=7)),
                         "literal_wall": wall_of(lambda: literal_draw(probs))}}
    same = all(torch.equal(a.view(-1), b) for a, b in zip(literal_flag(scores), S.topk_flag(scores, nn)))
    res["topk_flag_equals_literal"] = bool(same)
    res["topk_flag_ms"]["hip_over_literal"] = res["topk_flag_ms"]["hip"] / res["topk_flag_ms"]["literal"]
    res["sample_ms"]["hip_over_literal_wall"] = res["sample_ms"]["hip_wall"] / res["sample_ms"]["literal_wall"]
    return res


def show(r):
    print(f"n = {r['n']}, k = {r['batch']}, NN = {r['NN']} ({r['vector_MB']:.0f} MB per vector) on {r['device']}")
    print("  kernels  " + "  ".join(f"{name} {t:.3f} ms" for name, t in r["kernels_ms"].items()))
    f, s = r["topk_flag_ms"], r["sample_ms"]
    print(f"  topk_flag  HIP {f['hip']:.3f} ms  literal {f['literal']:.3f} ms  HIP / literal = {f['hip_over_literal']:.3f}"
          f"  (same bits: {r['topk_flag_equals_literal']})")
    print(f"  sample     HIP {s['hip']:.3f} ms (wall {s['hip_wall']:.3f})  literal wall {s['literal_wall']:.3f} ms  "
          f"HIP / literal = {s['hip_over_literal_wall']:.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="write the results as JSON")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per shape")
    ap.add_argument("--shape", nargs=3, metavar=("N", "BATCH", "NN"), help="(child) one shape, JSON on the last line")
    args = ap.parse_args()
    if args.shape:
        print(json.dumps(one_shape(*(int(v) for v in args.shape))))
        return 0
    results = []
    for n, k, nn in SHAPES:
        # a fresh child per shape: its memory is gone when it ends, and a step that hangs ends with its timeout
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", str(n), str(k), str(nn)],
                                 capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(f"n = {n}, k = {k}, NN = {nn}: no result within {args.timeout} s; stopping", file=sys.stderr)
            return 1
        if out.returncode != 0:
            print(out.stderr, file=sys.stderr)
            print(f"n = {n}, k = {k}, NN = {nn}: exit status {out.returncode}; stopping", file=sys.stderr)
            return 1
        results.append(json.loads(out.stdout.strip().splitlines()[-1]))
        show(results[-1])
        if args.out:                  # (after every shape: a later one that fails keeps the earlier results)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
