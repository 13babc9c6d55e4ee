#!/usr/bin/env python3
"""Bit parity of the one-node 2-layer training step (pygcn_amd/fused.py) between two commits: the same file runs on
both, because it reaches the code through the public calls only — model(...) with its arguments, set_gemm_scheme,
set_packed_hidden, set_input_product_cache.

For every case it takes ONE training step under a fixed torch.manual_seed (two with the input-product cache on:
the second is the one recorded) and writes

    sha256     of the output rows (and the full matrix with keep_full) and of every gradient (grad_x where asked)
    launches   the ordered C-ABI entry names that went through _native.launch during the step (the function is
               wrapped for its duration), as an index into the table `launch_sequences`

Every case runs TWICE in the process; where the two runs differ it is marked not_reproducible, with both sets of
digests, instead of being hashed.  A combination the model refuses is recorded as refused, with the message.

Cases (host code that chooses launches is what is under test, so the shapes are those that take each branch):
an R-MAT graph of 2001 vertices / ~20 000 edges (more than one 128-row tile, not a multiple of it); widths
256-256-256, 256-256-64 (l1_follows_l2), 200-256-40 (layer 1 not reassociable, the c_select branch), 48-64-16 in
fp32 and 128-128-128 in bf16; the six routes; loss rows sorted / permuted / with repeats / empty; dropout 0, 0.4,
0.5; schemes bf16x3 and h2; the packed hidden rows on and off where they apply; the input-product cache on and
off; x.requires_grad on and off.  The rows of X are spread over 24 octaves, or a bound that changed under "h2"
would not show (see run_case; measured: without the 1.0001·scale of the restricted pass's h_bound 40 cases differ,
with rows of one magnitude none did).  `model(x, g)` becomes one autograd node only from tuning.ROWGRAD_MIN_ROWS
vertices, so its three routes (RowGrad, NLLGrad, dense) run on a second graph of 16 411 vertices as well.

    python tools/fused_parity.py --out A.json                       on each commit (needs the GPU)
    python tools/fused_parity.py --compare A.json B.json [--speed S.json] --out profiles/fused_refactor_parity.json

--compare checks the two files case by case (one SHA-256 per case and commit over the case's digests and launch
names), names every case that differs, and writes both columns folded to one line per (widths, graph, route); it
exits 1 if a comparable case differs, or if an fp32 256-256-256 case at dropout 0 is not reproducible."""
import argparse
import hashlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTHS = [(256, 256, 256, "f32"), (256, 256, 64, "f32"), (200, 256, 40, "f32"), (48, 64, 16, "f32"),
          (128, 128, 128, "bf16")]
ROWS_ROUTES = ("rows", "rows_keep_full", "restricted")          # model(x, g, rows=idx, ...)
NODE_ROUTES = ("rowgrad", "nllgrad", "dense")                   # model(x, g) and what the loss does with it
IDX_KINDS = ("sorted", "permuted", "repeats", "empty")
DROPOUTS = (0.0, 0.4, 0.5)
SCHEMES = ("bf16x3", "h2")
GRAPHS = {"n2001": (2001, 20_000), "n16411": (16_411, 160_000)}


def cases():
    """(id, settings) in a fixed order."""
    for (fin, hid, ncls, dt), scheme, p, cache, xgrad in itertools.product(WIDTHS, SCHEMES, DROPOUTS, (0, 1), (0, 1)):
        packed_opts = (1, 0) if ((fin, hid, ncls) == (256, 256, 256) and p > 0.0) else (1,)
        for packed in packed_opts:
            for gname in GRAPHS:
                routes = [(r, k) for r in ROWS_ROUTES for k in IDX_KINDS] if gname == "n2001" else []
                routes += [(r, k) for r in NODE_ROUTES for k in (IDX_KINDS[:3] if r == "rowgrad" else ("all",))]
                if gname != "n2001" and cache and xgrad:
                    continue        # (a feature matrix that needs a gradient bypasses the cache: covered on n2001)
                for route, kind in routes:
                    cid = (f"{fin}-{hid}-{ncls}{dt}/{gname}/{route}/{kind}/p{p}/{scheme}/packed{packed}/cache{cache}"
                           f"/xgrad{xgrad}")
                    yield cid, dict(widths=(fin, hid, ncls), dtype=dt, graph=gname, route=route, idx=kind, dropout=p,
                                    scheme=scheme, packed=packed, cache=cache, xgrad=xgrad)


def digest(t):
    import torch
    t = t.detach().as_subclass(torch.Tensor).contiguous()
    h = hashlib.sha256(f"{tuple(t.shape)}{t.dtype}".encode())
    h.update(t.reshape(-1).view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


class Fixture:
    """The graphs, index lists and labels every case shares (seeded; built once)."""

    def __init__(self, dev):
        import torch
        from pygcn_amd import CSRGraph
        from pygcn_amd.utils import rmat_graph
        self.graphs, self.idx, self.labels = {}, {}, {}
        for name, (n, e) in GRAPHS.items():
            rowptr, col, val = rmat_graph(n, e, seed=42, perm_seed=43, device=dev)
            self.graphs[name] = CSRGraph(rowptr, col, val, (n, n))
            gen = torch.Generator(device="cpu").manual_seed(7)
            perm = torch.randperm(n, generator=gen).to(dev)
            self.idx[name] = {"sorted": torch.arange(3, n, 9, device=dev), "permuted": perm[:211].contiguous(),
                              "repeats": torch.cat((perm[300:400], perm[350:420])),
                              "empty": torch.empty(0, dtype=torch.int64, device=dev)}
            self.labels[name] = torch.randint(0, 1 << 30, (n,), generator=gen).to(dev)


def run_case(fx, c, dev):
    """One run of a case: ({tensor name: sha256}, [launch names]) of the recorded step.  (Graphs and index lists
    are shared, so the FIRST run of a case can contain one-off launches — a transpose, a schedule, the row blocks —
    that its second run does not: measure() keeps both lists where they differ.)"""
    import torch
    import torch.nn.functional as F
    from pygcn_amd import GCN, _native, fused, functional, spmm
    fin, hid, ncls = c["widths"]
    dt = torch.float32 if c["dtype"] == "f32" else torch.bfloat16
    g, y_all = fx.graphs[c["graph"]], fx.labels[c["graph"]] % ncls
    n = g.shape[0]
    idx = fx.idx[c["graph"]].get(c["idx"])
    was_packed = fused.packed_hidden()
    spmm.set_gemm_scheme(c["scheme"])
    fused.set_packed_hidden(bool(c["packed"]))
    fused.set_input_product_cache(bool(c["cache"]))
    torch.manual_seed(1234)
    model = GCN(fin, hid, ncls, dropout=c["dropout"]).to(device=dev, dtype=dt)
    model.train()
    # (rows of X spread over 24 octaves: under "h2" the low-order fp16 parts of small rows then depend on the
    #  power-of-two scale the bound selects, so a bound that changed shows in the result bits — with rows of one
    #  magnitude the scaling is exact and any sufficient bound gives the same bits)
    x = torch.randn(n, fin, device=dev, generator=torch.Generator(device=dev).manual_seed(44))
    x = (x * torch.exp2(((torch.arange(n, device=dev) * 7) % 25 - 12).float()).unsqueeze(1)).to(dt)
    x.requires_grad_(bool(c["xgrad"]))

    def step():
        torch.manual_seed(99)                                   # (the dropout seed comes from the generator's state)
        model.zero_grad(set_to_none=True)
        x.grad = None
        full = None
        if c["route"] == "rows":
            out = model(x, g, rows=idx)
        elif c["route"] == "rows_keep_full":
            out, full = model(x, g, rows=idx, keep_full=True)
        elif c["route"] == "restricted":
            out = model(x, g, rows=idx, restrict_forward=True)
        else:
            out = model(x, g)
        if c["route"] == "nllgrad":
            loss = functional.nll_loss(out, y_all)
        elif c["route"] == "dense":
            loss = F.nll_loss(out, y_all)
        else:
            if c["route"] == "rowgrad":
                out = out[idx]
            loss = F.nll_loss(out, y_all[idx])
        loss.backward()
        return out, full

    names = []
    orig = _native.launch

    def spy(name, *args, **kwargs):
        names.append(name)
        return orig(name, *args, **kwargs)
    _native.launch = spy
    try:
        for _ in range(2 if c["cache"] else 1):
            del names[:]
            out, full = step()
        torch.cuda.synchronize()
    finally:
        _native.launch = orig
        fused.set_input_product_cache(False)
        fused.set_packed_hidden(was_packed)
        spmm.set_gemm_scheme("bf16x3")
    d = {"out": digest(out), "finite": bool(torch.isfinite(out.detach()).all())}
    if full is not None:
        d["full"] = digest(full)
    for k, p in model.named_parameters():
        d["grad_" + k] = digest(p.grad) if p.grad is not None else None
    if c["xgrad"]:
        d["grad_x"] = digest(x.grad) if x.grad is not None else None
    return d, list(names)


def measure(out_path):
    import torch
    dev = torch.device("cuda:0")
    fx = Fixture(dev)
    sequences, table, result = [], {}, {}
    for cid, c in cases():
        runs = []
        try:
            for _ in range(2):
                runs.append(run_case(fx, c, dev))
        except RuntimeError as e:
            msg = str(e)
            if "HIP" in msg or "hip" in msg:            # a device error is a finding, not a refusal: stop here
                raise
            result[cid] = {"status": "refused", "message": msg.splitlines()[0][:200]}
            continue
        if runs[0][0] != runs[1][0]:
            result[cid] = {"status": "not_reproducible", "runs": [d for d, _ in runs]}
            continue

        def seq(names):
            if tuple(names) not in table:
                table[tuple(names)] = len(sequences)
                sequences.append(names)
            return table[tuple(names)]
        result[cid] = {"status": "ok", "sha256": runs[1][0], "launches": seq(runs[1][1])}
        if runs[0][1] != runs[1][1]:
            result[cid]["launches_first_run"] = seq(runs[0][1])
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "n_cases": len(result),
           "launch_sequences": sequences, "cases": result}
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    count = {s: sum(1 for v in result.values() if v["status"] == s) for s in ("ok", "not_reproducible", "refused")}
    count["with_non_finite_output"] = sum(1 for v in result.values()
                                          if v["status"] == "ok" and not v["sha256"]["finite"])
    print(json.dumps({"cases": len(result), **count, "distinct_launch_sequences": len(sequences)}))


def column(doc, cid):
    """One SHA-256 for a case of one commit: over its per-tensor digests and the names of its launches."""
    v = doc["cases"][cid]
    if v["status"] != "ok":
        return None
    seqs = [doc["launch_sequences"][v[k]] for k in ("launches", "launches_first_run") if k in v]
    return hashlib.sha256(json.dumps([v["sha256"], seqs], sort_keys=True).encode()).hexdigest()


def compare(path_a, path_b, speed, out_path):
    a, b = (json.load(open(p)) for p in (path_a, path_b))
    if list(a["cases"]) != list(b["cases"]):
        raise SystemExit("--compare: the two files do not list the same cases")
    rows, left_out, differ, must = {}, {}, [], []
    for cid in a["cases"]:
        va, vb = a["cases"][cid], b["cases"][cid]
        if va["status"] == "refused" or vb["status"] == "refused":
            rows[cid] = {"parent": va["status"], "new": vb["status"]}
            if va["status"] != vb["status"]:
                differ.append(cid)
        elif va["status"] == "not_reproducible":          # (on the parent itself: listed, not compared)
            left_out[cid] = {"parent": va["runs"], "new": vb.get("runs", vb.get("sha256"))}
            if cid.startswith("256-256-256f32/") and "/p0.0/" in cid:
                must.append(cid)
        else:
            rows[cid] = {"parent": column(a, cid), "new": column(b, cid)}
            if rows[cid]["parent"] != rows[cid]["new"]:
                differ.append(cid)
    # the comparison is case by case (above: `differ` names every case whose columns differ); the file that is
    # kept folds the cases of one (widths, graph, route) into one line, or it would be 2822 pairs of digests long
    groups = {}
    for cid, cols in rows.items():
        g = groups.setdefault("/".join(cid.split("/")[:3]), {"cases": 0, "parent": hashlib.sha256(),
                                                              "new": hashlib.sha256()})
        g["cases"] += 1
        for who in ("parent", "new"):
            g[who].update(f"{cid} {cols[who]}\n".encode())
    for g in groups.values():
        g["parent"], g["new"] = g["parent"].hexdigest(), g["new"].hexdigest()
    doc = {"what": __doc__.split("\n\n")[0].replace("\n", " "),
           "device": a["device"], "n_cases": len(a["cases"]), "n_compared": len(rows), "n_differ": len(differ),
           "differ": differ, "not_reproducible_on_parent": left_out,
           "column": "per commit, sha256 over the lines '<case id> <sha256 over [per-tensor sha256 digests, ordered "
                     "launch names] of the case>' of the group's cases, in the order of --list",
           "groups": groups}
    if speed:
        doc["speed"] = json.load(open(speed))

    def lines(d, depth):         # one line per entry down to `depth`, so that a group or a setting is one line
        if depth == 0 or not isinstance(d, dict) or not d:
            return json.dumps(d)
        return "{\n" + ",\n".join(f"{json.dumps(k)}: {lines(v, depth - 1)}" for k, v in d.items()) + "\n}"
    with open(out_path, "w") as f:
        f.write(lines(doc, 2) + "\n")
    print(json.dumps({k: doc[k] for k in ("n_cases", "n_compared", "n_differ")}), "left out:", len(left_out))
    if differ or must:
        raise SystemExit(f"{len(differ)} cases differ; {len(must)} fp32 256-256-256 dropout-0 cases not reproducible")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--compare", nargs=2, metavar=("PARENT", "NEW"))
    ap.add_argument("--speed", default=None, help="with --compare: a JSON file of bench.py figures to carry along")
    ap.add_argument("--list", action="store_true", help="print the case ids and exit")
    args = ap.parse_args()
    if args.list:
        print("\n".join(cid for cid, _ in cases()))
    elif args.compare:
        compare(*args.compare, args.speed, args.out)
    else:
        measure(args.out)


if __name__ == "__main__":
    main()
