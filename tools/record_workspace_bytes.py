"""Records what every *_workspace_bytes query of the C ABI answers on a grid of arguments, as JSON on stdout:
{query: [[arg, ..., bytes], ...]}.  The answers are ABI-visible (a caller sizes its buffers by them) and follow the
slab rules of the sweeps, so tests/golden/workspace_bytes.json holds them as recorded at a known commit and
tests/test_host_cpu.py replays every recorded call.  The queries cannot launch: no device is needed.

    python tools/record_workspace_bytes.py > tests/golden/workspace_bytes.json

The grid: n_rows at the slab edges (one slab of 64 rows, the 2048-slab cap, the int32 row bound, past every bound);
widths that the 16-byte lane rule takes and refuses at either dtype, and an unknown dtype; batch at 0, 1, the
gridDim.y bound 65535 and past it.
"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_ROWS = [0, 1, 2, 63, 64, 65, 64 * 2048, 64 * 2048 + 1, 2 ** 31 - 1, 2 ** 31 * 2048]
WIDTHS = [-4, 0, 3, 4, 8, 12, 24, 256, 1024, 1028, 2048, 4096]
DTYPES = [0, 1, 7]                       # GCN_DTYPE_F32, GCN_DTYPE_BF16, unknown
BATCHES = [0, 1, 65535, 65536]


def grid():
    """{query: [argument tuple, ...]}; gcn_spmm_workspace_bytes's first argument is its plan's n_chunks."""
    g = {}
    rows_widths = [(n, f, dt) for n in N_ROWS for f in WIDTHS for dt in DTYPES]
    g["gcn_bwd_colsum_workspace_bytes"] = rows_widths
    g["gcn_bn_workspace_bytes"] = rows_widths
    batched = [(n, f, 1, dt) for n, f, dt in rows_widths]
    batched += [(n, f, b, dt) for n in (1, 2, 65, 64 * 2048 + 1) for f in (8, 256) for b in BATCHES for dt in (0, 1)]
    for name in ("gcn_bn_batched_workspace_bytes", "gcn_pool_workspace_bytes", "gcn_attn_workspace_bytes"):
        g[name] = batched
    g["gcn_select_workspace_bytes"] = [(n, b) for n in N_ROWS + [1024, 1025, 1024 * 1024 + 1] for b in BATCHES]
    g["gcn_eval_workspace_bytes"] = ([(n, f, d, 1) for n in N_ROWS for f, d in ((1, 0), (2, 0), (17, 3), (64, 63), (64, 64), (65, 0))] +
                                     [(n, 17, 3, b) for n in (1, 65, 64 * 2048 + 1) for b in BATCHES + [20]])
    g["gcn_vmlp_workspace_bytes"] = ([(n, 32, 1, 32, 32) for n in N_ROWS] +
                                     [(65, c, t, h1, h2) for c, t, h1, h2 in ((0, 0, 1, 1), (1, 0, 1, 1), (64, 32, 64, 64),
                                                                              (65, 0, 16, 16), (32, 33, 16, 16), (32, 9, 16, 17),
                                                                              (32, 9, 33, 8), (32, 9, 65, 8), (32, 9, 0, 8))])
    g["gcn_bn_linear_workspace_bytes"] = ([(n, 32, 32, 1) for n in N_ROWS + [2 ** 40, 2 ** 40 + 1]] +
                                          [(65, 32, 32, b) for b in BATCHES] + [(65, 16, 32, 1), (65, 32, 64, 1)])
    g["gcn_sym_normalize_workspace_bytes"] = [(n,) for n in [-1] + N_ROWS]
    # (three queries add hipCUB's temporary-storage size to this library's own arrays, and hipCUB sizes that for
    #  the device it finds — a machine without one answers differently.  Recorded where hipCUB is not asked: row
    #  counts outside the planner's range, and matrices without entries)
    g["gcn_plan_device_workspace_bytes"] = [(-1,), (2 ** 31 - 1,), (2 ** 31 * 2048,)]
    g["gcn_spmm_workspace_bytes"] = [(c, f) for c in (0, 1, 3) for f in (0, 1, 256)]
    empty = [(0, 0, 0), (4, 4, 0), (2 ** 31 - 1, 4, 0), (60, 90, -1)]
    g["gcn_csr_transpose_workspace_bytes"] = empty
    g["gcn_coo_to_csr_workspace_bytes"] = empty
    for name in ("gcn_gemm_xw256_workspace_bytes", "gcn_gemm_xw256_h2_workspace_bytes", "gcn_gemm_xw256_b3_workspace_bytes"):
        g[name] = [()]
    shapes = [(k, n) for k in (64, 128, 256) for n in (64, 128, 256)]
    g["gcn_gemm_bf16_workspace_bytes"] = shapes
    lists = [0, 1, 31, 32, 33, 4096, 10 ** 6]
    g["gcn_gemm_atg256_workspace_bytes"] = [(n,) for n in lists]
    g["gcn_gemm_atg_bf16_workspace_bytes"] = [(n, k, m) for n in lists for k, m in shapes]
    return g


def ask(name, args):
    """One query of the loaded library; the plan of gcn_spmm_workspace_bytes is built from its n_chunks."""
    from pygcn_amd import _native
    fn = getattr(_native.lib(), name)
    if name == "gcn_spmm_workspace_bytes":
        plan = _native.GcnCsrPlan()
        plan.n_chunks = args[0]
        return int(fn(ctypes.byref(plan), *args[1:]))
    return int(fn(*args))


def main():
    from pygcn_amd import _native
    g = grid()
    queries = sorted(n for n in _native.SIGNATURES if n.endswith("_workspace_bytes"))
    assert queries == sorted(g), set(queries) ^ set(g)
    print("{")
    for k, name in enumerate(queries):
        rows = [list(a) + [ask(name, a)] for a in g[name]]
        print(f' "{name}": {json.dumps(rows, separators=(",", ":"))}' + ("," if k + 1 < len(queries) else ""))
    print("}")


if __name__ == "__main__":
    main()
