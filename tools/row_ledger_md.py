"""JSON written by `PYGCN_ROW_LEDGER=<file> pytest -m gpu tests/test_spmm_matrix_gpu.py` -> the table of
profiles/row_parity_ledger.md:  python tools/row_ledger_md.py <file> > profiles/row_parity_ledger.md"""
import json
import sys

rows = json.load(open(sys.argv[1]))
print("# Row-by-row parity of the sparse kernels (MI355X)\n")
print("`PYGCN_ROW_LEDGER=… pytest -m gpu tests/test_spmm_matrix_gpu.py`: the worst `err / bound` of every element of\n"
      "every check (plain, bias, ReLU, flags + maximum, log_softmax, dropout, operand hint, row selection, inf beside\n"
      "finite values, transpose; int32 and int64 row pointers, two schedules) per kernel variant.  Bound: "
      "`tests/_rowcheck.py`.\n")
print("| storage | F | kernel variant (expected_variant) | worst err / bound | fused log_softmax: worst err / its bound |")
print("|---|---|---|---|---|")
for r in rows:
    lsm = r.get("log_softmax_err_over_bound")
    print(f"| {r['dtype']} | {r['F']} | `{r['variant']}` | {r['worst_err_over_bound']:.3f} | "
          f"{'-' if lsm is None else format(lsm, '.3f')} |")
top = max(max(r["worst_err_over_bound"], r.get("log_softmax_err_over_bound") or 0.0) for r in rows)
print(f"\n{len(rows)} lines, largest ratio {top:.3f}.")
