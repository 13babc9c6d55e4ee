"""Which launching entry points the suite replays from a hipGraph (tests/test_capture_gpu.py), and which it cannot.

Every entry point of include/gcn_spmm.h whose last parameter is the stream stands in exactly one of two tables:

  CAPTURED    entry point -> the case of tests/test_capture_gpu.py that captures it on its own, replays it against
              the eager call bit for bit, refills its inputs in place and replays again;
  HOST_READ   entry point -> file:line of the host read in its Python wrapper.  Only an entry point whose wrapper's
              OUTPUT SHAPE depends on device data may stand here: the wrapper has to read a count back before it can
              allocate, so no capture can contain it.  (The `*_host` functions take no stream and launch nothing.)

Runs without a GPU: the header, the binding table and the wrappers' source lines are all it reads."""
import os
import re

from conftest import ROOT

CAPTURED = {
    "gcn_spmm_csr": "spmm_c_abi",
    "gcn_spmm_csr_ep": "spmm_epilogue",
    "gcn_rows_pack512": "packed_rows",
    "gcn_spmm_csr_packed": "packed_rows",
    "gcn_rows_pack384": "packed_rows",
    "gcn_spmm_csr_packed384": "packed_rows",
    "gcn_sddmm_csr": "sddmm",
    "gcn_relu_dropout_backward": "backward_sweeps",
    "gcn_relu_dropout_backward_colsum": "backward_sweeps",
    "gcn_log_softmax_backward_colsum": "backward_sweeps",
    "gcn_nll_log_softmax_backward_colsum": "backward_sweeps",
    "gcn_gemm_xw256_f32": "gemm_c_abi",
    "gcn_gemm_xw256_f32_b3": "gemm_xw256",
    "gcn_gemm_xw256_f32_h2": "gemm_xw256",
    "gcn_gemm_xw256_f32_b3_logsoftmax": "gemm_log_softmax",
    "gcn_gemm_xw_bf16": "gemm_bf16",
    "gcn_gemm_atg256_f32": "weight_grad",
    "gcn_gemm_atg256_f32_b3": "weight_grad",
    "gcn_gemm_atg256_f32_b3_colsum": "weight_grad",
    "gcn_gemm_atg_bf16": "weight_grad",
    "gcn_bn_stats": "bn_sweeps",
    "gcn_bn_apply": "bn_sweeps",
    "gcn_bn_backward_sums": "bn_sweeps",
    "gcn_bn_backward_apply": "bn_sweeps",
    "gcn_bn_stats_batched": "bn_sweeps_batched",
    "gcn_bn_apply_batched": "bn_sweeps_batched",
    "gcn_bn_backward_sums_batched": "bn_sweeps_batched",
    "gcn_bn_backward_apply_batched": "bn_sweeps_batched",
    "gcn_masked_colsum": "masked_pool",
    "gcn_masked_broadcast": "masked_pool",
    "gcn_attn_scores": "attention",
    "gcn_attn_normalize": "attention",
    "gcn_attn_backward": "attention",
    "gcn_select_kth": "select",
    "gcn_select_indices": "select",
    "gcn_topk_flag": "select",
    "gcn_race_keys": "select",
    "gcn_race_keys_dev": "select",
    "gcn_eval_ingest": "eval_ingest",
    "gcn_eval_ingest_backward": "eval_ingest",
    "gcn_vmlp_forward": "vertex_mlp",
    "gcn_vmlp_backward": "vertex_mlp",
    "gcn_dropout_rows": "dropout_rows",
    "gcn_bn_linear_forward": "bn_linear",
    "gcn_bn_linear_backward_sums": "bn_linear",
    "gcn_bn_linear_backward_apply": "bn_linear",
    "gcn_agg_linear_forward": "agg_linear",
    "gcn_agg_linear_backward": "agg_linear",
    "gcn_gather_f32": "gather",
    "gcn_row_normalize_device": "normalize_in_place",
    "gcn_sym_normalize_device": "normalize_in_place",
    "gcn_rows_unpack": "rows_unpack",
    "gcn_bits_row_counts": "rows_unpack",
    # fixed-shape results, no host read in the wrapper (the reads of share_transpose() and of a plan come later)
    "gcn_csr_transpose_device": "transpose",
    "gcn_csr_mirror_device": "mirror",
}

HOST_READ = {
    # entry point: (file, the wrapper's host read as it stands in that file, what is read)
    "gcn_plan_count_device": ("pygcn_amd/graph.py", "ni, nc, nl = (int(v) for v in counts.tolist())",
                              "the sizes of the schedule arrays"),
    "gcn_plan_fill_device": ("pygcn_amd/graph.py", "ni, nc, nl = (int(v) for v in counts.tolist())",
                             "its arrays are allocated from the counts of gcn_plan_count_device"),
    "gcn_coo_to_csr_device": ("pygcn_amd/graph.py", "k = int(nnz_out.item())", "the number of distinct entries"),
    "gcn_dense_to_csr_count": ("pygcn_amd/graph.py", "nnz = int(rowptr[-1].item())", "the number of kept entries"),
    "gcn_dense_to_csr_fill": ("pygcn_amd/graph.py", "nnz = int(rowptr[-1].item())",
                              "col and val are allocated from the count"),
    "gcn_csr_take_rows": ("pygcn_amd/graph.py", "total = int(rp[-1])", "the number of entries of the taken rows"),
    "gcn_csr_sample_rows": ("pygcn_amd/sampling.py", "total = int(rp_out[-1])", "the number of kept entries"),
    "gcn_rows_pack_count": ("pygcn_amd/spmm.py", "vals = torch.empty(int(offsets[-1])", "the number of non-zero values"),
    "gcn_rows_pack_values": ("pygcn_amd/spmm.py", "vals = torch.empty(int(offsets[-1])",
                             "vals is allocated from the count"),
}


def launching_entry_points():
    """name -> parameter list of every declaration of the header whose last parameter is `void *stream`."""
    hdr = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decls = re.findall(r"^[A-Za-z_][\w \*]*?\b(gcn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code, flags=re.M)
    return {name: params for name, params in decls
            if re.search(r"\bvoid\s*\*\s*stream\s*$", params.strip())}


def host_read_line(name):
    """(file, 1-based line number) of the host read cited for `name`; the line must exist exactly once."""
    path, text, _ = HOST_READ[name]
    lines = open(os.path.join(ROOT, path)).read().splitlines()
    hits = [i + 1 for i, line in enumerate(lines) if text in line]
    assert len(hits) == 1, f"{name}: `{text}` stands {len(hits)} times in {path}"
    return path, hits[0]


def test_every_launching_entry_point_is_in_exactly_one_table():
    import ctypes
    from pygcn_amd import _native
    launching = launching_entry_points()
    assert len(launching) > 60
    for name in launching:                  # the binding table agrees: a stream is its last argument
        assert name in _native.SIGNATURES and _native.SIGNATURES[name][1][-1] is ctypes.c_void_p, name
    both = set(CAPTURED) & set(HOST_READ)
    assert not both, f"in both tables: {sorted(both)}"
    listed = set(CAPTURED) | set(HOST_READ)
    assert listed == set(launching), f"missing: {sorted(set(launching) - listed)}, unknown: {sorted(listed - set(launching))}"


def test_host_read_entries_cite_a_host_read_behind_a_launch_of_theirs():
    """Each HOST_READ line exists, reads the device (int(...) of a device scalar, .item(), .tolist()), and a launch
    of that entry point stands in the same file — by its name, or for the second of a pair by its partner's."""
    for name in HOST_READ:
        path, line = host_read_line(name)
        text = HOST_READ[name][1]
        assert re.search(r"int\(|\.item\(\)|\.tolist\(\)", text), (name, text)
        src = open(os.path.join(ROOT, path)).read()
        assert f'"{name}"' in src, f"{path} does not launch {name}"
        assert not name.endswith("_host")


def test_captured_entries_name_cases_of_the_gpu_file():
    """Every case named in CAPTURED is a case the GPU file runs, and every case of the GPU file captures something
    (the file's own union check needs a GPU; this holds the names together without one)."""
    src = open(os.path.join(ROOT, "tests", "test_capture_gpu.py")).read()
    cases = set(re.findall(r'^@case\("([a-z0-9_]+)"', src, flags=re.M))
    assert set(CAPTURED.values()) == cases, set(CAPTURED.values()) ^ cases


def test_the_coverage_document_holds_both_tables():
    doc = open(os.path.join(ROOT, "profiles", "capture_coverage.md")).read()
    for name, case in CAPTURED.items():
        assert re.search(rf"\|\s*`{name}`\s*\|\s*`{case}`\s*\|", doc), f"{name} -> {case} is not in the document"
    for name in HOST_READ:
        path, line = host_read_line(name)
        assert re.search(rf"\|\s*`{name}`\s*\|\s*`{re.escape(path)}:{line}`", doc), f"{name}: {path}:{line} not cited"
