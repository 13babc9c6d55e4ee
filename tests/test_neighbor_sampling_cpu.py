"""CPU side of neighbour sampling (pygcn_amd/csrc/gcn_sample.hip, CSRGraph.sample_neighbors): the header, the binding
table and the library; every argument check of `gcn_csr_sample_rows`, which run before any launch; the numpy
restatement tests/_neighbor_ref.py on hand-written rows, its `rows` identity, and the LAW of its draws — the device is
held bit for bit to the restatement on the GPU (tests/test_neighbor_sampling_gpu.py), so the statistics are checked
here, once, on the restatement.  No GPU needed."""
import ctypes
import itertools
import json
import os
import re

import numpy as np
import pytest
import torch

import _neighbor_ref as R
from conftest import GOLDEN, ROOT

NAME, COUNT = "gcn_csr_sample_rows", 17
BADARG, ALIGN = -1, -2


def test_header_table_and_library():
    from pygcn_amd import _native, build
    hdr = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    assert re.search(r"#define GCN_ABI_VERSION\s+26\b", hdr) and _native.GCN_ABI_VERSION == 26
    assert _native.lib().gcn_abi_version() == 26                    # additive: the number did not move
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert NAME in _native.SIGNATURES and NAME in _native.EXPORTS
    decl = re.search(rf"\bint\s+{NAME}\s*\(([^)]*)\)\s*;", code)
    assert decl and len(decl.group(1).split(",")) == COUNT == len(_native.SIGNATURES[NAME][1])
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), NAME)
    assert getattr(_native.lib(), NAME).argtypes == _native.SIGNATURES[NAME][1]
    assert _native.SIGNATURES[NAME][0] is ctypes.c_int
    for name, value in (("GCN_SAMPLE_UNIFORM", 0), ("GCN_SAMPLE_WEIGHT", 1), ("GCN_SAMPLE_STRONGEST", 2),
                        ("GCN_SAMPLE_RESCALE_NONE", 0), ("GCN_SAMPLE_RESCALE_SUM", 1), ("GCN_SAMPLE_WAVE_ROW_MAX", 253),
                        ("GCN_SAMPLE_WAVE_SWEEP_ROWS", 65536)):
        assert int(re.search(rf"#define {name}\s+(\d+)", code).group(1)) == value == getattr(_native, name)
    assert R.MODES == ("uniform", "weight", "strongest")            # (the positions are the C constants)
    assert any(src.endswith("gcn_sample.hip") for src in build.SRCS)
    # the kernel takes no workspace: the set of *_workspace_bytes queries is the recorded one
    recorded = json.load(open(os.path.join(GOLDEN, "workspace_bytes.json")))
    assert sorted(n for n in _native.EXPORTS if n.endswith("_workspace_bytes")) == sorted(recorded)
    assert "workspace" not in decl.group(1)


# ------------------------------------------------------------------------------------------------ argument checks
P = 0x10000          # a "device address": aligned, never dereferenced — every call below fails its checks or has no rows


def _call(**over):
    from pygcn_amd import _native
    a = dict(rowptr=P, is64=0, col=P, val=P, rows=None, m=5, fanout=3, mode=0, seed=42, stream=0, diag=1, rescale=0,
             rowptr_out=P, out_is64=0, col_out=P, val_out=P)
    a.update(over)
    return _native.lib().gcn_csr_sample_rows(a["rowptr"], a["is64"], a["col"], a["val"], a["rows"], a["m"], a["fanout"],
                                             a["mode"], a["seed"], a["stream"], a["diag"], a["rescale"],
                                             a["rowptr_out"], a["out_is64"], a["col_out"], a["val_out"], None)


def _expect(code, **over):
    from pygcn_amd import _native
    assert _call(**over) == code, over
    assert _native.lib().gcn_last_error().decode().startswith(NAME + ":"), _native.lib().gcn_last_error()


@pytest.mark.parametrize("bad", [
    dict(fanout=0), dict(fanout=-4), dict(mode=3), dict(mode=-1), dict(rescale=2), dict(rescale=-1), dict(m=-1),
    dict(m=2 ** 40 + 1), dict(rowptr=None), dict(col=None), dict(val=None), dict(rowptr_out=None), dict(col_out=None),
    dict(val_out=None)])
def test_bad_arguments_are_refused_before_any_launch(bad):
    _expect(BADARG, **bad)


def test_misaligned_arrays_and_the_order_of_the_checks():
    for name in ("rowptr", "col", "val", "rowptr_out", "col_out", "val_out"):
        _expect(ALIGN, **{name: P + 2})
    _expect(ALIGN, rows=P + 4)
    _expect(ALIGN, rowptr=P + 4, is64=1)                             # a 64-bit row pointer: 8 bytes
    _expect(ALIGN, rowptr_out=P + 4, out_is64=1)
    _expect(BADARG, fanout=0, col=P + 2)                             # the argument rules first, the pointers after
    _expect(BADARG, mode=7, rowptr=None)


def test_no_rows_launch_nothing():
    assert _call(m=0) == 0
    assert _call(m=0, rowptr=None, col=None, val=None, rowptr_out=None, col_out=None, val_out=None) == 0
    _expect(BADARG, m=0, fanout=0)                                   # (the rule is still checked)
    # keep_diagonal together with a row list is fine — the row id is rows[r] — and so is any non-zero flag: m = 0
    assert _call(m=0, rows=P, diag=1) == 0 and _call(m=0, diag=7) == 0


def test_python_surface_refuses_without_a_device():
    from pygcn_amd import CSRGraph, functional, sampling
    assert callable(CSRGraph.sample_neighbors) and callable(functional.sample_neighbors)
    assert sampling.MODES == {name: i for i, name in enumerate(R.MODES)}
    with pytest.raises(RuntimeError, match="CSRGraph"):
        sampling.sample_neighbors(torch.eye(3), 2)
    with pytest.raises(RuntimeError, match="CSRGraph or a torch sparse tensor"):
        functional.sample_neighbors(torch.eye(3), 2)
    g = object.__new__(CSRGraph)                                     # (no device: only the argument rules are reached)
    g.shape = (3, 4)
    for kw, word in ((dict(fanout=0), "fanout"), (dict(fanout=2, by="random"), "by must be"),
                     (dict(fanout=2, rescale="mean"), "rescale"), (dict(fanout=2, stream=-1), "stream"),
                     (dict(fanout=2, stream=2 ** 32), "stream"), (dict(fanout=2, keep_diagonal=True), "square")):
        with pytest.raises(RuntimeError, match=word):
            g.sample_neighbors(**kw)


def test_train_flags_default_to_off():
    import subprocess
    import sys
    code = ("import train; a = train.parser.parse_args(['--fanout', '4', '--sample_by', 'weight']); "
            "b = train.parser.parse_args([]); print(a.fanout, a.sample_by, b.fanout, b.sample_by)\n"
            "try:\n    train.parser.parse_args(['--sample_by', 'loudest'])\n"
            "except SystemExit as e:\n    print('refused', e.code)")
    out = subprocess.run([sys.executable, "-c", code], cwd=os.path.join(ROOT, "pygcn_amd"), capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split("\n")[:2] == ["4 weight 0 uniform", "refused 2"], out.stdout


# ------------------------------------------------------------------------------------------------ the restatement
def _graph(degrees, n_cols, seed, values="random"):
    rng = np.random.default_rng(seed)
    rowptr = np.zeros(len(degrees) + 1, np.int64)
    np.cumsum(degrees, out=rowptr[1:])
    col = np.concatenate([np.sort(rng.choice(n_cols, d, replace=False)) for d in degrees] or [np.zeros(0)])
    val = rng.integers(1, 4096, col.size) / 4096.0 if values == "random" else np.asarray(values, np.float64)
    return rowptr, col.astype(np.int32), val.astype(np.float32)


def test_the_random_word_is_the_documented_philox_call():
    from _select_ref import philox4x32_10
    for e, seed, stream in ((0, 42, 0), (7, 42, 3), (2 ** 34 + 5, (1 << 63) + 9, 2 ** 32 - 1)):
        counter = np.array([[(e >> 2) & 0xFFFFFFFF, (e >> 2) >> 32, stream, 2]], np.uint64)
        want = philox4x32_10(counter, (seed & 0xFFFFFFFF, seed >> 32))[0, e & 3]
        assert R.random_words([e], seed, stream)[0] == want
    w = R.random_words(np.arange(64), 42, 0)
    assert len(set(w.tolist())) == 64
    assert not np.array_equal(w, R.random_words(np.arange(64), 42, 1))
    assert not np.array_equal(w, R.random_words(np.arange(64), 43, 0))
    # counter word 3 keeps the stream apart from the race keys' (1) and the dropout's (0)
    for other in (0, 1):
        counter = np.array([[0, 0, 0, other]], np.uint64)
        assert not np.array_equal(philox4x32_10(counter, (42, 0))[0], w[:4])


def test_hand_written_rows():
    rowptr, col = np.array([0, 6]), np.arange(6, dtype=np.int32)
    run = lambda val, K, **kw: R.sample_neighbors(rowptr, col, np.array(val, np.float32), 6, K, by="strongest",  # noqa: E731
                                                  keep_diagonal=False, **kw)
    assert run([3, 1, 3, 3, 0, 2], 2)[1].tolist() == [0, 2]             # ties: the entry stored earlier wins
    assert run([3, 1, 3, 3, 0, 2], 4)[1].tolist() == [0, 2, 3, 5]
    assert run([3, 1, 3, 3, 0, 2], 6)[1].tolist() == list(range(6)) == run([3, 1, 3, 3, 0, 2], 9)[1].tolist()
    nan, inf = float("nan"), float("inf")
    assert run([1, nan, inf, -inf, -0.0, 0.0], 1)[1].tolist() == [1]    # NaN above +inf
    assert run([1, nan, inf, -inf, -0.0, 0.0], 3)[1].tolist() == [0, 1, 2]
    assert run([-1, nan, inf, -inf, -0.0, 0.0], 4)[1].tolist() == [1, 2, 4, 5]   # -0 is +0: the earlier one first
    assert run([-1, nan, inf, -inf, -0.0, 0.0], 3)[1].tolist() == [1, 2, 4]
    # the values are the stored bits
    got = run([-1, nan, inf, -inf, -0.0, 0.0], 4)[2].view(np.uint32).tolist()
    assert got == np.array([nan, inf, -0.0, 0.0], np.float32).view(np.uint32).tolist()
    # the diagonal: row 0's entry in column 0 is weakest and still kept, as one of the K
    sq = R.sample_neighbors(np.array([0, 4, 4, 4, 4]), np.array([0, 1, 2, 3], np.int32),
                            np.array([1, 5, 7, 6], np.float32), 4, 2, by="strongest")
    assert sq[1].tolist() == [0, 2] and sq[0].tolist() == [0, 2, 2, 2, 2]
    off = R.sample_neighbors(np.array([0, 4, 4, 4, 4]), np.array([0, 1, 2, 3], np.int32),
                             np.array([1, 5, 7, 6], np.float32), 4, 2, by="strongest", keep_diagonal=False)
    assert off[1].tolist() == [2, 3]
    # rescale: S = 19, S' = 8, ratio = fp32(19 / 8)
    res = R.sample_neighbors(np.array([0, 4, 4, 4, 4]), np.array([0, 1, 2, 3], np.int32),
                             np.array([1, 5, 7, 6], np.float32), 4, 2, by="strongest", rescale="sum")
    assert res[2].tolist() == [np.float32(19 / 8), np.float32(7) * np.float32(19 / 8)]
    zero = R.sample_neighbors(np.array([0, 3]), np.array([0, 1, 2], np.int32), np.array([0, 0, 0], np.float32), 3, 2,
                              by="weight", seed=5, keep_diagonal=False, rescale="sum")
    assert zero[1].tolist() == [0, 1] and zero[2].tolist() == [0, 0]    # zeros by lowest position; S' = 0: untouched


@pytest.mark.parametrize("by", R.MODES)
def test_sampling_a_row_list_is_taking_rows_of_the_sample(by):
    degrees = [0, 1, 5, 9, 3, 40, 7, 7, 0, 12]
    rowptr, col, val = _graph(degrees, 64, 3)
    rows = np.array([9, 2, 2, 5, 0, 3, 5, 8])
    for K, rescale in ((1, None), (4, "sum"), (7, None)):
        kw = dict(by=by, seed=11, stream=2, keep_diagonal=False, rescale=rescale)
        whole = R.sample_neighbors(rowptr, col, val, 64, K, **kw)
        R.assert_same(R.sample_neighbors(rowptr, col, val, 64, K, rows=rows, **kw), R.take_rows(*whole, rows), by)
        assert np.diff(whole[0]).tolist() == [min(d, K) for d in degrees]
        for r in range(len(degrees)):                                  # ascending columns stay ascending, a subset
            c = whole[1][whole[0][r]:whole[0][r + 1]]
            assert np.all(np.diff(c) > 0) and set(c.tolist()) <= set(col[rowptr[r]:rowptr[r + 1]].tolist())


# ------------------------------------------------------------------------------------------------ the law of the draw
ROWS, DEG = 4096, 8


def _draws(by, K, values):
    rowptr = np.arange(ROWS + 1, dtype=np.int64) * DEG
    col = np.tile(np.arange(DEG, dtype=np.int32), ROWS)
    val = np.tile(np.asarray(values, np.float32), ROWS)
    rp, c, _ = R.sample_neighbors(rowptr, col, val, DEG, K, by=by, seed=42, stream=0, keep_diagonal=False)
    assert np.all(np.diff(rp) == K)
    return c.reshape(ROWS, K)


def _z(count, q):
    return abs(count / ROWS - q) / np.sqrt(q * (1 - q) / ROWS)


def test_uniform_draws_every_subset_equally_often():
    kept = _draws("uniform", 3, np.ones(DEG))
    single = max(_z(int((kept == j).sum()), 3 / 8) for j in range(DEG))
    pairs = max(_z(int(((kept == a).any(1) & (kept == b).any(1)).sum()), 3 * 2 / (8 * 7))
                for a, b in itertools.combinations(range(DEG), 2))
    print(f"uniform K=3: single {single:.2f} sigma, pairs {pairs:.2f} sigma")
    assert single <= 4.0 and pairs <= 4.5


def test_weight_draws_follow_plackett_luce():
    values = np.arange(1, DEG + 1, dtype=np.float64)
    p = values / values.sum()
    first = _draws("weight", 1, values)
    single = max(_z(int((first == j).sum()), p[j]) for j in range(DEG))
    two = _draws("weight", 2, values)
    pairs = max(_z(int(((two == a).any(1) & (two == b).any(1)).sum()),
                   p[a] * p[b] / (1 - p[a]) + p[a] * p[b] / (1 - p[b]))
                for a, b in itertools.combinations(range(DEG), 2))
    print(f"weight: K=1 single {single:.2f} sigma, K=2 pairs {pairs:.2f} sigma")
    assert single <= 4.0 and pairs <= 4.5
