"""Neighbour sampling on the MI355X (`gcn_csr_sample_rows`, pygcn_amd/csrc/gcn_sample.hip; CSRGraph.sample_neighbors).

Row pointer, columns and values of every sample are compared BIT FOR BIT with the numpy restatement
tests/_neighbor_ref.py.  Two remarks on "bit for bit":
  * rescale="sum" adds doubles, on the device in a fixed order of its own.  The test values are k / 4096 with
    1 <= k < 4096, so every such sum is exact in double, in any order, and the ratio fp32(S / S') has one value.
  * by="weight" takes a double-precision logarithm on either side; the race key is that quotient rounded to fp32,
    which hides the last bits of the logarithm (tests/test_select_gpu.py measures the same formula: at most one fp32
    step on fewer than 1e-4 of the keys), and a choice changes only where two keys of one row are that close.

The kernel has two row classes — up to GCN_SAMPLE_WAVE_ROW_MAX = 253 entries one wavefront holds the row, longer rows
take a workgroup that walks them in chunks of 1024 entries — so the ladder has 252 .. 257 and 1020 .. 1028 beside the
degrees the issue lists.  The law of the draw is checked on the restatement (tests/test_neighbor_sampling_cpu.py)."""
import gc
import os
import re
import subprocess
import sys
import weakref

import numpy as np
import pytest
import torch

import _neighbor_ref as R
import inputs as gin
from conftest import ROOT, assert_normwise, assert_parity

pytestmark = pytest.mark.gpu
TOL = 1e-5
FANOUTS = (1, 2, 10, 64, 300)
N_LADDER = 20011


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _device_graph(csr, shape, dev, rowptr_dtype=torch.int32):
    from pygcn_amd import CSRGraph
    rowptr, col, val = csr
    return CSRGraph(torch.from_numpy(np.asarray(rowptr, np.int64)).to(dev).to(rowptr_dtype),
                    torch.from_numpy(np.asarray(col, np.int32)).to(dev),
                    torch.from_numpy(np.asarray(val, np.float32)).to(dev), shape)


def _arrays(g):
    return g.rowptr.cpu().numpy(), g.col.cpu().numpy(), g.val.cpu().numpy()


def _summable(rng, size):
    return (rng.integers(1, 4096, size) / 4096.0).astype(np.float32)


def _rows_graph(rows, degrees, n, seed, with_diagonal=None, values=_summable):
    """An n x n CSR matrix whose row rows[i] has degrees[i] random ascending columns (the other rows are empty);
    with_diagonal[i] = True / False puts column rows[i] into the row / keeps it out."""
    rng = np.random.default_rng(seed)
    lens = np.zeros(n, np.int64)
    lens[np.asarray(rows)] = degrees
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=rowptr[1:])
    parts = []
    for i in np.argsort(rows).tolist():
        r, d = int(rows[i]), int(degrees[i])
        c = rng.choice(n, d, replace=False)
        if with_diagonal is not None and d:
            if with_diagonal[i] and r not in c:
                c[0] = r
            elif not with_diagonal[i] and r in c:
                taken = set(c.tolist())
                c[c == r] = next(x for x in range(n) if x not in taken)
        parts.append(np.sort(c))
    col = np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
    return rowptr, col, values(rng, col.size)


# ------------------------------------------------------------------------------------------------ the degree ladder
LADDER = sorted({0, 1, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097, 20000}               # the issue's
                | {k + s for k in FANOUTS for s in (-1, 0, 1)}                             # K - 1, K, K + 1
                | {252, 253, 254}                                                          # wavefront | workgroup rows
                | {1020, 1021, 1024, 1027, 1028, 2047, 2049})                              # one chunk | two | three


@pytest.fixture(scope="module")
def ladder(dev):
    """Every degree of LADDER twice over 20 011 columns: once with the row's diagonal entry, once without."""
    degrees = np.array(LADDER + LADDER)
    rows = 5 + 333 * np.arange(degrees.size)
    assert rows.max() < N_LADDER and degrees.size == 2 * len(LADDER)
    with_diag = np.arange(degrees.size) < len(LADDER)
    csr = _rows_graph(rows, degrees, N_LADDER, 1, with_diag)
    starts = csr[0][rows]
    assert {int(s) & 3 for s in starts} == {0, 1, 2, 3}                # every alignment of a row's first quad
    return csr, _device_graph(csr, (N_LADDER, N_LADDER), dev)


@pytest.mark.parametrize("by", R.MODES)
@pytest.mark.parametrize("K", FANOUTS)
def test_degree_ladder(ladder, K, by):
    csr, g = ladder
    for keep_diagonal in (True, False):
        for rescale in (None, "sum"):
            kw = dict(by=by, seed=42, stream=3, keep_diagonal=keep_diagonal, rescale=rescale)
            got = g.sample_neighbors(K, **kw)
            assert got.shape == (N_LADDER, N_LADDER) and got.rowptr.dtype == torch.int32
            assert got.item_cost == g.item_cost and got.long_thresh == g.long_thresh
            R.assert_same(_arrays(got), R.sample_neighbors(*csr, N_LADDER, K, **kw), f"K={K} {by} {kw}")
    assert np.diff(_arrays(got)[0]).max() == min(K, 20000)


# ------------------------------------------------------------------------------------------------ many short rows
@pytest.fixture(scope="module")
def many_rows(dev):
    """65 536 + 300 rows of degree 0 .. 12: more than GCN_SAMPLE_WAVE_SWEEP_ROWS = 65 536, the rows one sweep of the
    row-per-wavefront grid (16 384 workgroups of four wavefronts) covers — the last 300 rows are a second stride."""
    from pygcn_amd import _native
    n = _native.GCN_SAMPLE_WAVE_SWEEP_ROWS + 300
    rng = np.random.default_rng(2)
    lens = rng.integers(0, 13, n)
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=rowptr[1:])
    row_of = np.repeat(np.arange(n), lens)
    step = np.cumsum(rng.integers(1, 5, row_of.size))
    first = np.clip(row_of - 20, 0, n - 64)                              # columns near the diagonal: some rows hit it
    col = first + step - np.repeat(step[np.minimum(rowptr[:-1], step.size - 1)], lens) + 1
    assert col.min() >= 0 and col.max() < n and np.all((np.diff(col) > 0) | (np.diff(row_of) > 0))
    assert 0.01 < (col == row_of).mean() < 0.5
    csr = rowptr, col.astype(np.int32), _summable(rng, col.size)
    return n, csr, _device_graph(csr, (n, n), dev)


@pytest.mark.parametrize("by", R.MODES)
def test_more_rows_than_one_sweep_of_the_wave_grid(many_rows, by):
    n, csr, g = many_rows
    kw = dict(by=by, seed=7, stream=1, rescale="sum")                    # (square: the diagonal is kept)
    R.assert_same(_arrays(g.sample_neighbors(5, **kw)), R.sample_neighbors(*csr, n, 5, **kw), by)


# ------------------------------------------------------------------------------------------------ row pointer widths
@pytest.mark.parametrize("out64", [False, True], ids=["out32", "out64"])
@pytest.mark.parametrize("in64", [False, True], ids=["in32", "in64"])
def test_wide_row_pointers(dev, in64, out64):
    from pygcn_amd.sampling import sample_neighbors
    n = 400
    degrees = np.array([0, 1, 2, 7, 8, 9, 100, 253, 254, 300, 399])
    csr = _rows_graph(3 + 36 * np.arange(degrees.size), degrees, n, 3)
    g = _device_graph(csr, (n, n), dev, torch.int64 if in64 else torch.int32)
    rows = np.array([363, 3, 3, 39, 255, 291, 0, 327])
    for by in R.MODES:
        for r in (None, rows):
            kw = dict(by=by, seed=9, rows=r, keep_diagonal=True, rescale="sum")
            got = sample_neighbors(g, 8, _rowptr_is64=out64, **kw)
            assert got.rowptr.dtype == (torch.int64 if out64 else torch.int32)
            assert got.shape == (n if r is None else len(rows), n)
            R.assert_same(_arrays(got), R.sample_neighbors(*csr, n, 8, **kw), f"{by} rows={r is not None}")


# ------------------------------------------------------------------------------------------------ ties
DEGREES_TIES = np.array([5, 70, 253, 254, 300, 1500])


def test_strongest_on_two_values_keeps_the_lowest_positions(dev):
    two = lambda rng, size: rng.choice(np.array([0.25, 0.5], np.float32), size)  # noqa: E731
    n = 1600
    rows = 11 + 200 * np.arange(DEGREES_TIES.size)
    csr = _rows_graph(rows, DEGREES_TIES, n, 4, values=two)
    g = _device_graph(csr, (n, n), dev)
    for K in (3, 64, 200):
        got = _arrays(g.sample_neighbors(K, by="strongest", keep_diagonal=False))
        R.assert_same(got, R.sample_neighbors(*csr, n, K, by="strongest", keep_diagonal=False), f"K={K}")
        for r, d in zip(rows.tolist(), DEGREES_TIES.tolist()):
            if d > K:                                                    # spelled out: the halves first, by position
                v, c = csr[2][csr[0][r]:csr[0][r + 1]], csr[1][csr[0][r]:csr[0][r + 1]]
                halves, quarters = np.flatnonzero(v == 0.5), np.flatnonzero(v == 0.25)
                want = np.sort(np.concatenate([halves[:K], quarters[:max(0, K - halves.size)]]))
                assert np.array_equal(got[1][got[0][r]:got[0][r + 1]], c[want]), (K, r)


def test_strongest_follows_the_selection_order_on_special_values(dev):
    bits = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800123, 0xBF800000,
                     0x3F800000, 0xC0000000, 0x00000001, 0x80000001], np.uint32)      # +-0, +-inf, four NaNs, +-1, ...
    special = lambda rng, size: rng.choice(bits, size).view(np.float32)  # noqa: E731
    n = 1600
    rows = 11 + 200 * np.arange(DEGREES_TIES.size)
    csr = _rows_graph(rows, DEGREES_TIES, n, 5, values=special)
    g = _device_graph(csr, (n, n), dev)
    for K in (4, 100):
        for keep_diagonal in (False, True):
            kw = dict(by="strongest", keep_diagonal=keep_diagonal)
            R.assert_same(_arrays(g.sample_neighbors(K, **kw)), R.sample_neighbors(*csr, n, K, **kw), f"K={K}")


def test_weight_takes_zeros_last_and_by_lowest_position(dev):
    def mostly_zero(rng, size):
        v = np.zeros(size, np.float32)
        v[rng.choice(size, size // 40, replace=False)] = _summable(rng, size // 40)
        return v
    n = 1600
    rows = 11 + 200 * np.arange(DEGREES_TIES.size)
    csr = _rows_graph(rows, DEGREES_TIES, n, 6, values=mostly_zero)
    positive = [int((csr[2][csr[0][r]:csr[0][r + 1]] > 0).sum()) for r in rows.tolist()]
    assert max(positive) < 64 and positive[-1] > 10
    g = _device_graph(csr, (n, n), dev)
    for K in (10, 64):
        for rescale in (None, "sum"):
            kw = dict(by="weight", seed=21, keep_diagonal=False, rescale=rescale)
            got = _arrays(g.sample_neighbors(K, **kw))
            R.assert_same(got, R.sample_neighbors(*csr, n, K, **kw), f"K={K} {rescale}")
        for r, d, pos in zip(rows.tolist(), DEGREES_TIES.tolist(), positive):
            if d > K > pos:                                              # every positive entry, then the first zeros
                v, c = csr[2][csr[0][r]:csr[0][r + 1]], csr[1][csr[0][r]:csr[0][r + 1]]
                want = np.sort(np.concatenate([np.flatnonzero(v > 0), np.flatnonzero(v == 0)[:K - pos]]))
                assert np.array_equal(got[1][got[0][r]:got[0][r + 1]], c[want]), (K, r)


# ------------------------------------------------------------------------------------------------ against from_dense
@pytest.mark.parametrize("K", [1, 7, 40])
def test_strongest_is_from_dense_with_keep_per_row(dev, K):
    from pygcn_amd import CSRGraph
    n = 300
    rng = np.random.default_rng(8)
    dense = np.where(rng.random((n, n)) < 0.3, rng.integers(1, 64, (n, n)) / 64.0, 0.0).astype(np.float32)
    dense[5] = 0
    dense[6, 17:17 + K] = 0.5
    dense[6, :17] = 0
    dense[6, 17 + K:] = 0
    g = CSRGraph.from_dense(torch.from_numpy(dense).to(dev))
    want = CSRGraph.from_dense(g.to_dense(), keep_per_row=K)
    got = g.sample_neighbors(K, by="strongest", keep_diagonal=False)
    R.assert_same(_arrays(got), _arrays(want), f"K={K}")
    assert int(np.diff(_arrays(got)[0]).max()) == K


# ------------------------------------------------------------------------------------------------ rows, streams, seeds
@pytest.fixture(scope="module")
def small(dev):
    n = 400
    degrees = np.array([0, 1, 2, 7, 8, 9, 100, 253, 254, 300, 399])
    csr = _rows_graph(3 + 36 * np.arange(degrees.size), degrees, n, 3)
    return n, csr, _device_graph(csr, (n, n), dev)


@pytest.mark.parametrize("by", R.MODES)
def test_sampling_a_row_list_is_taking_rows_of_the_sample(small, dev, by):
    n, csr, g = small
    rows = torch.tensor([363, 3, 3, 39, 255, 291, 0, 327, 363, 219], device=dev)
    for K, rescale in ((1, None), (8, "sum"), (260, "sum")):
        kw = dict(by=by, seed=5, stream=9, rescale=rescale)
        part, whole = g.sample_neighbors(K, rows=rows, **kw), g.sample_neighbors(K, **kw).take_rows(rows)
        assert part.shape == whole.shape == (rows.numel(), n)
        R.assert_same(_arrays(part), _arrays(whole), f"{by} K={K}")
    with pytest.raises(RuntimeError, match="out of range"):
        g.sample_neighbors(3, rows=torch.tensor([0, n], device=dev))
    empty = g.sample_neighbors(3, rows=torch.zeros(0, dtype=torch.int64, device=dev))
    assert empty.shape == (0, n) and empty.nnz == 0


def test_streams_seeds_and_the_generator(small, dev):
    from pygcn_amd.functional import sample_neighbors
    n, csr, g = small
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(_arrays(a), _arrays(b)))  # noqa: E731
    for by in ("uniform", "weight"):
        a = g.sample_neighbors(8, by=by, seed=1, stream=0)
        assert same(a, g.sample_neighbors(8, by=by, seed=1, stream=0))                # the same draw, bit for bit
        assert not same(a, g.sample_neighbors(8, by=by, seed=1, stream=1))
        assert not same(a, g.sample_neighbors(8, by=by, seed=2, stream=0))
        assert np.array_equal(_arrays(a)[0], _arrays(g.sample_neighbors(8, by=by, seed=2))[0])
        torch.manual_seed(5)
        first, second = g.sample_neighbors(8, by=by), g.sample_neighbors(8, by=by)
        torch.manual_seed(5)
        assert same(first, g.sample_neighbors(8, by=by)) and not same(first, second)   # seed=None: torch's generator
    strong = g.sample_neighbors(8, by="strongest", seed=1, stream=0)
    assert same(strong, g.sample_neighbors(8, by="strongest", seed=99, stream=7))      # no draw: both ignored
    state = torch.cuda.get_rng_state(dev)
    g.sample_neighbors(8, by="strongest")
    assert torch.equal(state, torch.cuda.get_rng_state(dev))                           # ... and the generator left alone
    r, c, v = g.coo()
    sparse = torch.sparse_coo_tensor(torch.stack([r, c]), v, (n, n)).coalesce()
    assert same(sample_neighbors(sparse, 8, seed=1), g.sample_neighbors(8, seed=1))    # through as_graph
    rect = _device_graph((csr[0][:11], csr[1][:csr[0][10]], csr[2][:csr[0][10]]), (10, n), dev)
    assert rect.sample_neighbors(1, seed=1).shape == (10, n)                           # not square: no diagonal rule
    with pytest.raises(RuntimeError, match="square"):
        rect.sample_neighbors(1, keep_diagonal=True)


# ------------------------------------------------------------------------------------------------ end to end
def _step_against_the_oracle(oracle, model, x, graph, a, labels, idx, restrict):
    dev = x.device
    idx_t = torch.from_numpy(idx).to(dev)
    model.train()
    model.zero_grad()
    out_rows = model(x, graph, rows=idx_t, restrict_forward=True) if restrict else model(x, graph, rows=idx_t)
    loss = torch.nn.functional.nll_loss(out_rows, torch.from_numpy(labels).to(dev)[idx_t])
    loss.backward()
    p = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    ref_loss, fw, grads, _ = oracle.gcn2_loss_backward(x.cpu().numpy(), a, p, labels, idx)
    _, _, grads64 = oracle.gcn2_loss_backward_f64(x.cpu().numpy(), a, p, labels, idx, relu_mask=fw["h1"] > 0)
    assert_normwise(out_rows.detach().cpu(), fw["logp"][idx], TOL, "selected rows")
    assert abs(loss.item() - ref_loss) <= TOL * abs(ref_loss)
    for k, v in grads.items():
        mod, name = k.split(".")
        got = getattr(getattr(model, mod), name).grad
        assert got is not None and torch.isfinite(got).all(), k
        assert_parity(got.cpu(), v, grads64[k], k + ".grad")


@pytest.mark.parametrize("restrict", [False, True], ids=["rows", "restricted"])
def test_cora_step_on_a_sampled_graph(oracle, dev, restrict):
    """1433 -> 16 -> 7 on the committed Cora graph cut to a fan-out of 4 (the diagonal kept, rows rescaled to their
    sum): the device's sample is the restatement's — pattern bit for bit, the values to one fp32 step, since the row
    sums of 1 / d are not exact — and the step through it is the oracle's step on the restated graph."""
    from pygcn_amd import GCN
    from pygcn_amd import fused
    from pygcn_amd.utils import load_data
    idx = load_data()[3].numpy()
    npz = np.load(gin.__file__.replace("inputs.py", "cora_graph.npz"))
    a = oracle.cora_adjacency(npz["edges"], int(npz["n"]))
    n = a.shape[0]
    csr = (a.rowptr, a.col, a.val)
    g = _device_graph(csr, (n, n), dev)
    kw = dict(seed=1, rescale="sum")
    want = R.sample_neighbors(*csr, n, 4, **kw)
    gs = g.sample_neighbors(4, **kw)
    got = _arrays(gs)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    steps = np.abs(got[2].view(np.int32).astype(np.int64) - want[2].view(np.int32).astype(np.int64))
    assert int(steps.max()) <= 1
    assert int(np.diff(want[0]).max()) == 4 < int(np.diff(a.rowptr).max())
    sums = np.add.reduceat(got[2].astype(np.float64), got[0][:-1].astype(np.int64))
    assert np.abs(sums - 1).max() < 1e-6                                 # row-normalised stays row-normalised
    restated = oracle.CSR(*want, (n, n))
    x = torch.from_numpy(gin.cora_features()).to(dev)
    torch.manual_seed(42)
    model = GCN(1433, 16, 7, dropout=0.0).to(dev)
    _step_against_the_oracle(oracle, model, x, gs, restated, gin.cora_labels(), idx, restrict)
    # a fresh graph per step is released with its row sets: nothing but the caller holds it
    assert gs in fused._ROWSETS
    alive = weakref.ref(gs)
    model.zero_grad()
    del gs
    gc.collect()
    assert alive() is None


# ------------------------------------------------------------------------------------------------ the training script
def _train(*flags):
    r = subprocess.run([sys.executable, "train.py", "--epochs", "3", *flags], cwd=os.path.join(ROOT, "pygcn_amd"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [re.sub(r" time: [\d.]+s", "", ln) for ln in r.stdout.splitlines() if ln.startswith(("Epoch:", "Test set"))]
    assert len(lines) == 4 and "Optimization Finished!" in r.stdout, r.stdout[-2000:]
    return lines


PLAIN = []


def _plain():
    if not PLAIN:
        PLAIN.append(_train())
    return PLAIN[0]


def test_train_script_without_the_flag_is_unchanged(dev):
    """Two runs of `python train.py --epochs 3`: one never enters the flag's code path; the other samples every
    epoch with a fan-out above the largest degree, which cuts nothing — the sample is the graph, its arrays copied —
    and draws nothing from torch's generator (the seed is the run's).  The printed lines are the same."""
    assert _train("--fanout", "100000") == _plain()


@pytest.mark.parametrize("flags", [(), ("--restrict_forward",)], ids=["full", "restrict_forward"])
def test_train_script_with_a_fanout(dev, flags):
    sampled = _train("--fanout", "4", *flags)
    assert sampled != _plain()
    for ln in sampled:
        numbers = re.findall(r"[:=] *([-+]?\d+\.\d+|nan|inf)", ln)
        assert numbers and all(np.isfinite(float(v)) for v in numbers), ln
