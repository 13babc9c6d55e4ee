"""Neighbour sampling — a fan-out for the rows of a prepared adjacency.

  sample_neighbors(graph, K)      every row keeps at most K of its stored entries, redrawn per (seed, stream):
                                  GraphSAGE-style sampling, DropEdge as its special case.

The receptive field of a set of loss rows (`model(x, adj, rows=idx, restrict_forward=True)`) is set by the longest
rows it touches: one hub pulls in everything the hub touches.  A fan-out bounds that.  The rule is stated in
include/gcn_spmm.h, "Neighbour sampling"; the kernels are pygcn_amd/csrc/gcn_sample.hip (`gcn_csr_sample_rows`): a
per-row select with no sort and no workspace, bitwise reproducible, whose keys depend on (seed, stream, entry index)
only — so `g.sample_neighbors(K, seed=s, rows=R)` is, bit for bit, `g.sample_neighbors(K, seed=s).take_rows(R)`.

This module is the launcher: argument checks, the scan of min(d, K) with torch ops, the allocation, one call."""
import torch

from . import _native
from .graph import CSRGraph
from .spmm import next_dropout_seed

MODES = {"uniform": _native.GCN_SAMPLE_UNIFORM, "weight": _native.GCN_SAMPLE_WEIGHT,
         "strongest": _native.GCN_SAMPLE_STRONGEST}
RESCALES = {None: _native.GCN_SAMPLE_RESCALE_NONE, "sum": _native.GCN_SAMPLE_RESCALE_SUM}


def sample_neighbors(graph, fanout, by="uniform", seed=None, stream=0, rows=None, keep_diagonal=None, rescale=None,
                     _rowptr_is64=None):
    """`CSRGraph.sample_neighbors` (documented there).  `_rowptr_is64` forces a 64-bit row pointer on the result."""
    if not isinstance(graph, CSRGraph):
        raise RuntimeError(f"sample_neighbors: expected a CSRGraph, got {type(graph)}")
    K = int(fanout)
    if K < 1:
        raise RuntimeError(f"sample_neighbors: fanout must be at least 1, got {fanout}")
    if by not in MODES:
        raise RuntimeError(f'sample_neighbors: by must be "uniform", "weight" or "strongest", got {by!r}')
    if rescale not in RESCALES:
        raise RuntimeError(f'sample_neighbors: rescale must be None or "sum", got {rescale!r}')
    stream = int(stream)
    if not 0 <= stream < 2 ** 32:
        raise RuntimeError(f"sample_neighbors: stream must lie in [0, 2^32), got {stream}")
    square = graph.shape[0] == graph.shape[1]
    if keep_diagonal is None:
        keep_diagonal = square
    elif keep_diagonal and not square:
        raise RuntimeError(f"sample_neighbors: keep_diagonal needs a square matrix, got {graph.shape}")
    dev, rp = graph.device, graph.rowptr
    if rows is not None:
        rows = torch.as_tensor(rows).to(device=dev, dtype=torch.int64).contiguous()
        if rows.dim() != 1:
            raise RuntimeError("sample_neighbors: rows must be a 1-D index list")
        if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= graph.shape[0]):
            raise RuntimeError("sample_neighbors: row index out of range")
    m = graph.shape[0] if rows is None else int(rows.numel())
    if seed is None:           # (the strongest entries are no draw: the generator is left alone)
        seed = next_dropout_seed(dev) if by != "strongest" else 0
    # rowptr_out needs no pass over the entries: it is the scan of min(d, K)
    rp_out = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    if m:
        d = (rp[1:] - rp[:-1]) if rows is None else (rp[rows + 1] - rp[rows])
        torch.cumsum(d.to(torch.int64).clamp_(max=K), 0, out=rp_out[1:])
    total = int(rp_out[-1])    # one 8-byte read: the number of kept entries
    if total < 2 ** 31 - 1 and not _rowptr_is64:
        rp_out = rp_out.to(torch.int32)
    col_out = torch.empty(total, dtype=torch.int32, device=dev)
    val_out = torch.empty(total, dtype=torch.float32, device=dev)
    if total:
        _native.launch("gcn_csr_sample_rows", dev, rp.data_ptr(), int(rp.dtype == torch.int64), graph.col.data_ptr(),
                       graph.val.data_ptr(), rows.data_ptr() if rows is not None else None, m, K, MODES[by],
                       int(seed) & 0xFFFFFFFFFFFFFFFF, stream, int(bool(keep_diagonal)), RESCALES[rescale],
                       rp_out.data_ptr(), int(rp_out.dtype == torch.int64), col_out.data_ptr(), val_out.data_ptr())
    return CSRGraph(rp_out, col_out, val_out, (m, graph.shape[1]), item_cost=graph.item_cost,
                    long_thresh=graph.long_thresh, validate=False)
