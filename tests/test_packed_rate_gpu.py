"""The packed layer-2 route after its kernels went through LDS: `pack512_kernel` builds a row's slot in
a wave-private LDS image and stores it whole, several rows per wave; `spmm_wide_packed_kernel` stages each gathered
slot in a wave-private LDS copy and reads the mask and the lane's value words from there.  Both must stay what they
were: the pack against the NumPy reference of the format (tests/_pack512_ref.py) at every row count around a wave's
and a block's share of rows, the packed SpMM against the dense launch bit for bit — on inputs that are first shown,
with NumPy, to hold the cases the expansion can get wrong."""
import os
import re

import numpy as np
import pytest
import torch

import _pack512_ref as ref512

pytestmark = pytest.mark.gpu

CAP = ref512.CAPACITY
_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pygcn_amd", "csrc", "gcn_pack.hip")
R = int(re.search(r"#define GCN_PACK512_ROWS_PER_WAVE (\d+)", open(_SRC).read()).group(1))     # rows per wave pass
B = 4 * R                                                                                       # rows per block


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _sparse_rows(m, density, seed):
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((m, 256)).astype(np.float32)
    if density < 1.0:
        h[rng.random((m, 256)) >= density] = 0.0
    return h


def _check_pack(h, H):
    """Device slots of H (a device view of `h`) against the reference: every defined word, the overflow marks, the
    expansion bit for bit (rows that overflowed: the stored part)."""
    from pygcn_amd.spmm import rows_pack512
    want, written, want_ovf = ref512.pack(h)
    got = rows_pack512(H).slots.cpu().numpy().view(np.uint32)
    assert got.shape == want.shape
    assert np.array_equal(got[written], want[written]), "a defined word differs"
    back, ovf = ref512.expand(np.where(written, got, 0))
    assert np.array_equal(ovf, want_ovf), "overflow marks"
    bits, hb = back.view(np.uint32), h.view(np.uint32)
    assert np.array_equal(bits[~ovf], hb[~ovf]), "expansion of a row that fits"
    ref_back, _ = ref512.expand(want)
    assert np.array_equal(bits[ovf], ref_back.view(np.uint32)[ovf]), "stored part of an overflowed row"
    return want_ovf


ROW_COUNTS = sorted({1, R - 1, R, R + 1, B - 1, B, B + 1, 2 * B + 1} - {0})


@pytest.mark.parametrize("density", [0.0, 0.25, 1.0])
@pytest.mark.parametrize("m", ROW_COUNTS)
def test_pack_around_a_wave_and_a_block_of_rows(dev, m, density):
    h = _sparse_rows(m, density, 7000 * m + int(100 * density))
    ovf = _check_pack(h, torch.from_numpy(h).to(dev))
    assert ovf.all() if density == 1.0 else not ovf.any() if density == 0.0 else True


@pytest.mark.parametrize("m", ROW_COUNTS)
def test_pack_special_rows_at_every_place_in_a_wave(dev, m):
    """The format's edge rows (capacity, one over, all set, -0.0 / NaN / inf, empty), rotated by m so that each of
    them meets every place among a wave's rows, in a buffer of m + 12 rows."""
    s, _ = ref512.special_rows()
    h = np.concatenate([_sparse_rows(m, 0.25, m), np.roll(s, m, axis=0)])
    _check_pack(h, torch.from_numpy(h).to(dev))


@pytest.mark.parametrize("m", [1, R + 1, 2 * B + 1])
def test_pack_reads_rows_at_their_pitch(dev, m):
    h = _sparse_rows(m, 0.25, 40 + m)
    buf = torch.full((m, 320), 7.0, device=dev)
    buf[:, :256] = torch.from_numpy(h).to(dev)
    H = buf[:, :256]
    assert H.stride(0) == 320
    _check_pack(h, H)


# ------------------------------------------------------------------ packed SpMM against the dense launch
def _nibble_rows():
    """Four rows whose quarters hold, nibble by nibble, the patterns 0..7 / 8..15 behind an even number of earlier
    values, and the same behind one more value (a leading nibble 0001)."""
    rows = np.zeros((4, 256), np.float32)
    val = 1.0
    for r, (lead, pats) in enumerate([(0, range(8)), (0, range(8, 16)), (1, range(8)), (1, range(8, 16))]):
        for q in range(4):
            cols = ref512.quarter_columns(q)
            seq = ([1] if lead else []) + list(pats)
            for cb, pat in enumerate(seq):
                for j in range(4):
                    if (pat >> j) & 1:
                        rows[r, cols[4 * cb + j]] = val
                        val += 1.0
    return rows


BUILT = 9


def _hidden(n, seed):
    """[n, 256]: thirds at densities 0.02 / 0.25 / 0.44 (relu-like, non-negative); the last BUILT rows are built by
    hand.  Returns the rows and the names of the built ones."""
    rng = np.random.default_rng(seed)
    h = np.concatenate([np.abs(_sparse_rows(n // 3, 0.02, seed)), np.abs(_sparse_rows(n // 3, 0.25, seed + 1)),
                        np.abs(_sparse_rows(n - 2 * (n // 3), 0.44, seed + 2))])
    names = {}

    def fill(r, q, k):
        h[r] = 0.0
        h[r, ref512.quarter_columns(q)[np.sort(rng.permutation(64)[:k])]] = rng.random(k).astype(np.float32) + 0.5
    b = n - BUILT
    fill(b, 1, CAP); names["29 in quarter 1"] = b
    fill(b + 1, 3, CAP + 1); names["30 in quarter 3"] = b + 1
    h[b + 2] = 0.0; names["all zero"] = b + 2
    h[b + 3:b + 7] = _nibble_rows(); names["nibbles"] = b + 3
    fill(b + 7, 0, 64); names["64 in quarter 0"] = b + 7
    h[b + 8] = 0.0
    for q in range(4):                                              # every quarter full to the last word
        h[b + 8, ref512.quarter_columns(q)[64 - CAP:]] = rng.random(CAP).astype(np.float32) + 0.5
    names["every quarter at 29, highest bits"] = b + 8
    return h, names


def _graph(n, seed, must, long_len=100):
    """CSR [n, n]: row 0 empty, rows 1..4 with 1, 63, 64 and 65 entries, row 5 with `long_len`, the rest 1..13; row 3
    gathers every column in `must`, and every tenth row gathers one of them alone or first."""
    rng = np.random.default_rng(seed)
    deg = np.minimum(rng.poisson(4, n), 12) + 1
    deg[:6] = [0, 1, 63, 64, 65, long_len]
    deg[n // 2] = 0
    rows = []
    for r, d in enumerate(deg):
        if d == 0:
            rows.append(np.zeros(0, np.int32))
            continue
        forced = list(must) if r == 3 else [must[(r // 10) % len(must)]] if r % 10 == 1 else []
        others = rng.permutation(np.setdiff1d(np.arange(n), forced))[: d - len(forced)]
        rows.append(np.sort(np.concatenate([forced, others])).astype(np.int32))
    rowptr = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
    col = np.concatenate(rows).astype(np.int32)
    val = (1.0 - rng.random(col.size)).astype(np.float32)
    return rowptr, col, val


@pytest.fixture(scope="module")
def case(dev):
    """The inputs of the SpMM tests, checked with NumPy to hold what they are meant to hold, and the dense launch's
    result for either row-pointer width (computed once, never written to)."""
    from pygcn_amd import CSRGraph, spmm_csr
    n = 300
    h, names = _hidden(n, 77)
    slots, written, ovf = ref512.pack(h)
    u = slots.view(np.uint32)
    # -- what the rows hold
    r = names["29 in quarter 1"]
    assert u[r, 32 + 2] == CAP and written[r, 32 + 31] and not ovf[r], "a quarter whose last value is in word 31"
    r = names["30 in quarter 3"]
    assert u[r, 96 + 2] == CAP + 1 and ovf[r]
    assert ovf[names["64 in quarter 0"]] and not h[names["all zero"]].any()
    r = names["every quarter at 29, highest bits"]
    assert all(u[r, 32 * q + 2] == CAP for q in range(4)) and not ovf[r]
    for lo, hi, d in ((0, n // 3, 0.02), (n // 3, 2 * (n // 3), 0.25), (2 * (n // 3), n - BUILT, 0.44)):
        assert abs(float((h[lo:hi] != 0).mean()) - d) < 0.02
    seen = set()                                         # (nibble pattern, parity of the earlier values) in rows that fit
    for r in np.flatnonzero(~ovf):
        for q in range(4):
            nz = (h[r, ref512.quarter_columns(q)] != 0).astype(int)
            before = np.concatenate([[0], np.cumsum(nz)])
            for cb in range(16):
                pat = int(nz[4 * cb:4 * cb + 4] @ [1, 2, 4, 8])
                seen.add((pat, int(before[4 * cb]) & 1))
    assert seen == {(p, e) for p in range(16) for e in (0, 1)}, "a nibble pattern is missing at one parity"
    built = set(range(names["nibbles"], names["nibbles"] + 4))
    assert {(int((h[r, ref512.quarter_columns(0)][4 * cb:4 * cb + 4] != 0) @ [1, 2, 4, 8])) for r in built
            for cb in range(16)} == set(range(16))
    # -- what the graph gathers
    must = sorted(set(names.values()) | set(range(names["nibbles"], names["nibbles"] + 4)))
    rowptr, col, val = _graph(n, 5, must)
    deg = np.diff(rowptr)
    assert list(deg[:6]) == [0, 1, 63, 64, 65, 100]
    gathered = np.zeros(n, bool)
    gathered[col] = True
    assert gathered[must].all() and (gathered & ovf).any() and (gathered & ~ovf).any()
    H = torch.from_numpy(h).to(dev)
    out = {}
    for is64 in (False, True):
        g = CSRGraph(torch.from_numpy(rowptr if is64 else rowptr.astype(np.int32)).to(dev),
                     torch.from_numpy(col).to(dev), torch.from_numpy(val).to(dev), (n, n), long_thresh=32)
        assert g.plan(torch.float32).n_long >= 4             # rows 2..5 are chunked at long_thresh = 32
        out[is64] = (g, spmm_csr(g, H))
    return {"h": h, "H": H, "slots": slots, "written": written, "out": out, "n": n}


@pytest.mark.parametrize("is64", [False, True])
def test_packed_spmm_is_the_dense_launch_bit_for_bit(dev, case, is64):
    from pygcn_amd import CSRGraph, spmm_csr
    from pygcn_amd.spmm import rows_pack512
    g, dense = case["out"][is64]
    P = rows_pack512(case["H"])
    got = spmm_csr(g, packed=P)
    assert torch.equal(dense.view(torch.int32), got.view(torch.int32))
    assert torch.equal(got[0], torch.zeros(256, device=dev))                 # the empty row
    again = spmm_csr(g, packed=P)                                            # the same launch twice: the same bits
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    # the default schedule too (long_thresh 256: no chunks, row 5 is a tile and a half)
    g2 = CSRGraph(g.rowptr, g.col, g.val, (case["n"], case["n"]))
    assert torch.equal(spmm_csr(g2, case["H"]), spmm_csr(g2, packed=P))


@pytest.mark.parametrize("fill", [0xFFFFFFFF, 0x7FC00000])
def test_undefined_slot_words_are_never_used(dev, case, fill):
    """Slots packed on the host, every word the format leaves undefined set to all ones / a NaN: the product does
    not change (the pack kernel leaves whatever its LDS image held in those words)."""
    from pygcn_amd import spmm_csr
    from pygcn_amd.spmm import PackedRows
    u = case["slots"].view(np.uint32).copy()
    assert (~case["written"]).any()
    u[~case["written"]] = fill
    P = PackedRows(torch.from_numpy(u.view(np.int32)).to(dev), case["H"])
    for is64 in (False, True):
        g, dense = case["out"][is64]
        assert torch.equal(dense.view(torch.int32), spmm_csr(g, packed=P).view(torch.int32))
