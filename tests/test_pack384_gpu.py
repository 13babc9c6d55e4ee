"""The pooled 384-byte packed rows on the GPU: `pack384_kernel` against the NumPy reference of the format
(tests/_pack384_ref.py) word for word on the defined words, at every row count around a wave's and a block's share of
rows and with the format's edge rows at every place in a block; `spmm_csr(g, packed=rows_pack384(H))` against the dense
launch `spmm_csr(g, H)` bit for bit, on inputs first shown with NumPy to hold what the expansion can get wrong."""
import os
import re

import numpy as np
import pytest
import torch

import _pack384_ref as ref384

pytestmark = pytest.mark.gpu

CAP = ref384.CAPACITY
_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pygcn_amd", "csrc", "gcn_pack.hip")
R = int(re.search(r"#define GCN_PACK384_ROWS_PER_WAVE (\d+)", open(_SRC).read()).group(1))     # rows per wave pass
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


def _at_pitch(h, pitch, dev):
    """A device view of `h` whose rows are `pitch` elements apart (the gaps hold 7.0)."""
    buf = torch.full((h.shape[0], pitch), 7.0, device=dev)
    buf[:, :256] = torch.from_numpy(h).to(dev)
    H = buf[:, :256]
    assert H.stride(0) == pitch or h.shape[0] == 1
    return H


def _check_pack(h, H):
    """Device slots of H (a device view of `h`) against the reference: every defined word, and the rows that fit
    come back bit for bit."""
    from pygcn_amd.spmm import rows_pack384
    want, defined, want_ovf = ref384.pack384(h)
    P = rows_pack384(H)
    assert P.slot_bytes == 384 and P.slots.data_ptr() % 128 == 0
    got = P.slots.cpu().numpy().view(np.uint32)
    assert got.shape == want.shape == (h.shape[0], 96)
    bad = np.argwhere(defined & (got != want))
    assert bad.size == 0, f"a defined word differs: (row, word) {bad[:4].tolist()}"
    back, ovf = ref384.unpack384(np.where(defined, got, 0))
    assert np.array_equal(ovf, want_ovf), "overflow marks"
    assert np.array_equal(back.view(np.uint32)[~ovf], h.view(np.uint32)[~ovf]), "a row that fits"
    return want_ovf


ROW_COUNTS = sorted({1, R, R + 1, B - 1, B, B + 1, 2 * B + 1})


@pytest.mark.parametrize("density", [0.0, 0.25, 1.0])
@pytest.mark.parametrize("m", ROW_COUNTS)
def test_pack_around_a_wave_and_a_block_of_rows(dev, m, density):
    h = _sparse_rows(m, density, 7000 * m + int(100 * density))
    for pitch in (256, 260, 320):
        ovf = _check_pack(h, _at_pitch(h, pitch, dev))
        assert ovf.all() if density == 1.0 else not ovf.any() if density == 0.0 else True


@pytest.mark.parametrize("offset", range(B))
def test_pack_edge_rows_at_every_place_in_a_block(dev, offset):
    """Totals 86 / 87 / 88, (64, 0, 0, 23), (0, 0, 23, 64), all set, all zero, -0.0 / NaN / inf / denormals: behind
    `offset` other rows, so that each of them meets every place among a wave's rows and every wave of a block."""
    s, names = ref384.special_rows()
    h = np.concatenate([_sparse_rows(offset, 0.25, offset), s, _sparse_rows(1, 0.25, 99)])
    ovf = _check_pack(h, torch.from_numpy(h).to(dev))
    assert set(np.flatnonzero(ovf) - offset) >= {names["total 88"], names["all set"], names["all -0.0"]}
    assert not ovf[offset + names["total 87"]]


# ------------------------------------------------------------------ the gather against the dense launch
N_NIBBLE = 64


def _nibble_rows():
    """64 rows that fit.  Row (r, s) holds, in every quarter q, the four nibbles of lanes i = s, s + 4, s + 8, s + 12
    with the pattern (r + i + 3 q) mod 16: over r = 0..15 every pattern meets every lane of every quarter, and of the
    four patterns v, v + 4, v + 8, v + 12 of a quarter at most one is empty, so quarters 1..3 begin behind a prefix."""
    rows = np.zeros((N_NIBBLE, 256), np.float32)
    val = 1.0
    for r in range(16):
        for s in range(4):
            for q in range(4):
                cols = ref384.quarter_columns(q)
                for i in range(s, 16, 4):
                    for j in range(4):
                        if ((r + i + 3 * q) % 16 >> j) & 1:
                            rows[4 * r + s, cols[4 * i + j]] = val
                            val += 1.0
    return rows


def _hidden(n, seed):
    """[n, 256]: thirds at densities 0.02 / 0.25 / 0.44 (relu-like; the last third overflows), then the format's edge
    rows, then the nibble rows.  Returns the rows, the edge rows' places and the first nibble row."""
    s, names = ref384.special_rows()
    k = n - s.shape[0] - N_NIBBLE
    h = np.concatenate([np.abs(_sparse_rows(k // 3, 0.02, seed)), np.abs(_sparse_rows(k // 3, 0.25, seed + 1)),
                        np.abs(_sparse_rows(k - 2 * (k // 3), 0.44, seed + 2)), s, _nibble_rows()])
    return h, {name: k + r for name, r in names.items()}, k + s.shape[0]


DEGREES = [0, 1, 7, 8, 9, 63, 64, 65, 100]


def _graph(n, seed, hot, must):
    """CSR [n, n]: rows 0..8 with DEGREES entries (row 8 is the long one and gathers every column in `must`), one more
    empty row, the rest 2..13; every row with an entry gathers hot[0], every row with two or more hot[1] as well."""
    rng = np.random.default_rng(seed)
    deg = np.minimum(rng.poisson(4, n), 11) + 2
    deg[:len(DEGREES)] = DEGREES
    deg[n // 2] = 0
    rows = []
    for r, d in enumerate(deg):
        forced = list(hot[:d])
        if r == 8:
            forced = (forced + [c for c in must if c not in forced])[:d]
        others = rng.permutation(np.setdiff1d(np.arange(n), forced))[: d - len(forced)]
        rows.append(np.sort(np.concatenate([forced, others])).astype(np.int32))
    rowptr = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
    col = np.concatenate(rows).astype(np.int32)
    val = (1.0 - rng.random(col.size)).astype(np.float32)
    return rowptr, col, val


@pytest.fixture(scope="module")
def case(dev):
    """The inputs of the gather tests, checked with NumPy to hold what they are meant to hold, and the dense launch's
    result for either row-pointer width (computed once, never written to)."""
    from pygcn_amd import CSRGraph, spmm_csr
    n = 300
    h, names, nib0 = _hidden(n, 384)
    slots, defined, ovf = ref384.pack384(h)
    # -- what the rows hold: every nibble pattern at every lane of every quarter in rows that fit, quarters 1..3
    #    behind a non-zero prefix
    seen = set()
    for r in range(nib0, nib0 + N_NIBBLE):
        assert not ovf[r]
        before = 0
        for q in range(4):
            nz = (h[r, ref384.quarter_columns(q)] != 0).astype(int)
            for i in range((r - nib0) % 4, 16, 4):
                assert q == 0 or before > 0
                seen.add((q, i, int(nz[4 * i:4 * i + 4] @ [1, 2, 4, 8])))
            before += int(nz.sum())
    assert seen == {(q, i, v) for q in range(4) for i in range(16) for v in range(16)}
    assert ovf[names["total 88"]] and ovf[names["all set"]] and not ovf[names["total 87"]]
    assert defined[names["total 87"], 95] and int(slots[names["all set"], 8]) >> 24 == 255
    # -- what the graph gathers
    hot = [names["total 87"], names["all set"]]                       # one that fits, one that overflowed
    must = sorted(set(names.values()) | set(range(nib0, nib0 + N_NIBBLE)))
    rowptr, col, val = _graph(n, 5, hot, must)
    deg = np.diff(rowptr)
    assert list(deg[:len(DEGREES)]) == DEGREES and deg[n // 2] == 0
    for r in range(n):
        mine = col[rowptr[r]:rowptr[r + 1]]
        assert deg[r] == 0 or hot[0] in mine
        assert deg[r] < 2 or hot[1] in mine
    gathered = np.zeros(n, bool)
    gathered[col] = True
    cold = gathered.copy()
    cold[hot] = False
    assert gathered[must].all() and (cold & ovf).sum() > 10 and (cold & ~ovf).sum() > 10
    H = torch.from_numpy(h).to(dev)
    out = {}
    for is64 in (False, True):
        g = CSRGraph(torch.from_numpy(rowptr if is64 else rowptr.astype(np.int32)).to(dev),
                     torch.from_numpy(col).to(dev), torch.from_numpy(val).to(dev), (n, n), long_thresh=32)
        assert g.plan(torch.float32).n_long >= 4             # rows 5..8 are chunked at long_thresh = 32
        out[is64] = (g, spmm_csr(g, H))
    return {"h": h, "H": H, "slots": slots, "defined": defined, "ovf": ovf, "out": out, "n": n}


@pytest.mark.parametrize("is64", [False, True])
def test_gather_is_the_dense_launch_bit_for_bit(dev, case, is64):
    from pygcn_amd import CSRGraph, spmm_csr
    from pygcn_amd.spmm import rows_pack384
    g, dense = case["out"][is64]
    P = rows_pack384(case["H"])
    got = spmm_csr(g, packed=P)
    assert torch.equal(dense.view(torch.int32), got.view(torch.int32))
    assert torch.equal(got[0], torch.zeros(256, device=dev))                 # the empty row
    again = spmm_csr(g, packed=P)                                            # the same launch twice: the same bits
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    # the default schedule too (long_thresh 256: no chunks, row 8 is a tile and a half)
    g2 = CSRGraph(g.rowptr, g.col, g.val, (case["n"], case["n"]))
    assert torch.equal(spmm_csr(g2, case["H"]).view(torch.int32), spmm_csr(g2, packed=P).view(torch.int32))
    with pytest.raises(RuntimeError):
        spmm_csr(g, packed=P, relu=True)


@pytest.mark.parametrize("fill", [0xFFFFFFFF, 0x7FC00000])
def test_undefined_slot_words_are_never_used(dev, case, fill):
    """Slots packed on the host; the words past 9 + total and every value word of an overflowed slot set to all ones /
    a NaN: the product does not change."""
    from pygcn_amd import spmm_csr
    from pygcn_amd.spmm import PackedRows
    u = case["slots"].copy()
    assert not case["defined"][case["ovf"], 9:].any() and (~case["defined"][~case["ovf"]]).any()
    u[~case["defined"]] = fill
    P = PackedRows(torch.from_numpy(u.view(np.int32)).to(dev), case["H"])
    assert P.slot_bytes == 384                                               # (read off the width of the slots)
    for is64 in (False, True):
        g, dense = case["out"][is64]
        assert torch.equal(dense.view(torch.int32), spmm_csr(g, packed=P).view(torch.int32))
