"""The pooled 384-byte packed row format without a GPU: the NumPy reference that the GPU tests judge the kernels by
(tests/_pack384_ref.py) against the format's own statement, the capacity constant, the binding table, and the
overflow share the capacity was chosen for."""
import os
import re

import numpy as np

import _pack384_ref as ref384
from conftest import ROOT


def test_reference_round_trips_bit_for_bit():
    rng = np.random.default_rng(3)
    h = rng.standard_normal((60, 256)).astype(np.float32)
    h[rng.random((60, 256)) >= 0.25] = 0.0
    s, _ = ref384.special_rows()
    h = np.concatenate([h, s])
    slots, defined, ovf = ref384.pack384(h)
    assert slots.shape == (h.shape[0], 96) and slots.dtype == np.uint32
    back, ovf2 = ref384.unpack384(slots)
    assert np.array_equal(ovf, ovf2) and ovf.any() and not ovf.all()
    assert np.array_equal(back.view(np.uint32)[~ovf], h.view(np.uint32)[~ovf])
    total = (h.view(np.uint32) != 0).sum(1)
    assert np.array_equal(ovf, total > ref384.CAPACITY)
    assert np.array_equal(defined.sum(1), 9 + np.where(ovf, 0, total))
    assert not slots[~defined].any()


def test_reference_layout_is_the_keep_bit_order_of_the_gemm():
    """Quarter q, bit 4 cb + j <-> column 16 cb + 4 q + j; the header's running counts; one pool."""
    for c in (0, 3, 4, 15, 16, 100, 255):
        h = np.zeros((1, 256), np.float32)
        h[0, c] = 2.5
        slots, _, _ = ref384.pack384(h)
        q, cb, j = (c >> 2) & 3, c >> 4, c & 3
        masks = [int(slots[0, 2 * k]) | (int(slots[0, 2 * k + 1]) << 32) for k in range(4)]
        assert masks == [(1 << (4 * cb + j)) if k == q else 0 for k in range(4)]
        want = sum((1 if q <= k else 0) << (8 * k) for k in range(3)) | (1 << 24)
        assert slots[0, 8] == want
        assert slots[0, 9] == np.float32(2.5).view(np.uint32) and not slots[0, 10:].any()
    h = np.zeros((1, 256), np.float32)                      # quarter 3's lowest bit comes after quarter 0's highest
    h[0, ref384.quarter_columns(3)[0]], h[0, ref384.quarter_columns(0)[63]] = 3.0, 4.0
    slots, _, _ = ref384.pack384(h)
    assert list(slots[0, 9:11].view(np.float32)) == [4.0, 3.0] and slots[0, 8] == (1 | 1 << 8 | 1 << 16 | 2 << 24)


def test_reference_edge_rows():
    h, names = ref384.special_rows()
    slots, defined, ovf = ref384.pack384(h)
    assert set(np.flatnonzero(ovf)) == {names[k] for k in ("total 88", "all set", "all -0.0")}
    for k in ("all set", "all -0.0"):
        assert [int(slots[names[k], 8] >> (8 * b)) & 0xFF for b in range(4)] == [64, 128, 192, 255]
        assert not defined[names[k], 9:].any()
    assert defined[names["total 87"]].all() and not defined[names["total 86"], 95]
    assert [int(slots[names["64 0 0 23"], 8] >> (8 * b)) & 0xFF for b in range(4)] == [64, 64, 64, 87]
    assert [int(slots[names["0 0 23 64"], 8] >> (8 * b)) & 0xFF for b in range(4)] == [0, 0, 23, 87]
    back, _ = ref384.unpack384(slots)
    r = names["special values"]
    assert np.signbit(back[r, 1]) and back[r, 1] == 0 and np.isnan(back[r, 17]) and back[r, 35] == np.inf \
        and back[r, 255] == -np.inf and back.view(np.uint32)[r, 100] == 1 and back.view(np.uint32)[r, 101] == 0x807FFFFF


def test_capacity_abi_and_entry_points():
    from pygcn_amd import _native, spmm
    hdr = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    assert int(re.search(r"#define GCN_PACK384_CAPACITY\s+(\d+)", hdr).group(1)) == ref384.CAPACITY \
        == spmm.PACK384_CAPACITY == 87
    assert int(re.search(r"#define GCN_ABI_VERSION\s+(\d+)", hdr).group(1)) == 26 == _native.GCN_ABI_VERSION
    assert _native.lib().gcn_abi_version() == 26
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, like in (("gcn_rows_pack384", "gcn_rows_pack512"), ("gcn_spmm_csr_packed384", "gcn_spmm_csr_packed")):
        m = re.search(r"\bint %s\((.*?)\);" % name, code, re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_native.SIGNATURES[name][1]), name
        assert _native.SIGNATURES[name] == _native.SIGNATURES[like]
        assert hasattr(_native.lib(), name)


def test_overflow_share_at_a_quarter_density():
    """The reference alone: 200 000 rows of Bernoulli(1/4) overflow at the binomial tail P(Bin(256, 1/4) > 87) =
    5.1e-4; the guard is 2e-3."""
    from math import comb
    tail = sum(comb(256, k) * 3 ** (256 - k) for k in range(88, 257)) / 4 ** 256
    assert 5.0e-4 < tail < 5.2e-4
    rng = np.random.default_rng(87)
    m, piece, over = 200_000, 20_000, 0
    for lo in range(0, m, piece):
        h = (rng.random((piece, 256)) < 0.25).astype(np.float32)
        over += int(ref384.overflowed(h).sum())
    assert np.array_equal(ref384.pack384(h[:500])[2], ref384.overflowed(h[:500]))
    assert over / m <= 2e-3, over / m
