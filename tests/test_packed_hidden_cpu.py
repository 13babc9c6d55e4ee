"""The fixed-slot packed row format without a GPU: the NumPy reference of pack / expand that the GPU tests judge
the kernel by (tests/_pack512_ref.py) is checked against the format's own statement, and the C-ABI's new entry
points are what the header and the binding table say."""
import os
import re

import numpy as np
import torch

import _pack512_ref as ref512
from conftest import ROOT


def test_reference_pack_round_trips_bit_for_bit():
    rng = np.random.default_rng(1)
    h = rng.standard_normal((40, 256)).astype(np.float32)
    h[rng.random((40, 256)) >= 0.25] = 0.0
    h[3] = 0.0
    slots, written, ovf = ref512.pack(h)
    assert slots.shape == (40, 128) and slots.dtype == np.uint32
    back, ovf2 = ref512.expand(slots)
    assert np.array_equal(ovf, ovf2)
    assert np.array_equal(back.view(np.uint32)[~ovf], h.view(np.uint32)[~ovf])
    assert not written[3, 3:32].any() and written[3, :3].all() and not slots[3].any()
    # the count word is the population count of the mask, sub-slot by sub-slot; at 25 % density no quarter of
    # these rows comes near the capacity
    for q in range(4):
        cnt = (h[:, ref512.quarter_columns(q)] != 0).sum(1)
        assert np.array_equal(slots[:, 32 * q + 2], cnt)
    assert not ovf.any()


def test_reference_layout_is_the_keep_bit_order_of_the_gemm():
    """Quarter q, bit 4 cb + j <-> column 16 cb + 4 q + j: one value set at a time."""
    for c in (0, 3, 4, 15, 16, 100, 255):
        h = np.zeros((1, 256), np.float32)
        h[0, c] = 2.5
        slots, _, _ = ref512.pack(h)
        q, cb, j = (c >> 2) & 3, c >> 4, c & 3
        mask = int(slots[0, 32 * q]) | (int(slots[0, 32 * q + 1]) << 32)
        assert mask == 1 << (4 * cb + j)
        assert slots[0, 32 * q + 2] == 1 and slots[0, 32 * q + 3] == np.float32(2.5).view(np.uint32)
        others = [k for k in range(4) if k != q]
        assert not slots[0].reshape(4, 32)[others].any()
    assert sorted(np.concatenate([ref512.quarter_columns(q) for q in range(4)])) == list(range(256))


def test_reference_overflow_and_special_values():
    h, names = ref512.special_rows()
    slots, written, ovf = ref512.pack(h)
    assert set(np.flatnonzero(ovf)) == {names["quarter 1 one over"], names["quarter 2 all set"], names["all -0.0"]}
    back, _ = ref512.expand(slots)
    keep = ~ovf
    assert np.array_equal(back.view(np.uint32)[keep], h.view(np.uint32)[keep])
    r = names["quarter 1 one over"]                   # the first CAPACITY values of the quarter survive, in bit order
    cols = ref512.quarter_columns(1)
    set_cols = cols[h[r, cols] != 0]
    assert np.array_equal(back[r, set_cols[:ref512.CAPACITY]], h[r, set_cols[:ref512.CAPACITY]])
    assert back[r, set_cols[ref512.CAPACITY]] == 0
    assert written[r, 32: 64].all() and slots[r, 34] == ref512.CAPACITY + 1
    r = names["special values"]                        # -0.0 is a stored value, NaN and the infinities too
    assert np.signbit(back[r, 1]) and np.isnan(back[r, 17]) and back[r, 35] == np.inf and back[r, 255] == -np.inf


def test_entry_points_and_capacity_are_declared():
    from pygcn_amd import _native, spmm
    hdr = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    assert int(re.search(r"#define GCN_PACK512_CAPACITY\s+(\d+)", hdr).group(1)) == ref512.CAPACITY \
        == spmm.PACK512_CAPACITY
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("gcn_rows_pack512", "gcn_spmm_csr_packed", "gcn_gemm_xw256_f32_b3_logsoftmax"):
        m = re.search(r"\bint %s\((.*?)\);" % name, code, re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_native.SIGNATURES[name][1]), name
        assert hasattr(_native.lib(), name)


def test_the_route_is_off_without_its_conditions():
    from pygcn_amd import fused
    h1, w2 = torch.zeros(4, 256), torch.zeros(256, 256)
    before = fused.packed_hidden()
    try:
        fused.set_packed_hidden(False)
        assert not fused.packed_hidden_applies(h1, w2, None, 0.5)        # switched off
        fused.set_packed_hidden(True)
        assert fused.packed_hidden()
        assert not fused.packed_hidden_applies(h1, w2, None, 0.5)        # not a HIP tensor
        assert not fused.packed_hidden_applies(h1, w2, None, 0.0)        # no dropout: eval mode
    finally:
        fused.set_packed_hidden(before)
