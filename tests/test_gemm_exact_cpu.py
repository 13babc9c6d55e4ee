"""The exactness tests of tests/test_gemm_exact_gpu.py mean what they claim — shown without a GPU:
the operand builders of tests/_gemm_exact.py keep their promises (every summation order gives the
float64 result), the census is sensitive to each of the six kept part products, and the case table
reaches every instantiation of the two dispatch lists parsed from gcn_gemm.hip."""
import itertools

import numpy as np
import pytest
import torch

import _gemm_exact as E


def _sum_orders(P):
    """Sums of P [M, K, N] (float32 products) over K in several orders, all in float32: forward, backward,
    a random permutation, numpy's pairwise sum, chunks of 16 and of 32 added into a running total (the two
    K chunkings of the kernels) and the two halves of K added at the end."""
    P = P.numpy()
    K = P.shape[1]
    out = []
    for order in (np.arange(K), np.arange(K)[::-1], np.random.default_rng(3).permutation(K)):
        acc = np.zeros((P.shape[0], P.shape[2]), np.float32)
        for k in order:
            acc = acc + P[:, k, :]
        out.append(acc)
    out.append(P.sum(axis=1, dtype=np.float32))
    for chunk in (16, 32):
        acc = np.zeros((P.shape[0], P.shape[2]), np.float32)
        for k0 in range(0, K, chunk):
            acc = acc + P[:, k0:k0 + chunk, :].sum(axis=1, dtype=np.float32)
        out.append(acc)
    out.append(P[:, :K // 2].sum(axis=1, dtype=np.float32) + P[:, K // 2:].sum(axis=1, dtype=np.float32))
    return out


def _assert_every_order_exact(X, W):
    ref = X.double() @ W.double()
    ref32 = E.exact_f32(ref)
    P = X.to(torch.float32)[:, :, None] * W.to(torch.float32)[None, :, :]
    assert torch.equal(P.double(), X.double()[:, :, None] * W.double()[None, :, :]), "a product is rounded"
    for got in _sum_orders(P):
        assert np.array_equal(got, ref32.numpy())


def _assert_parts(x, h, m, l):
    p = E.split3(x)
    assert torch.equal(p["h"], h) and torch.equal(p["m"], m) and torch.equal(p["l"], l)
    assert torch.equal(p["h"].double() + p["m"].double() + p["l"].double(), x.double())


def test_integer_operands_sum_exactly_in_every_order():
    X, W = E.int_operand((9, 256), 1), E.int_operand((256, 256), 2)
    assert float(X.abs().max()) == 8 and float(W.abs().max()) == 8 and float(X.min()) == -8
    assert float((X.double() @ W.double()).abs().max()) <= 256 * 64
    _assert_every_order_exact(X, W)
    # one bf16 part, and one fp16 part after the h2 scheme's scaling of max|X| = 8 to 2^14
    zero = torch.zeros_like(X)
    _assert_parts(X, X, zero, zero)
    scaled = X * 2.0 ** 11
    assert torch.equal(scaled.to(torch.float16).to(torch.float32), scaled)
    # the weight gradient at the longest list of the GPU test: |sum| <= 64 n_list < 2^24
    assert 64 * max(E.ATG_BIG) < 2 ** 24
    A, G = E.int_operand((300, 256), 3), E.int_operand((300, 256), 4)
    _assert_every_order_exact(A.t().contiguous()[:8], G)


@pytest.mark.parametrize("K", [128, 256])
def test_bf16_integer_operands_survive_the_rounding(K):
    mx, mw = E.bf16_ranges(K)
    assert K * mx * mw <= 256
    X = E.int_operand((9, K), 5, -mx, mx, torch.bfloat16)
    W = E.int_operand((K, 128), 6, -mw, mw, torch.bfloat16)
    assert float(X.float().abs().max()) == mx and float(W.float().abs().max()) == mw
    _assert_every_order_exact(X.float(), W.float())
    ref = E.exact_f32(X.double() @ W.double())
    assert torch.equal(ref.to(torch.bfloat16).to(torch.float32), ref)       # the single rounding to bf16 is exact
    # ... and so is every integer the bound allows
    every = torch.arange(-256, 257, dtype=torch.float32)
    assert torch.equal(every.to(torch.bfloat16).to(torch.float32), every)


def test_census_values_have_the_parts_the_docstrings_state():
    c3, c2, p2 = E.census_c3((64, 256), 7), E.census_c2((64, 256), 8), E.pow2_signed((500,), 9)
    for v in (c3, c2, p2):
        assert float(v.abs().min()) >= E.ENVELOPE_MIN and bool(torch.isfinite(v).all())
    h3 = torch.sign(c3) * torch.pow(torch.tensor(2.0), torch.floor(torch.log2(c3.abs())))
    _assert_parts(c3, h3, h3 * 2.0 ** -9, h3 * 2.0 ** -17)
    h2 = torch.sign(c2) * torch.pow(torch.tensor(2.0), torch.floor(torch.log2(c2.abs())))
    _assert_parts(c2, h2, h2 * 2.0 ** -9, torch.zeros_like(c2))
    _assert_parts(p2, p2, torch.zeros_like(p2), torch.zeros_like(p2))
    # every exponent of [-40, 40] and both signs occur; the parts stay inside the documented envelope
    exps = torch.floor(torch.log2(c3.abs())).unique()
    assert exps.numel() == 81 and float(exps.min()) == -40 and float(exps.max()) == 40
    assert bool((c3 > 0).any()) and bool((c3 < 0).any())
    assert float(E.split3(c3)["l"].abs().min()) >= E.ENVELOPE_MIN


def test_part_sums_are_exact_in_every_order_and_arbitrary_values_are_not():
    """Every subset sum of the census parts, in every order of adding them, is exact in float32 — which
    arbitrary 24-bit values do not offer: adding their parts as h, l, m is off for some."""
    for v in (E.census_c3((4096,), 10), E.census_c2((4096,), 11)):
        p = E.split3(v)
        for order in itertools.permutations("hml"):
            acc32, acc64 = torch.zeros_like(v), torch.zeros_like(v, dtype=torch.float64)
            for name in order:
                acc32, acc64 = acc32 + p[name], acc64 + p[name].double()
                assert torch.equal(acc32.double(), acc64)
    x = torch.randn(200000, generator=torch.Generator().manual_seed(12))
    p = E.split3(x)
    assert torch.equal(p["h"].double() + p["m"].double() + p["l"].double(), x.double())
    off = ((p["h"] + p["l"]) + p["m"]) != x
    assert 0 < int(off.sum()) < x.numel() // 100


@pytest.mark.parametrize("case", E.CENSUS_CASES)
def test_census_products_sum_exactly_in_every_order(case):
    X, W = E.census_xw(case, 9, 20)
    _assert_every_order_exact(X, W)
    # one non-zero product per output element, nothing outside the envelope
    assert int(((X[:, :, None] != 0) & (W[None, :, :] != 0)).sum(1).max()) == 1
    ref = X.double() @ W.double()
    assert float(ref[ref != 0].abs().min()) >= E.ENVELOPE_MIN
    A, G = E.census_atg(case, 256, 21)
    assert int(((A[:, :, None] != 0) & (G[:, None, :] != 0)).sum(0).max()) == 1
    _assert_every_order_exact(A.t().contiguous()[:9], G)
    E.exact_f32(E.weight_grad_ref(A, G)[0])


def test_the_census_sees_each_of_the_six_part_products():
    """The emulation with all six kept products reproduces the expected result of every census case; with
    any ONE of them removed it differs in at least one case — in exactly the cases CENSUS_NEEDS names."""
    assert set().union(*E.CENSUS_NEEDS.values()) == set(E.KEPT_PRODUCTS) and len(E.KEPT_PRODUCTS) == 6
    for build, rows in ((E.census_xw, 257), (lambda c, n, s: _atg_as_product(c, n, s), 256)):
        seen = {p: set() for p in E.KEPT_PRODUCTS}
        for case in E.CENSUS_CASES:
            X, W = build(case, rows, 30)
            ref = X.double() @ W.double()
            assert torch.equal(E.emulated_product(X, W), ref)
            for p in E.KEPT_PRODUCTS:
                if not torch.equal(E.emulated_product(X, W, without=p), ref):
                    seen[p].add(case)
        for p in E.KEPT_PRODUCTS:
            assert seen[p] == {c for c in E.CENSUS_CASES if p in E.CENSUS_NEEDS[c]}, (p, seen[p])
            assert seen[p], f"no census case sees the part product {p}"


def _atg_as_product(case, n, seed):
    A, G = E.census_atg(case, n, seed)
    return A.t().contiguous(), G


def test_the_emulation_is_the_three_part_product_on_ordinary_values():
    """On random operands the six kept products reproduce the float64 product to the scheme's 2^-24-level
    accuracy.  Dropping m·m costs at most 2^-16 per product (|m| <= 2^-8 |x|: half an ulp of bf16's 8 bits) —
    with these standard normal operands at K = 256 that comes to 2e-6 .. 4e-6 of a row's largest entry: the
    same order as the empirical gates of tests/test_gemm_gpu.py (2e-6 / 4e-6), which is why the census of
    tests/test_gemm_exact_gpu.py looks at each part product on its own."""
    g = torch.Generator().manual_seed(31)
    X, W = torch.randn(64, 256, generator=g), torch.randn(256, 256, generator=g)
    ref = X.double() @ W.double()
    scale = ref.abs().amax(1)
    assert bool(((E.emulated_product(X, W) - ref).abs().amax(1) <= 2e-7 * scale).all())
    lost = (E.emulated_product(X, W, without=("m", "m")) - E.emulated_product(X, W)).abs()
    assert bool((lost <= 2.0 ** -16 * (X.double().abs() @ W.double().abs())).all())
    assert float((lost.amax(1) / scale).min()) > 2e-7         # (visible: above what the kept products leave)


def test_references_of_the_store_sections():
    y = torch.tensor([[-3.0, 0.0, 5.0, 7.0]])
    bias = torch.tensor([1.0, -1.0, -6.0, 0.0])
    assert torch.equal(E.forward_store(y, bias), torch.tensor([[-2.0, -1.0, -1.0, 7.0]]))
    assert torch.equal(E.forward_store(y, bias, relu=True), torch.tensor([[0.0, 0.0, 0.0, 7.0]]))
    keep = torch.tensor([[True, True, False, True]])
    assert torch.equal(E.forward_store(y, None, True, keep, np.float32(2.0)), torch.tensor([[0.0, 0.0, 0.0, 14.0]]))
    mask = torch.tensor([[1.0, -0.0, 0.0, 2.0 ** -100], [-1.0, 3.0, 0.0, 0.0]])
    got = E.masked_store(torch.cat([y, y]), mask, torch.tensor([1, 0]), 1.5)
    assert torch.equal(got, torch.tensor([[0.0, 0.0, 0.0, 0.0], [-4.5, 0.0, 0.0, 10.5]]))
    assert torch.equal(E.mask_row_index(3), torch.arange(3))
    assert torch.equal(E.mask_row_index(2, x_rows=torch.tensor([5, 4, 3])), torch.tensor([5, 4]))
    assert torch.equal(E.mask_row_index(2, torch.tensor([5, 4]), torch.tensor([9, 8])), torch.tensor([9, 8]))
    m = E.sign_mask((64, 256), 1)
    assert bool((m == 0).any()) and bool(torch.signbit(m[m == 0]).any()) and not bool(torch.signbit(m[m == 0]).all())
    assert bool((m > 0).any()) and bool((m < 0).any())
    mb = E.sign_mask((64, 256), 1, torch.bfloat16)
    assert torch.equal(mb.float() > 0, m > 0)
    # keep bits: the documented lane order, column by column
    bits = torch.zeros(2, 8, dtype=torch.int32)
    for col in (0, 5, 19, 131, 255):
        q, j, cw = (col >> 2) & 3, col & 3, col >> 4
        word, bit = 2 * q + (cw >> 3), 4 * (cw & 7) + j
        bits[1, word] |= np.int32(np.uint32(1 << bit).view(np.int32) if bit == 31 else 1 << bit)
    dec = E.keep_bits_decode(bits, 2)
    assert not bool(dec[0].any()) and sorted(dec[1].nonzero().flatten().tolist()) == [0, 5, 19, 131, 255]


def test_the_case_table_reaches_every_instantiation():
    """The dense counterpart of test_the_width_lists_reach_every_variant: the instantiation lists parsed
    from gcn_gemm.hip, and the case table pushed through the restated dispatch."""
    import test_gemm_exact_gpu as gpu
    assert gpu.XW_CASES is E.XW_CASES and gpu.BF16_CASES is E.BF16_CASES and gpu.R1_CASES is E.R1_CASES
    xw = E.parse_xw_kernels()
    assert len(xw) == 20 and len(set(xw)) == 20
    assert set(xw) == ({(f, e, False) for f in (0, 1) for e in (0, 1, 2, 4, 5, 6)}
                       | {(2, e, False) for e in (0, 1, 2, 3, 4, 5)} | {(2, 4, True), (2, 5, True)})
    missing = set(xw) - E.reached_xw()
    assert not missing, sorted(missing)
    assert E.reached_xw() <= set(xw)                       # (the rule never asks for a kernel that does not exist)
    bf = E.parse_bf16_kernels()
    assert len(bf) == 21 and set(bf) == {(k, n, e) for k, n in E.BF16_SHAPES for e in range(7)}
    assert set(bf) == E.reached_bf16()
    # integer operands reach every instantiation on their own, at small heights; the big heights reach the
    # plain, one forward, one masked and the keep-bit sections of each kernel form
    ints = [c for c in E.XW_CASES if c["operands"] == "int" and len(c["heights"]) > 1]
    assert E.reached_xw(ints) == set(xw)
    big = E.reached_xw([c for c in E.XW_CASES if len(c["heights"]) == 1 and c["operands"] == "int"])
    assert big == ({(f, e, False) for f in (0, 1) for e in (0, 5, 2)}
                   | {(2, 0, False), (2, 5, False), (2, 2, False), (2, 3, False), (2, 4, True), (2, 5, True)})
    # the census runs on both kernels behind _b3: plain, one forward and one masked section each
    cen = E.reached_xw([c for c in E.XW_CASES if c["operands"].startswith("census")])
    assert cen == {(f, e, False) for f in (1, 2) for e in (0, 4, 2)}
    for c in E.XW_CASES:
        for M in c["heights"]:
            assert M >= 1
    # heights: one row, both sides of an MFMA tile and of a workgroup tile, a second tile on two workgroups
    assert E.S16_BIG == 32897 and -(-E.S16_BIG // 128) == 258 and E.S16_BIG % 128 == 1
    assert E.T256_BIG == 65793 and -(-E.T256_BIG // 256) == 258 and E.T256_BIG % 256 == 1
    assert -(-(-(-E.BF16_BIG // 32)) // 4) == 256 * 3 + 1  # one more workgroup than 3 per CU are resident
    assert E.atg_wgs(32800) == (256, 51) and E.atg_wgs(70001)[0] == 256 and E.atg_wgs(129) == (2, 0)


def test_the_restated_rule_refuses_what_the_host_code_refuses():
    R = E.Refused
    ok = E.expected_xw_kernel
    assert ok("b3", False, relu=True, keep_bits_out=True) == (2, 4, True)
    assert ok("b3", False, relu=True, dropout_p=0.5, keep_bits_out=True) == (2, 5, True)
    assert ok("b3", False, mask_bits=True) == (2, 3, False)
    assert ok("b3", False, mask_src=True, mask_bits=True) == (2, 3, False)
    refused = [
        dict(scheme="b3", has_rows=True, relu=True, keep_bits_out=True),            # keep bits with a row list
        dict(scheme="b3", has_rows=True, mask_bits=True),
        dict(scheme="b3", has_rows=False, relu=True, dropout_p=0.3, keep_bits_out=True),   # p not in {0, 1/2}
        dict(scheme="b3", has_rows=False, relu=True, dropout_p=0.25, keep_bits_out=True),
        dict(scheme="b3", has_rows=False, relu=True, keep_bits_out=True, ldx=1 << 21),     # a pitch >= 2^21
        dict(scheme="b3", has_rows=False, relu=True, keep_bits_out=True, ldy=1 << 21),
        dict(scheme="b3", has_rows=False, mask_bits=True, ldx=1 << 21),
        dict(scheme="b3", has_rows=False, mask_bits=True, ldy=1 << 21),
        dict(scheme="b3", has_rows=False, bias=True, keep_bits_out=True),           # keep bits without ReLU
        dict(scheme="b3", has_rows=False, keep_bits_out=True),
        dict(scheme="h2", has_rows=False, relu=True, keep_bits_out=True),           # the two-part scheme
        dict(scheme="h2", has_rows=False, mask_bits=True),
        dict(scheme="b3", has_rows=False, relu=True, mask_bits=True),               # forward + backward
        dict(scheme="b3", has_rows=False, bias=True, mask_src=True),
        dict(scheme="b3", has_rows=False, dropout_p=0.5),                           # dropout without ReLU
        dict(scheme="b3", has_rows=False, relu=True, dropout_p=1.0),
        dict(scheme="b3", has_rows=False, ldx=255),
    ]
    for kw in refused:
        with pytest.raises(R) as info:
            ok(**kw)
        assert info.value.code == E.GCN_E_BADARG, kw
    with pytest.raises(R) as info:
        ok("b3", False, ldy=258)
    assert info.value.code == E.GCN_E_ALIGN
    # at a pitch of 2^21 the three-part entry point falls back to the row-list kernel's form
    for kw in (dict(ldx=1 << 21), dict(ldy=1 << 21)):
        assert ok("b3", False, **kw) == (1, 0, False) and ok("b3", False, mask_src=True, **kw) == (1, 2, False)
        assert ok("b3", False, ldx=(1 << 21) - 4) == (2, 0, False)
    assert ok("b3", False, bias=True, relu=True, dropout_p=0.3) == (1, 6, False)   # no s16 instantiation of EPI 6
    with pytest.raises(R):
        E.expected_bf16_kernel(256, 256)
    with pytest.raises(R):
        E.expected_bf16_kernel(128, 128, relu=True, mask_src=True)
    assert E.dropout_threshold16(0.5) == 32768 and E.dropout_threshold16(0.0) == 0
    assert E.dropout_threshold16(0.3) == 19661 and E.dropout_threshold16(1e-9) == 1
