"""Every instantiation of the dense-product kernels (pygcn_amd/csrc/gcn_gemm.hip) on exactly summable
operands: the result must be the float64 result BIT FOR BIT, whatever the kernel's summation order —
no tolerance appears in this file.  Operands, references, the restated dispatch and the case table are
tests/_gemm_exact.py; tests/test_gemm_exact_cpu.py shows (without a GPU) that the operands are exact,
that the census sees each of the six part products and that the table reaches every instantiation.

The kernels are called through the C ABI (the entry point selects the scheme), every workspace is
filled with NaN bytes first, every output sits in a sentinel-filled buffer that is compared as a
whole (guard rows, guard columns, the keep-bit rows past M), unlisted operand rows and the gaps of
pitched operands hold NaN."""
import ctypes

import numpy as np
import pytest
import torch

import _gemm_exact as E
from _gemm_exact import BF16_CASES, R1_CASES, XW_CASES, case_id

pytestmark = pytest.mark.gpu

SENT = -24680.5                   # exactly representable in fp32 and bf16; no result of these operands
BITS_SENT = 0x5A5A5A5A
MASK_SCALE = 1.5
SEED = 0x9E3779B97F4A7C15
ROW_BASE = 7
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _caches():
    yield
    _OPERANDS.clear()
    _KEEP.clear()


def _lib():
    from pygcn_amd import _native
    return _native.lib()


def _check(rc, what):
    from pygcn_amd import _native
    _native.check(rc, what)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan_ws(nbytes, dev):
    """A workspace of NaN bytes: scratch, so no result may depend on what it held."""
    return torch.full((max(int(nbytes), 16),), 0xFF, dtype=torch.uint8, device=dev)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _assert_same(got, exp, what):
    if torch.equal(got, exp):
        return
    bad = (got != exp).nonzero()
    first = [(tuple(i.tolist()), float(got[tuple(i)]), float(exp[tuple(i)])) for i in bad[:6]]
    pytest.fail(f"{what}: {bad.shape[0]} of {got.numel()} elements differ; (index, got, expected) {first}")


class Window:
    """An output [rows, width] as a window of a larger sentinel-filled buffer: `guard` rows below it, columns
    [col0, col0 + width) of a row pitch `ld`.  check() compares the WHOLE buffer."""

    def __init__(self, rows, width, dtype, dev, ld=None, col0=0, guard=3):
        self.rows, self.width, self.col0 = rows, width, col0
        self.ld = ld or width
        self.buf = torch.full((rows + guard, self.ld), SENT, dtype=dtype, device=dev)
        self.view = self.buf[:rows, col0:col0 + width]
        self.ptr = self.view.data_ptr()

    def check(self, ref, what):
        exp = torch.full_like(self.buf, SENT)
        exp[:self.rows, self.col0:self.col0 + self.width] = ref.to(self.buf.dtype)
        _assert_same(self.buf, exp, what)


def _pitched(t, ld, lead=0):
    """A copy of the 2-D tensor t with row pitch `ld` whose base lies `lead` ELEMENTS behind an allocation's
    (256-byte aligned) start; the gaps and the lead hold NaN."""
    n, w = t.shape
    buf = torch.full((lead + n * ld,), NAN, dtype=t.dtype, device=t.device)
    view = buf[lead:].view(n, ld)[:, :w]
    view.copy_(t)
    assert view.stride(0) == ld and view.data_ptr() == buf.data_ptr() + lead * t.element_size()
    return view


# ---- operands (cached per module: the float64 references of the large heights are formed once) ----
_OPERANDS = {}
_KEEP = {}


def _row_list(kind, M, n_src, seed, dev):
    if kind is None:
        return None
    if kind == "identity":
        return torch.arange(M, dtype=torch.int32, device=dev)
    r = torch.randint(0, n_src, (M,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)
    if M >= 2:
        r[M // 2] = r[0]                                   # a shuffled list WITH duplicates
    return r.to(dev)


def _poison_unlisted(X, rows):
    """NaN in every row a list does not name: unlisted rows are never read."""
    if rows is not None:
        listed = torch.zeros(X.shape[0], dtype=torch.bool, device=X.device)
        listed[rows.long()] = True
        X[~listed] = NAN
    return X


def _xw_operands(kind, M, rows_kind, dev):
    """(X source, x_rows, W, the exact float32 product of the listed rows) for a table case."""
    key = ("xw", kind, M, rows_kind)
    if key not in _OPERANDS:
        n_src = M if rows_kind in (None, "identity") else M + 13
        seed = 1000 + 7 * M
        if kind == "int":
            X, W = E.int_operand((n_src, 256), seed), E.int_operand((256, 256), seed + 1)
        else:
            X, W = E.census_xw(kind.split("_")[1], n_src, seed)
        X, W = X.to(dev), W.to(dev)
        rows = _row_list(rows_kind, M, n_src, seed + 2, dev)
        y32 = E.exact_f32(E.product_ref(X, W, rows))
        val = (_poison_unlisted(X, rows), rows, W, y32)
        if M < 1000:
            return val
        _OPERANDS[key] = val
    return _OPERANDS[key]


def _keep(oracle, p, M, N, dev):
    key = (p, M, N)
    if key not in _KEEP:
        if len(_KEEP) > 12:
            _KEEP.clear()
        k = oracle.dropout_keep(SEED, np.arange(M), N, p, row_base=ROW_BASE)
        _KEEP[key] = torch.from_numpy(np.ascontiguousarray(k)).to(dev)
    return _KEEP[key]


class Store:
    """The epilogue struct of a named store section (E.STORES) for M output rows, what keeps its tensors alive,
    and the store it must produce from the exact accumulators."""

    def __init__(self, name, M, x_rows, n_src, dev, oracle, dtype=torch.float32, N=256, ld_mask=None, seed=0):
        from pygcn_amd import _native
        f = E.STORES[name]
        self.name, self.M, self.N, self.f, self.dev, self.x_rows = name, M, N, f, dev, x_rows
        self.bias = E.int_bias(N, seed + 11).to(dev) if f.get("bias") else None
        self.p = f.get("dropout_p", 0.0)
        self.keep = _keep(oracle, self.p, M, N, dev) if self.p > 0 else None
        self.scale = oracle.dropout_scale(self.p) if self.p > 0 else None
        self.mask = self.mask_rows = self.bits = self.mask_bits = None
        g = torch.Generator().manual_seed(seed + 12)
        masked = f.get("mask_src") or f.get("mask_bits")
        if masked:
            n_mask = M + 37 if f.get("mask_rows") else n_src
            if f.get("mask_rows"):
                self.mask_rows = torch.randint(0, n_mask, (M,), generator=g, dtype=torch.int32).to(dev)
            self.n_mask = n_mask
        if f.get("mask_src"):
            m = E.sign_mask((self.n_mask, N), seed + 13, dtype).to(dev)
            self.mask = _pitched(m, ld_mask) if ld_mask else m
        if f.get("keep_bits_out"):
            self.bits = torch.full((M + 5, 8), BITS_SENT, dtype=torch.int32, device=dev)
        self.struct = None
        if f:
            self.struct = _native.GcnGemmEpilogue(
                _ptr(self.bias), int(bool(f.get("relu"))), float(self.p), SEED, None,
                _ptr(self.mask), self.mask.stride(0) if self.mask is not None else 0, MASK_SCALE,
                _ptr(self.mask_rows), ROW_BASE, _ptr(self.bits), None)

    def use_mask_bits(self, bits, mask_ref):
        """Backward mask from keep bits a forward launch wrote (`mask_ref`: that launch's exact output)."""
        self.mask_bits, self.mask = bits, mask_ref
        self.struct.mask_bits = bits.data_ptr()
        self.struct.mask_src = None

    def byref(self):
        return ctypes.byref(self.struct) if self.struct is not None else None

    def expected(self, y32):
        f = self.f
        if f.get("mask_src") or f.get("mask_bits"):
            idx = E.mask_row_index(self.M, self.x_rows, self.mask_rows, self.dev)
            return E.masked_store(y32, self.mask, idx, MASK_SCALE)
        return E.forward_store(y32, self.bias, bool(f.get("relu")), self.keep, self.scale)

    def check_bits(self, stored, what):
        """keep_bits_out: `out > 0` in the documented lane order for rows < M, the sentinel below."""
        if self.bits is None:
            return
        _assert_same(E.keep_bits_decode(self.bits, self.M).to(torch.int32), (stored > 0).to(torch.int32), what + " keep bits")
        guard = self.bits[self.M:]
        _assert_same(guard, torch.full_like(guard, BITS_SENT), what + " keep-bit rows past M")


def _call_xw(entry, X, rows, W, Yw, M, ep=None, absmax=None, bound=None):
    """One launch through the C ABI; returns the code."""
    L, dev = _lib(), X.device
    if entry == "r1":
        ws = _nan_ws(L.gcn_gemm_xw256_workspace_bytes(), dev)
        return L.gcn_gemm_xw256_f32(X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0), Yw.ptr, Yw.ld, M,
                                    ws.data_ptr(), ws.numel(), _stream())
    if entry == "b3":
        ws = _nan_ws(L.gcn_gemm_xw256_b3_workspace_bytes(), dev)
        return L.gcn_gemm_xw256_f32_b3(X.data_ptr(), X.stride(0), _ptr(rows), W.data_ptr(), W.stride(0), Yw.ptr, Yw.ld,
                                       M, _ptr(absmax), ep, ws.data_ptr(), ws.numel(), _stream())
    ws = _nan_ws(L.gcn_gemm_xw256_h2_workspace_bytes(), dev)
    return L.gcn_gemm_xw256_f32_h2(X.data_ptr(), X.stride(0), _ptr(rows), W.data_ptr(), W.stride(0), Yw.ptr, Yw.ld, M,
                                   bound.data_ptr(), _ptr(absmax), ep, ws.data_ptr(), ws.numel(), _stream())


def _forward_bits(n_mask, dev, seed, oracle, p):
    """A forward launch (ReLU, dropout at p = 0 or 1/2, keep_bits_out) of gcn_gemm_xw256_f32_b3 over n_mask rows:
    (the bits it wrote, its exact output) — the mask a backward launch then reads as bits."""
    from pygcn_amd import _native
    X, W = E.int_operand((n_mask, 256), seed, zero_fraction=0.3).to(dev), E.int_operand((256, 256), seed + 1).to(dev)
    keep, scale = (_keep(oracle, p, n_mask, 256, dev), oracle.dropout_scale(p)) if p > 0 else (None, None)
    out = E.forward_store(E.exact_f32(E.product_ref(X, W)), None, True, keep, scale)
    bits = torch.full((n_mask + 5, 8), BITS_SENT, dtype=torch.int32, device=dev)
    ep = _native.GcnGemmEpilogue(None, 1, float(p), SEED, None, None, 0, 1.0, None, ROW_BASE, bits.data_ptr(), None)
    Yw = Window(n_mask, 256, torch.float32, dev)
    _check(_call_xw("b3", X, None, W, Yw, n_mask, ctypes.byref(ep)), "forward launch with keep_bits_out")
    Yw.check(out, "forward launch with keep_bits_out")
    _assert_same(E.keep_bits_decode(bits, n_mask).to(torch.int32), (out > 0).to(torch.int32), "keep bits")
    assert bool((out > 0).any()) and bool((out == 0).any())
    return bits, out


def _run_xw_case(c, M, dev, oracle, pitched=False):
    entry, rows_kind, store = c["entry"], c["rows"], c["store"]
    X, rows, W, y32 = _xw_operands(c["operands"], M, rows_kind, dev)
    what = f"{case_id(c)} M={M}" + (" pitched" if pitched else "")
    # the instantiation this launch must take (and that the host code does not refuse it)
    form = E.expected_xw_kernel(entry, rows is not None, **E.dispatch_fields(store))
    assert form in set(E.parse_xw_kernels())
    if pitched:
        X, W = _pitched(X, 320), _pitched(W, 512, lead=1)          # ldx 320; ldw 512, W 4 bytes off the 16-byte grid
        assert W.data_ptr() % 16 == 4
    st = Store(store, M, rows, X.shape[0], dev, oracle, ld_mask=512 if pitched else None, seed=M)
    if E.STORES[store].get("mask_bits"):
        # (the bits of a ReLU launch where the mask is read at the row, of a dropout launch where through mask_rows)
        st.use_mask_bits(*_forward_bits(st.n_mask, dev, 500 + M, oracle, 0.5 if st.mask_rows is not None else 0.0))
    Yw = Window(M, 256, torch.float32, dev, ld=288, col0=8, guard=64) if pitched else Window(M, 256, torch.float32, dev)
    absmax = torch.zeros(1, dtype=torch.float32, device=dev)
    bound = torch.full((1,), 8.0, dtype=torch.float32, device=dev) if entry == "h2" else None
    _check(_call_xw(entry, X, rows, W, Yw, M, st.byref(), absmax, bound), what)
    exp = st.expected(y32)
    Yw.check(exp, what)
    st.check_bits(exp, what)
    # y_absmax = the maximum of the values actually stored, exactly
    _assert_same(absmax, exp.abs().max().reshape(1), what + " y_absmax")


# ------------------------------------------------------------------------------------------------
# the 256 x 256 product
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", XW_CASES, ids=case_id)
def test_xw256_is_the_float64_product_bit_for_bit(dev, oracle, c):
    """gcn_gemm_xw256_f32_b3 / _h2 through every instantiation of XwKernels: integer operands through every
    store section at the heights that reach each path, the census through both three-part kernels."""
    for M in c["heights"]:
        _run_xw_case(c, M, dev, oracle)


@pytest.mark.parametrize("c", [c for c in XW_CASES if c["operands"] == "int" and len(c["heights"]) > 1], ids=case_id)
def test_xw256_pitches_and_guard_bands(dev, oracle, c):
    """The pitch parameters of the C ABI, which the Python wrappers never pass: Y as the window [:, 8:264] of a
    288-wide buffer with 64 guard rows below, ldx = 320, ldw = 512 with W's base 4 bytes off the 16-byte grid,
    ld_mask = 512 — all gaps NaN; the guards, and the keep-bit rows past M, keep their sentinel."""
    for M in (c["heights"][0], c["heights"][3], c["heights"][-1]):
        _run_xw_case(c, M, dev, oracle, pitched=True)


@pytest.mark.parametrize("c", R1_CASES, ids=case_id)
def test_round_one_kernel_is_the_float64_product_bit_for_bit(dev, c):
    """gcn_gemm_xw256_f32 (the VGPR-staged three-part kernel, kept as the bit-exact reference of the scheme)."""
    for M in c["heights"]:
        X, _, W, y32 = _xw_operands(c["operands"], M, None, dev)
        for pitched in (False, True) if M < 1000 else (False,):
            Xp, Wp = (_pitched(X, 320), _pitched(W, 512, lead=1)) if pitched else (X, W)
            Yw = Window(M, 256, torch.float32, dev, ld=288, col0=8, guard=64) if pitched else Window(M, 256, torch.float32, dev)
            _check(_call_xw("r1", Xp, None, Wp, Yw, M), "gcn_gemm_xw256_f32")
            Yw.check(y32, f"gcn_gemm_xw256_f32 {c['operands']} M={M} pitched={pitched}")


@pytest.mark.parametrize("which", ["ldx", "ldy"])
def test_three_part_product_at_a_pitch_of_two_to_the_21(dev, which):
    """At ldx = 2^21 or ldy = 2^21 the contiguous-row kernel cannot address a tile (32-bit offsets from the tile
    origin): gcn_gemm_xw256_f32_b3 falls back to the row-list kernel's form and stays exact; the keep-bit forms,
    which exist in the other kernel only, are refused with GCN_E_BADARG, and gemm_keep_bits_usable agrees."""
    from pygcn_amd import _native
    from pygcn_amd.gemm import gemm_keep_bits_usable
    M, big = 3, 1 << 21
    ldx, ldy = (big, 256) if which == "ldx" else (256, big)
    assert E.expected_xw_kernel("b3", False, ldx=ldx, ldy=ldy) == (1, 0, False)
    X0, W = E.int_operand((M, 256), 77).to(dev), E.int_operand((256, 256), 78).to(dev)
    y32 = E.exact_f32(E.product_ref(X0, W))
    X = X0
    if which == "ldx":
        X = torch.zeros((M, big), dtype=torch.float32, device=dev)[:, :256]      # (25 MB)
        X.copy_(X0)
        assert X.stride(0) == big and not gemm_keep_bits_usable(X) and gemm_keep_bits_usable(X0)
    mask = E.sign_mask((M, 256), 79).to(dev)
    for name in ("plain", "mask"):
        Yw = Window(M, 256, torch.float32, dev, ld=ldy, guard=0)
        ep = None
        if name == "mask":
            ep = ctypes.byref(_native.GcnGemmEpilogue(None, 0, 0.0, 0, None, mask.data_ptr(), 256, MASK_SCALE, None, 0, None, None))
        _check(_call_xw("b3", X, None, W, Yw, M, ep), f"b3 at {which} = 2^21")
        exp = y32 if ep is None else E.masked_store(y32, mask, torch.arange(M, device=dev), MASK_SCALE)
        Yw.check(exp, f"b3 {name} at {which} = 2^21")
        del Yw
    bits = torch.full((M + 5, 8), BITS_SENT, dtype=torch.int32, device=dev)
    Yw = Window(M, 256, torch.float32, dev, ld=ldy, guard=0)
    for fields, kw in ((dict(relu=True, keep_bits_out=True), dict(relu=1, keep=bits.data_ptr(), mb=None)),
                       (dict(mask_bits=True), dict(relu=0, keep=None, mb=bits.data_ptr()))):
        with pytest.raises(E.Refused):
            E.expected_xw_kernel("b3", False, ldx=ldx, ldy=ldy, **fields)
        ep = _native.GcnGemmEpilogue(None, kw["relu"], 0.0, 0, None, None, 0, 1.0, None, 0, kw["keep"], kw["mb"])
        assert _call_xw("b3", X, None, W, Yw, M, ctypes.byref(ep)) == E.GCN_E_BADARG
    torch.cuda.synchronize()
    Yw.check(torch.full((M, 256), SENT, device=dev), "a refused launch stores nothing")     # nothing was launched
    _assert_same(bits, torch.full_like(bits, BITS_SENT), "a refused launch writes no keep bits")
    # one pitch below the limit the contiguous-row kernel runs (and is exact: the table's cases)
    assert E.expected_xw_kernel("b3", False, ldx=big - 4, ldy=256) == (2, 0, False)


def test_refusals_of_the_keep_bit_forms(dev):
    """Keep bits with a row list, with p not in {0, 1/2}, without ReLU, under the two-part scheme: GCN_E_BADARG, as
    the restated rule says, and nothing is stored."""
    from pygcn_amd import _native
    M = 5
    X, W = E.int_operand((M, 256), 81).to(dev), E.int_operand((256, 256), 82).to(dev)
    rows = torch.arange(M, dtype=torch.int32, device=dev)
    bits = torch.full((M + 5, 8), BITS_SENT, dtype=torch.int32, device=dev)
    bound = torch.full((1,), 8.0, device=dev)
    Yw = Window(M, 256, torch.float32, dev)
    for entry, r, relu, p, keep, mb in (("b3", rows, 1, 0.0, True, False), ("b3", rows, 0, 0.0, False, True),
                                        ("b3", None, 1, 0.3, True, False), ("b3", None, 0, 0.0, True, False),
                                        ("h2", None, 1, 0.0, True, False), ("h2", None, 0, 0.0, False, True)):
        with pytest.raises(E.Refused):
            E.expected_xw_kernel(entry, r is not None, relu=bool(relu), dropout_p=p, keep_bits_out=keep, mask_bits=mb)
        ep = _native.GcnGemmEpilogue(None, relu, p, SEED, None, None, 0, 1.0, None, 0,
                                     bits.data_ptr() if keep else None, bits.data_ptr() if mb else None)
        assert _call_xw(entry, X, r, W, Yw, M, ctypes.byref(ep), None, bound) == E.GCN_E_BADARG
    torch.cuda.synchronize()
    Yw.check(torch.full((M, 256), SENT, device=dev), "a refused launch stores nothing")
    _assert_same(bits, torch.full_like(bits, BITS_SENT), "a refused launch writes no keep bits")


# ------------------------------------------------------------------------------------------------
# the bf16 streaming product
# ------------------------------------------------------------------------------------------------
def _bf16_operands(K, N, M, dev):
    key = ("bf16", K, N, M)
    if key not in _OPERANDS:
        mx, mw = E.bf16_ranges(K)
        X = E.int_operand((M, K), 2000 + M, -mx, mx, torch.bfloat16).to(dev)
        W = E.int_operand((K, N), 2001 + K + N, -mw, mw, torch.bfloat16).to(dev)
        val = (X, W, E.exact_f32(E.product_ref(X, W)))
        if M < 1000:
            return val
        _OPERANDS[key] = val
    return _OPERANDS[key]


def _run_bf16_case(c, M, dev, oracle, pitched=False):
    L = _lib()
    K, N, store = c["K"], c["N"], c["store"]
    what = f"{case_id(c)} M={M}" + (" pitched" if pitched else "")
    assert E.expected_bf16_kernel(K, N, **E.STORES[store]) in set(E.parse_bf16_kernels())
    X, W, y32 = _bf16_operands(K, N, M, dev)
    if pitched:
        X, W = _pitched(X, K + 24), _pitched(W, N + 6, lead=1)     # ldw no multiple of 8, W 2 bytes off the grid
    st = Store(store, M, None, M, dev, oracle, dtype=torch.bfloat16, N=N, ld_mask=N + 8 if pitched else None, seed=M + K)
    Yw = Window(M, N, torch.bfloat16, dev, ld=N + 16, col0=8, guard=40) if pitched else Window(M, N, torch.bfloat16, dev)
    ws = _nan_ws(L.gcn_gemm_bf16_workspace_bytes(K, N), dev)
    _check(L.gcn_gemm_xw_bf16(X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0), Yw.ptr, Yw.ld, M, K, N,
                              st.byref(), ws.data_ptr(), ws.numel(), _stream()), what)
    # the epilogue on the exact fp32 accumulators, then ONE rounding to bf16 (exact for the plain product)
    exp = st.expected(y32).to(torch.bfloat16)
    if store == "plain":
        assert torch.equal(exp.float(), y32)
    Yw.check(exp, what)


@pytest.mark.parametrize("c", BF16_CASES, ids=case_id)
def test_bf16_product_is_the_float64_product_bit_for_bit(dev, oracle, c):
    """gcn_gemm_xw_bf16 through all 21 instantiations (three shapes x EPI 0..6) on integer operands whose fp32
    accumulators are integers of at most 256."""
    for M in c["heights"]:
        _run_bf16_case(c, M, dev, oracle)


@pytest.mark.parametrize("c", [c for c in BF16_CASES if len(c["heights"]) > 1], ids=case_id)
def test_bf16_product_pitches_and_guard_bands(dev, oracle, c):
    """ldx, ldy, ldw and ld_mask above the width, W's base 2 bytes off the 16-byte grid, guard columns on both
    sides of Y and guard rows below it."""
    for M in (1, 33, 129):
        _run_bf16_case(c, M, dev, oracle, pitched=True)


# ------------------------------------------------------------------------------------------------
# the weight gradient
# ------------------------------------------------------------------------------------------------
def _atg_list(listed, n_list, n_src, poison_row, seed, dev):
    """An index list of n_list entries padded to a multiple of 16 with entries that name the NaN-poisoned row: a
    padding entry must be a valid index, but the row it names must not be summed."""
    if listed:
        r = torch.randint(0, n_src, (n_list,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)
        if n_list >= 2:
            r[n_list // 2] = r[0]                          # duplicates
    else:
        r = torch.arange(n_list, dtype=torch.int32)
    pad = torch.full(((-n_list) % 16,), poison_row, dtype=torch.int32)
    return torch.cat([r, pad]).to(dev)


def _atg_operands(entry, n_list, lists, dev, census=None):
    key = ("atg", entry == "bf16", n_list, lists, census)
    if key in _OPERANDS:
        return _OPERANDS[key]
    width, dtype = (128, torch.bfloat16) if entry == "bf16" else (256, torch.float32)
    la, lg = lists in ("both", "a"), lists in ("both", "g")
    if census is None:
        n_a, n_g = (n_list + 9 if la else n_list), (n_list + 5 if lg else n_list)
        A = E.int_operand((n_a + 1, width), 3000 + n_list, dtype=dtype).to(dev)
        G = E.int_operand((n_g + 1, width), 3001 + n_list, dtype=dtype).to(dev)
    else:
        n_a = n_g = 256
        A, G = (torch.cat([t, torch.zeros(1, 256)]).to(dev) for t in E.census_atg(census, 256, 3100))
    A[n_a], G[n_g] = NAN, NAN                               # the row the padding entries name
    ra, rg = _atg_list(la, n_list, n_a, n_a, 3002 + n_list, dev), _atg_list(lg, n_list, n_g, n_g, 3003 + n_list, dev)
    if census is not None and la:
        # the census needs DISTINCT one-hot rows, the same for both operands: one shuffled list without duplicates
        perm = torch.randperm(256, generator=torch.Generator().manual_seed(3101))[:n_list].to(torch.int32).to(dev)
        ra, rg = ra.clone(), rg.clone()
        ra[:n_list], rg[:n_list] = perm, perm
    out64, cs64 = E.weight_grad_ref(A, G, ra, rg, n_list)
    A, G = _poison_unlisted(A, ra[:n_list]), _poison_unlisted(G, rg[:n_list])
    val = (A, ra, G, rg, E.exact_f32(out64), cs64)
    if n_list >= 1000:
        _OPERANDS[key] = val
    return val


def _run_atg(entry, n_list, lists, dev, pitched=False, census=None):
    L = _lib()
    A, ra, G, rg, out32, cs64 = _atg_operands(entry, n_list, lists, dev, census)
    what = f"weight gradient {entry} n_list={n_list} lists={lists}" + (" pitched" if pitched else "") + \
           (f" census {census}" if census else "")
    width = A.shape[1]
    if pitched:
        A, G = _pitched(A, 512), _pitched(G, 512)
    Ow = Window(width, width, torch.float32, dev, ld=512, col0=8, guard=40) if pitched else Window(width, width, torch.float32, dev)
    args = (A.data_ptr(), A.stride(0), ra.data_ptr(), G.data_ptr(), G.stride(0), rg.data_ptr(), n_list)
    if entry == "bf16":
        ws = _nan_ws(L.gcn_gemm_atg_bf16_workspace_bytes(n_list, 128, 128), dev)
        rc = L.gcn_gemm_atg_bf16(*args, 128, 128, Ow.ptr, Ow.ld, ws.data_ptr(), ws.numel(), _stream())
    else:
        ws = _nan_ws(L.gcn_gemm_atg256_workspace_bytes(n_list), dev)
        tail = (ws.data_ptr(), ws.numel(), _stream())
        if entry == "h2":
            b = torch.full((2,), 8.0, dtype=torch.float32, device=dev)
            rc = L.gcn_gemm_atg256_f32(*args, b.data_ptr(), b[1:].data_ptr(), Ow.ptr, Ow.ld, *tail)
        elif entry == "b3":
            rc = L.gcn_gemm_atg256_f32_b3(*args, Ow.ptr, Ow.ld, *tail)
        else:
            cs = torch.full((256 + 8,), SENT, dtype=torch.float32, device=dev)
            rc = L.gcn_gemm_atg256_f32_b3_colsum(*args, Ow.ptr, Ow.ld, cs.data_ptr(), *tail)
    _check(rc, what)
    Ow.check(out32, what)
    if entry == "b3_colsum":
        # the column sum equals the float64 sum exactly — wherever that sum is a float32 (integer operands; census
        # patterns whose G rows are one-hot: one term per column).  A dense census G has column sums of up to 256
        # terms over 80 binades, which no float32 holds: there only the guard behind the 256 sums is checked.
        cs32 = cs64.to(torch.float32)
        if torch.equal(cs32.double(), cs64):
            _assert_same(cs[:256], cs32, what + " column sums")
        else:
            assert census == "ii"
        _assert_same(cs[256:], torch.full((8,), SENT, device=dev), what + " behind the column sums")


@pytest.mark.parametrize("lists", E.ATG_LISTS)
@pytest.mark.parametrize("entry", E.ATG_ENTRIES)
def test_weight_gradient_is_the_float64_sum_bit_for_bit(dev, entry, lists):
    """gcn_gemm_atg256_f32 / _b3 / _b3_colsum / gcn_gemm_atg_bf16 on integer operands: both lists shuffled with
    duplicates, one of them, none (identity lists); unlisted rows and the row the padding names hold NaN."""
    for n_list in E.ATG_SMALL:
        _run_atg(entry, n_list, lists, dev)


@pytest.mark.parametrize("n_list", E.ATG_BIG)
@pytest.mark.parametrize("entry", E.ATG_ENTRIES)
def test_weight_gradient_over_many_workgroups(dev, entry, n_list):
    """32 800 entries are 1025 super-steps: 256 workgroups of which 51 get no work — their partial products must
    still count as zero; 70 001 entries leave the last workgroup a ragged slab."""
    _run_atg(entry, n_list, "both", dev)
    _run_atg(entry, n_list, "none", dev)


@pytest.mark.parametrize("entry", E.ATG_ENTRIES)
def test_weight_gradient_pitches_and_guard_bands(dev, entry):
    """lda = ldg = 512 (gaps NaN), `out` as the window [:, 8:8 + width] of a 512-wide buffer with guard rows."""
    for n_list in (17, 129):
        _run_atg(entry, n_list, "both", dev, pitched=True)


@pytest.mark.parametrize("case", E.CENSUS_CASES)
@pytest.mark.parametrize("entry", ["b3", "b3_colsum"])
def test_weight_gradient_census(dev, entry, case):
    """The three census patterns over a list of distinct one-hot rows: one product per element of the gradient."""
    for n_list, lists in ((256, "none"), (200, "both")):
        _run_atg(entry, n_list, lists, dev, census=case)


# ------------------------------------------------------------------------------------------------
# the Python wrappers forward the same results
# ------------------------------------------------------------------------------------------------
def test_the_wrappers_forward_the_same_results(dev, oracle, gemm_scheme):
    from pygcn_amd.gemm import gemm_bf16, gemm_keep_bits_usable, gemm_xw256, weight_grad_rows
    M = 257
    X, _, W, y32 = _xw_operands("int", M, None, dev)
    Xs, rows, _, y32s = _xw_operands("int", M, "shuffled", dev)
    bound = torch.full((1,), 8.0, device=dev)
    absmax = torch.zeros(1, device=dev)
    _assert_same(gemm_xw256(X, W, x_bound=bound, y_absmax=absmax), y32, "gemm_xw256")
    _assert_same(absmax, y32.abs().max().reshape(1), "gemm_xw256 y_absmax")
    _assert_same(gemm_xw256(Xs, W, x_bound=bound, rows=rows), y32s, "gemm_xw256 with rows")
    bias = E.int_bias(256, 5).to(dev)
    keep, scale = _keep(oracle, 0.5, M, 256, dev), oracle.dropout_scale(0.5)
    got = gemm_xw256(X, W, x_bound=bound, bias=bias, relu=True, dropout_p=0.5, seed=SEED, row_base=ROW_BASE)
    fwd = E.forward_store(y32, bias, True, keep, scale)
    _assert_same(got, fwd, "gemm_xw256 forward epilogue")
    mask = E.sign_mask((M + 37, 256), 6).to(dev)
    mrows = torch.randint(0, M + 37, (M,), generator=torch.Generator().manual_seed(9), dtype=torch.int32).to(dev)
    got = gemm_xw256(X, W, x_bound=bound, mask_src=mask, mask_rows=mrows, mask_scale=MASK_SCALE)
    _assert_same(got, E.masked_store(y32, mask, mrows, MASK_SCALE), "gemm_xw256 backward mask")
    if gemm_keep_bits_usable(X, None, 0.5):
        bits = torch.full((M, 8), BITS_SENT, dtype=torch.int32, device=dev)
        got = gemm_xw256(X, W, bias=bias, relu=True, dropout_p=0.5, seed=SEED, row_base=ROW_BASE, keep_bits_out=bits)
        _assert_same(got, fwd, "gemm_xw256 keep_bits_out")
        got = gemm_xw256(X, W, mask_src=fwd, mask_bits=bits, mask_scale=MASK_SCALE)
        _assert_same(got, E.masked_store(y32, fwd, torch.arange(M, device=dev), MASK_SCALE), "gemm_xw256 mask_bits")
    else:
        assert gemm_scheme == "h2"
    # the weight gradient: identity lists, unpadded lists (padded by the wrapper), the column sums
    n = 129
    A, ra, G, rg, out32, cs64 = _atg_operands("b3", n, "both", dev)
    _assert_same(weight_grad_rows(A, G, ra[:n].contiguous(), rg[:n].contiguous(), a_bound=bound, g_bound=bound), out32,
                 "weight_grad_rows with lists")
    A0, _, G0, _, out0, cs0 = _atg_operands("b3", n, "none", dev)
    _assert_same(weight_grad_rows(A0[:n], G0[:n], a_bound=bound, g_bound=bound), out0, "weight_grad_rows")
    if gemm_scheme == "bf16x3":
        got, cs = weight_grad_rows(A, G, ra[:n].contiguous(), rg[:n].contiguous(), colsum_g=True)
        _assert_same(got, out32, "weight_grad_rows colsum_g")
        _assert_same(cs, E.exact_f32(cs64), "weight_grad_rows column sums")
        # bf16 storage does not depend on the scheme: once
        Ab, rab, Gb, rgb, outb, _ = _atg_operands("bf16", n, "both", dev)
        got = weight_grad_rows(Ab, Gb, rab[:n].contiguous(), rgb[:n].contiguous())
        _assert_same(got, outb.to(torch.bfloat16), "weight_grad_rows bf16")
        for K, N in E.BF16_SHAPES:
            Xb, Wb, yb = _bf16_operands(K, N, 129, dev)
            _assert_same(gemm_bf16(Xb, Wb), yb.to(torch.bfloat16), f"gemm_bf16 {K}x{N}")
            bb = E.int_bias(N, 7).to(dev)
            kb = _keep(oracle, 0.5, 129, N, dev)
            got = gemm_bf16(Xb, Wb, bias=bb.to(torch.bfloat16), relu=True, dropout_p=0.5, seed=SEED, row_base=ROW_BASE)
            _assert_same(got, E.forward_store(yb, bb, True, kb, scale).to(torch.bfloat16), f"gemm_bf16 {K}x{N} forward epilogue")
            mb = E.sign_mask((129, N), 8, torch.bfloat16).to(dev)
            got = gemm_bf16(Xb, Wb, mask_src=mb, mask_scale=MASK_SCALE)
            _assert_same(got, E.masked_store(yb, mb, torch.arange(129, device=dev), MASK_SCALE).to(torch.bfloat16),
                         f"gemm_bf16 {K}x{N} backward mask")
