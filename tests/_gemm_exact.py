"""Exactly summable operands for the dense-product kernels of pygcn_amd/csrc/gcn_gemm.hip, their
float64 references, the host dispatch restated in Python and the one case table that
tests/test_gemm_exact_cpu.py (no GPU) and tests/test_gemm_exact_gpu.py iterate over.

Plain torch / numpy: nothing here calls a pygcn_amd kernel.  The idea: on operands whose
part products and partial sums are all exactly representable in float32, EVERY summation order gives
the float64 result bit for bit — so a kernel instantiation that differs from the reference in one
element has an indexing, staging, dispatch or missing-term error, never a rounding difference, and
the comparison needs no tolerance."""
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEMM_SOURCE = os.path.join(ROOT, "pygcn_amd", "csrc", "gcn_gemm.hip")

GCN_E_BADARG, GCN_E_ALIGN = -1, -2
ENVELOPE_MIN = 1e-30          # the three-part scheme keeps full accuracy for 1e-30 <= |x| (gemm_xw256's docstring)

# The six part products the three-part scheme keeps, as (part of the left operand, part of the right
# operand): every term down to 2^-16 of the leading one (include/gcn_spmm.h, gcn_gemm_xw256_f32_b3).
KEPT_PRODUCTS = (("h", "h"), ("h", "m"), ("m", "h"), ("h", "l"), ("l", "h"), ("m", "m"))


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


# ------------------------------------------------------------------------------------------------
# a. operand builders
# ------------------------------------------------------------------------------------------------
def int_operand(shape, seed, lo=-8, hi=8, dtype=torch.float32, zero_fraction=0.0):
    """Integers in [lo, hi] as `dtype`.

    Exact because: with |x|, |w| <= 8 every product is an integer of at most 64, and any partial sum
    of at most 2^18 of them, in any order, is an integer below 2^24 — float32 holds it exactly.  An
    integer of at most 8 has 4 significant bits: it is its own leading bf16 part (m = l = 0) and,
    scaled by a power of two, its own leading fp16 part, so every kept part product is one of these
    integers or zero.  For bf16 STORAGE (dtype=torch.bfloat16) the caller picks [lo, hi] with
    K * max|x| * max|w| <= 256: the fp32 accumulator then holds an integer of at most 256, which the
    single rounding to bf16 (8 significant bits) keeps."""
    g = _gen(seed)
    v = torch.randint(lo, hi + 1, tuple(shape), generator=g).to(torch.float32)
    if zero_fraction > 0.0:
        v = torch.where(torch.rand(tuple(shape), generator=g) < zero_fraction, torch.zeros(()), v)
    return v.to(dtype)


def _census_values(shape, seed, third_part, e_range=40):
    g = _gen(seed)
    e = torch.randint(-e_range, e_range + 1, tuple(shape), generator=g).double()
    sign = torch.randint(0, 2, tuple(shape), generator=g).double() * 2 - 1
    mant = 1.0 + 2.0 ** -9 + (2.0 ** -17 if third_part else 0.0)
    return (sign * mant * torch.pow(torch.tensor(2.0, dtype=torch.float64), e)).to(torch.float32)


def census_c3(shape, seed):
    """±2^e (1 + 2^-9 + 2^-17), e random in [-40, 40]: bf16 parts h = ±2^e, m = ±2^(e-9), l = ±2^(e-17).

    Exact because: the value has 18 significant bits (a float32); rounding to bf16 (8 bits) drops
    2^-9 + 2^-17 < half an ulp of 2^-7, the remainder 2^-9 (1 + 2^-8) is a tie that rounds to the even
    2^-9, and 2^-17 is left as the third part.  Every subset sum of such parts — and of their products
    with one power of two — has at most 18 significant bits, so any order of adding them is exact."""
    return _census_values(shape, seed, True)


def census_c2(shape, seed):
    """±2^e (1 + 2^-9): bf16 parts h = ±2^e, m = ±2^(e-9), l = 0.

    Exact because: the product of two such values is ±2^(e+k) (1 + 2^-8 + 2^-18) = hh + hm + mh + mm,
    19 significant bits, and every subset sum of the four terms has no more."""
    return _census_values(shape, seed, False)


def pow2_signed(shape, seed, k_range=20):
    """±2^k, k random in [-k_range, k_range]: one bf16 part (m = l = 0); multiplying by it is exact."""
    g = _gen(seed)
    k = torch.randint(-k_range, k_range + 1, tuple(shape), generator=g).double()
    sign = torch.randint(0, 2, tuple(shape), generator=g).double() * 2 - 1
    return (sign * torch.pow(torch.tensor(2.0, dtype=torch.float64), k)).to(torch.float32)


def one_hot_rows(n, columns, values):
    """[n, 256] with row r = values[r] * e_{columns[r]}."""
    out = torch.zeros(n, 256, dtype=torch.float32)
    out[torch.arange(n), columns] = values
    return out


CENSUS_CASES = ("i", "ii", "iii")
# which of the six kept part products a census case makes visible (left part, right part)
CENSUS_NEEDS = {"i": {("h", "h"), ("m", "h"), ("l", "h")},
                "ii": {("h", "h"), ("h", "m"), ("h", "l")},
                "iii": {("h", "h"), ("h", "m"), ("m", "h"), ("m", "m")}}


def census_xw(case, M, seed):
    """(X [M, 256], W [256, 256]) of census case (i), (ii) or (iii): every output element is ONE non-zero
    product, so a dropped part product changes it and no summation can hide or round anything.
      (i)   X dense c3, W = diag(±2^k):           Y[r, c] = X[r, c] W[c, c]      needs hh, mh, lh
      (ii)  X row r = ±2^k e_{r mod 256}, W dense c3: Y[r, c] = X[r, j] W[j, c]   needs hh, hm, hl
      (iii) X dense c2, W = diag(c2):             Y[r, c] = X[r, c] W[c, c]      needs hh, hm, mh, mm."""
    if case == "i":
        return census_c3((M, 256), seed), torch.diag(pow2_signed((256,), seed + 1))
    if case == "ii":
        return (one_hot_rows(M, torch.arange(M) % 256, pow2_signed((M,), seed + 1)), census_c3((256, 256), seed))
    if case == "iii":
        return census_c2((M, 256), seed), torch.diag(census_c2((256,), seed + 1))
    raise ValueError(case)


def census_atg(case, n, seed):
    """(A [n, 256], G [n, 256]), n <= 256, the same three patterns for the weight gradient
    out = Σ_r A[r]ᵀ ⊗ G[r]: the one-hot rows sit at DISTINCT columns π(r), so out has one product per element.
      (i)   A dense c3, G[r] = ±2^k e_π(r);  (ii) A[r] = ±2^k e_π(r), G dense c3;  (iii) A dense c2, G[r] = c2 e_π(r)."""
    assert n <= 256
    perm = torch.randperm(256, generator=_gen(seed + 2))[:n]
    if case == "i":
        return census_c3((n, 256), seed), one_hot_rows(n, perm, pow2_signed((n,), seed + 1))
    if case == "ii":
        return one_hot_rows(n, perm, pow2_signed((n,), seed + 1)), census_c3((n, 256), seed)
    if case == "iii":
        return census_c2((n, 256), seed), one_hot_rows(n, perm, census_c2((n,), seed + 1))
    raise ValueError(case)


def sign_mask(shape, seed, dtype=torch.float32):
    """A backward mask with every sign pattern `mask > 0` has to tell apart: negative, -0.0, +0.0, a
    small and an ordinary positive value (1e-30 — 2^-100 for bf16 — is a normal number in both types)."""
    small = 2.0 ** -100
    table = torch.tensor([-2.0, -0.0, 0.0, small, 1.0, 3.0, -small], dtype=torch.float32)
    idx = torch.randint(0, table.numel(), tuple(shape), generator=_gen(seed))
    return table[idx].to(dtype)


# ------------------------------------------------------------------------------------------------
# b. the split, emulated
# ------------------------------------------------------------------------------------------------
def _bf16_round(x):
    return x.to(torch.bfloat16).to(torch.float32)


def split3(x):
    """split3 of gcn_gemm.hip: h = bf16(x), m = bf16(x - h), l = bf16((x - h) - m), as float32 tensors
    (round to nearest even, three times; the subtractions are exact)."""
    x = x.to(torch.float32)
    h = _bf16_round(x)
    r1 = x - h
    m = _bf16_round(r1)
    return {"h": h, "m": m, "l": _bf16_round(r1 - m)}


def emulated_product(X, W, without=None):
    """The three-part product as the kernels form it, in float64: Σ over the KEPT part products of
    part(X) · part(W) — all six, or all but `without`.  For the CPU tests only."""
    px, pw = split3(X), split3(W)
    acc = torch.zeros(X.shape[0], W.shape[1], dtype=torch.float64)
    for a, b in KEPT_PRODUCTS:
        if (a, b) != without:
            acc += px[a].double() @ pw[b].double()
    return acc


# ------------------------------------------------------------------------------------------------
# c. references (any device: they follow their operands)
# ------------------------------------------------------------------------------------------------
def exact_f32(ref64):
    """float64 -> float32, asserting that nothing is rounded: the operands kept their promise."""
    out = ref64.to(torch.float32)
    assert torch.equal(out.double(), ref64), "the float64 reference is not a float32: the operands are not exact"
    return out


def product_ref(X, W, rows=None):
    """float64 X[rows] · W."""
    src = X if rows is None else X.index_select(0, rows.long())
    return src.double() @ W.double()


def weight_grad_ref(A, G, rows_a=None, rows_g=None, n_list=None):
    """float64 Σ_{r < n_list} A[rows_a[r]]ᵀ ⊗ G[rows_g[r]] and the column sums of the listed G rows."""
    a = A if rows_a is None else A.index_select(0, rows_a[:n_list].long())
    g = G if rows_g is None else G.index_select(0, rows_g[:n_list].long())
    a, g = a[:n_list].double(), g[:n_list].double()
    return a.t() @ g, g.sum(0)


def int_bias(n, seed):
    return int_operand((n,), seed, -8, 8)


def forward_store(y32, bias=None, relu=False, keep=None, scale=None):
    """What a forward epilogue stores for the exact float32 accumulators y32:
    y + bias (integers: exact), max(., 0), then keep ? float32(y) * float32(scale) : 0 — one rounding
    (none at p = 1/2, where the scale is 2).  `keep`: bool tensor from oracle.dropout_keep, `scale`:
    oracle.dropout_scale's float32."""
    y = y32.to(torch.float32)
    if bias is not None:
        y = y + bias.to(y.device, torch.float32)
    if relu:
        y = torch.clamp_min(y, 0.0)
    if keep is not None:
        s = torch.tensor(float(scale), dtype=torch.float32, device=y.device)
        y = torch.where(keep.to(y.device), y * s, torch.zeros((), dtype=torch.float32, device=y.device))
    return y


def masked_store(y32, mask, mask_row_index, scale):
    """What the backward-mask store section stores: mask[mask_row_index[r], c] > 0 ? y * scale : 0
    (`scale` such as 1.5 keeps integers exact in float32)."""
    y = y32.to(torch.float32)
    m = mask.index_select(0, mask_row_index.long()).to(torch.float32)
    s = torch.tensor(float(scale), dtype=torch.float32, device=y.device)
    return torch.where(m > 0, y * s, torch.zeros((), dtype=torch.float32, device=y.device))


def mask_row_index(M, x_rows=None, mask_rows=None, device="cpu"):
    """The mask row of output row r: mask_rows[r] if given, else the INPUT row (x_rows[r], or r)."""
    if mask_rows is not None:
        return mask_rows[:M].long()
    if x_rows is not None:
        return x_rows[:M].long()
    return torch.arange(M, device=device)


def keep_bits_decode(bits, M):
    """bool [M, 256] from the kernel's keep bits ([>= M, 8] int32, H2Epi in gcn_gemm.hip): bit 4 c + j of word
    2 q + w of row r <-> column 16 (8 w + c) + 4 q + j."""
    b = bits[:M].to(torch.int64) & 0xFFFFFFFF
    col = torch.arange(256, device=bits.device)
    j, q, cw = col & 3, (col >> 2) & 3, col >> 4
    w, c = cw >> 3, cw & 7
    return ((b[:, 2 * q + w] >> (4 * c + j)) & 1).bool()


# ------------------------------------------------------------------------------------------------
# d. the host dispatch, restated
# ------------------------------------------------------------------------------------------------
class Refused(Exception):
    """The entry point answers these options with an error code instead of a launch."""
    def __init__(self, code, why):
        super().__init__(why)
        self.code = code


def dropout_threshold16(p):
    """gcn_dropout_threshold16: keep iff the 16-bit field >= round(p 2^16), clamped to [1, 65535]; 0 = off."""
    p = float(np.float32(p))
    if not p > 0.0:
        return 0
    return int(min(65535.0, max(1.0, float(int(p * 65536.0 + 0.5)))))


def _store_section(who, bias, relu, dropout_p, mask_src, mask_bits):
    if not (dropout_p >= 0.0) or dropout_p >= 1.0:
        raise Refused(GCN_E_BADARG, f"{who}: dropout_p must be in [0, 1)")
    if dropout_p > 0.0 and not relu:
        raise Refused(GCN_E_BADARG, f"{who}: dropout needs relu")
    if (mask_src or mask_bits) and (bias or relu or dropout_p > 0.0):
        raise Refused(GCN_E_BADARG, f"{who}: forward epilogue and backward mask exclude each other")
    thresh = dropout_threshold16(dropout_p)
    fwd = bool(bias or relu or thresh != 0)
    return fwd, thresh


def expected_xw_kernel(scheme, has_rows, bias=False, relu=False, dropout_p=0.0, mask_src=False, mask_bits=False,
                       keep_bits_out=False, ldx=256, ldy=256):
    """(form, EPI, BITS) as xw256_launch chooses among XwKernels — scheme "h2" (gcn_gemm_xw256_f32_h2) or "b3"
    (gcn_gemm_xw256_f32_b3); form 0 / 1: gemm_xw256_h2_kernel<EPI, form>, 2: gemm_xw256_s16_kernel<EPI, BITS>.
    Raises Refused where the host code refuses."""
    who = "gcn_gemm_xw256_f32_" + scheme
    sch = {"h2": 0, "b3": 1}[scheme]
    fwd, thresh = _store_section(who, bias, relu, dropout_p, mask_src, mask_bits)
    if ldx < 256 or ldy < 256:
        raise Refused(GCN_E_BADARG, f"{who}: bad sizes")
    if ldx % 4 or ldy % 4:
        raise Refused(GCN_E_ALIGN, f"{who}: X / Y rows must be 16-byte aligned")
    if not fwd:
        epi = 3 if mask_bits else (2 if mask_src else 0)
    else:
        epi = 1 if not relu else (4 if thresh == 0 else (5 if thresh == 32768 else 6))
    s16 = sch == 1 and not has_rows and epi != 6 and ldx < (1 << 21) and ldy < (1 << 21)
    if (mask_bits or keep_bits_out) and not (s16 and ((not fwd) if mask_bits else bool(relu))):
        raise Refused(GCN_E_BADARG, f"{who}: keep_bits_out / mask_bits need contiguous rows, the three-part scheme, "
                                    "ReLU with dropout_p in {0, 1/2} or no forward epilogue")
    return (2 if s16 else sch, epi, bool(keep_bits_out and fwd))


BF16_SHAPES = ((128, 128), (128, 256), (256, 128))


def expected_bf16_kernel(K, N, bias=False, relu=False, dropout_p=0.0, mask_src=False, mask_rows=False):
    """(K, N, EPI) of gemm_bf16_kernel as gcn_gemm_xw_bf16 chooses (the GCN_LAUNCH_BF16 chain)."""
    who = "gcn_gemm_xw_bf16"
    fwd, thresh = _store_section(who, bias, relu, dropout_p, mask_src, False)
    if (K, N) not in BF16_SHAPES:
        raise Refused(GCN_E_BADARG, f"{who}: (K, N) must be (128,128), (128,256) or (256,128)")
    if fwd:
        epi = 1 if not relu else (4 if thresh == 0 else (5 if thresh == 32768 else 6))
    else:
        epi = 0 if not mask_src else (2 if not mask_rows else 3)
    return (K, N, epi)


def parse_xw_kernels(source=None):
    """The instantiations of `using XwKernels = XwList<...>` as a list of (form, EPI, BITS)."""
    text = source if source is not None else open(GEMM_SOURCE).read()
    m = re.search(r"using\s+XwKernels\s*=\s*XwList<(.*?)>\s*;", text, re.S)
    assert m, "gcn_gemm.hip no longer defines XwKernels as one XwList<...>"
    items = re.findall(r"Xw<\s*(\d+)\s*,\s*(\d+)\s*(?:,\s*(true|false)\s*)?>", m.group(1))
    assert len(items) == m.group(1).count("Xw<")
    return [(int(f), int(e), b == "true") for f, e, b in items]


def parse_bf16_kernels(source=None):
    """The instantiations gcn_gemm_xw_bf16 can launch: (shapes of the GCN_LAUNCH_BF16(K, N) calls) x (the EPI
    values of the GCN_LAUNCH_BF16_E(KK, NN, EPI) chain), as a list of (K, N, EPI)."""
    text = source if source is not None else open(GEMM_SOURCE).read()
    epis = [int(e) for e in re.findall(r"GCN_LAUNCH_BF16_E\(KK,\s*NN,\s*(\d+)\)", text)]
    shapes = [(int(k), int(n)) for k, n in re.findall(r"GCN_LAUNCH_BF16\((\d+),\s*(\d+)\)", text)]
    assert epis and shapes, "gcn_gemm.hip no longer launches gemm_bf16_kernel through GCN_LAUNCH_BF16"
    assert len(set(epis)) == len(epis) and len(set(shapes)) == len(shapes)
    return [(k, n, e) for k, n in shapes for e in epis]


# ------------------------------------------------------------------------------------------------
# e. the case table
# ------------------------------------------------------------------------------------------------
# store sections by name -> the epilogue fields that select them
STORES = {
    "plain": dict(),
    "bias": dict(bias=True),
    "bias_relu": dict(bias=True, relu=True),
    "drop_half": dict(bias=True, relu=True, dropout_p=0.5),
    "drop_03": dict(bias=True, relu=True, dropout_p=0.3),
    "mask": dict(mask_src=True),                           # read at the input row
    "mask_rows": dict(mask_src=True, mask_rows=True),      # read through mask_rows
    "keep_p0": dict(relu=True, keep_bits_out=True),
    "keep_half": dict(bias=True, relu=True, dropout_p=0.5, keep_bits_out=True),
    "mask_bits": dict(mask_bits=True),
    "mask_bits_rows": dict(mask_bits=True, mask_rows=True),
}
KEEP_BIT_STORES = ("keep_p0", "keep_half", "mask_bits", "mask_bits_rows")


def dispatch_fields(store):
    """The fields of STORES[store] that decide the instantiation of the 256 x 256 product."""
    f = dict(STORES[store])
    f.pop("mask_rows", None)
    return f


# heights: the smallest that reach each path of a kernel (one row, a partial MFMA tile, one tile and
# its neighbours, one workgroup tile and its neighbours), and the height at which two of the 256
# persistent workgroups carry a second tile, one of them a single row
S16_SMALL, S16_BIG = (1, 15, 16, 17, 127, 128, 129), 128 * 256 + 128 + 1
T256_SMALL, T256_BIG = (1, 31, 32, 33, 255, 256, 257), 256 * 256 + 256 + 1
BIG_STORES = ("plain", "drop_half", "mask_rows")          # big heights: plain, one forward, one masked section
BIG_STORES_S16 = BIG_STORES + KEEP_BIT_STORES


def _xw_cases():
    cases = []
    # integer operands through every instantiation; x_rows: None = contiguous, "shuffled" = a shuffled list
    # with duplicates over a NaN-poisoned source
    for scheme in ("b3", "h2"):
        for rows in (None, "shuffled"):
            for store in STORES:
                if store in KEEP_BIT_STORES and (scheme != "b3" or rows is not None):
                    continue                               # (refused: see test_the_restated_rule_refuses...)
                s16 = scheme == "b3" and rows is None and store != "drop_03"
                cases.append(dict(entry=scheme, rows=rows, store=store, operands="int",
                                  heights=S16_SMALL if s16 else T256_SMALL))
                big = BIG_STORES_S16 if s16 else BIG_STORES
                if store in big:
                    cases.append(dict(entry=scheme, rows=rows, store=store, operands="int",
                                      heights=(S16_BIG if s16 else T256_BIG,)))
    # the census: both kernels behind _b3 (contiguous rows; an identity and a shuffled row list), plain + one
    # forward + one masked section each
    for case in CENSUS_CASES:
        for rows in (None, "identity", "shuffled"):
            for store in ("plain", "bias_relu", "mask"):
                cases.append(dict(entry="b3", rows=rows, store=store, operands="census_" + case,
                                  heights=(129,) if rows is None else (257,)))
    return cases


XW_CASES = _xw_cases()
# round 1's kernel (gcn_gemm_xw256_f32: no row list, no epilogue) is no member of XwKernels
R1_CASES = ([dict(operands="int", heights=T256_SMALL), dict(operands="int", heights=(T256_BIG,))]
            + [dict(operands="census_" + c, heights=(257,)) for c in CENSUS_CASES])

BF16_SMALL, BF16_BIG = (1, 31, 32, 33, 127, 129), 98305     # 98 305: persistent workgroups take a second round
BF16_STORES = ("plain", "bias", "bias_relu", "drop_half", "drop_03", "mask", "mask_rows")
BF16_CASES = [dict(K=K, N=N, store=store, heights=BF16_SMALL) for K, N in BF16_SHAPES for store in BF16_STORES] + \
             [dict(K=K, N=N, store=store, heights=(BF16_BIG,)) for K, N in BF16_SHAPES
              for store in ("plain", "drop_half", "mask_rows")]


def bf16_ranges(K):
    """(max|x|, max|w|) of integer operands with K * max|x| * max|w| <= 256 (int_operand's docstring)."""
    return (1, 2) if K == 128 else (1, 1)


ATG_ENTRIES = ("h2", "b3", "b3_colsum", "bf16")             # gcn_gemm_atg256_f32, _b3, _b3_colsum, gcn_gemm_atg_bf16
ATG_SMALL = (1, 15, 16, 17, 31, 32, 33, 129)
ATG_BIG = (32800, 70001)        # 32 800 = 1025 super-steps: 256 workgroups of which 51 get no work
ATG_LISTS = ("both", "a", "g", "none")                      # which operand is read through a (shuffled, duplicated) list


def atg_wgs(n_list):
    """atg_wgs of gcn_gemm.hip: workgroups (= partial products the reduction adds), and how many of them get no
    super-step."""
    supers = (n_list + 31) // 32
    n_wg = max(1, min(256, (supers + 3) // 4))
    per = (supers + n_wg - 1) // n_wg
    return n_wg, n_wg - (supers + per - 1) // per


def reached_xw(cases=None):
    """The XwKernels instantiations the case table reaches through the restated dispatch."""
    out = set()
    for c in (XW_CASES if cases is None else cases):
        out.add(expected_xw_kernel(c["entry"], c["rows"] is not None, **dispatch_fields(c["store"])))
    return out


def reached_bf16(cases=None):
    out = set()
    for c in (BF16_CASES if cases is None else cases):
        f = STORES[c["store"]]
        out.add(expected_bf16_kernel(c["K"], c["N"], **f))
    return out


def case_id(c):
    parts = [str(c[k]) for k in ("entry", "K", "N", "rows", "store", "operands") if k in c and c[k] is not None]
    h = c["heights"]
    parts.append("M%d" % h[0] if len(h) == 1 else "small")
    return "-".join(parts)
