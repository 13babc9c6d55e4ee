"""NumPy reference of the fixed-slot packed row format (include/gcn_spmm.h, gcn_rows_pack512): pack and expand,
in plain NumPy on the CPU — what tests/test_packed_hidden_cpu.py and tests/test_packed_hidden_gpu.py agree on.

A 256-wide fp32 row becomes one 512-byte slot = 128 uint32 words = four sub-slots of 32 words, one per column
quarter q: columns 16 cb + 4 q + j (cb 0..15, j 0..3) at bit 4 cb + j.  Sub-slot: [0] [1] the 64-bit mask of the
elements whose BIT PATTERN is non-zero, [2] their number, [3 ..] the values in bit order; a quarter with more than
CAPACITY values overflows (its first CAPACITY values are stored) and marks its row."""
import numpy as np

CAPACITY = 29
WIDTH = 256


def quarter_columns(q):
    """The 64 columns of quarter q in bit order."""
    return np.array([16 * cb + 4 * q + j for cb in range(16) for j in range(4)])


def pack(h):
    """h float32 [m, 256] -> (slots uint32 [m, 128] with unwritten words 0, written bool [m, 128], overflow bool [m])."""
    h = np.ascontiguousarray(h, np.float32)
    assert h.ndim == 2 and h.shape[1] == WIDTH
    bits = h.view(np.uint32)
    m = h.shape[0]
    slots = np.zeros((m, 128), np.uint32)
    written = np.zeros((m, 128), bool)
    overflow = np.zeros(m, bool)
    for q in range(4):
        v = bits[:, quarter_columns(q)]                       # [m, 64] in bit order
        nz = v != 0
        mask = (nz.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(1, dtype=np.uint64)
        count = nz.sum(1)
        base = 32 * q
        slots[:, base] = (mask & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        slots[:, base + 1] = (mask >> np.uint64(32)).astype(np.uint32)
        slots[:, base + 2] = count.astype(np.uint32)
        written[:, base:base + 3] = True
        overflow |= count > CAPACITY
        for r in range(m):
            vals = v[r][nz[r]][:CAPACITY]
            slots[r, base + 3: base + 3 + vals.size] = vals
            written[r, base + 3: base + 3 + vals.size] = True
    return slots, written, overflow


def expand(slots):
    """slots uint32 [m, 128] -> (h float32 [m, 256], overflow bool [m]).  Rows that overflowed come back with the
    values that were stored (the first CAPACITY of an overflowed quarter) and zeros for the rest of that quarter:
    a reader must take their dense row."""
    slots = np.asarray(slots).view(np.uint32).reshape(-1, 128)
    m = slots.shape[0]
    bits = np.zeros((m, WIDTH), np.uint32)
    overflow = np.zeros(m, bool)
    for q in range(4):
        base = 32 * q
        mask = slots[:, base].astype(np.uint64) | (slots[:, base + 1].astype(np.uint64) << np.uint64(32))
        nz = ((mask[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)      # [m, 64]
        count = slots[:, base + 2].astype(np.int64)
        assert np.array_equal(count, nz.sum(1)), "count word != popcount(mask)"
        overflow |= count > CAPACITY
        cols = quarter_columns(q)
        for r in range(m):
            idx = np.flatnonzero(nz[r])[:CAPACITY]
            bits[r, cols[idx]] = slots[r, base + 3: base + 3 + idx.size]
    return bits.view(np.float32), overflow


def special_rows():
    """float32 [12, 256]: the edge cases of the format — quarters at capacity, one over, all 64 set; -0.0, NaN,
    +-inf as stored values; an empty row.  (row -> what it holds) in `names`."""
    rng = np.random.default_rng(512)
    h = np.zeros((12, WIDTH), np.float32)
    names = {}

    def fill(r, q, k, name):
        cols = quarter_columns(q)[rng.permutation(64)[:k]]
        h[r, cols] = rng.standard_normal(k).astype(np.float32) + 3.0
        names[name] = r
    fill(0, 0, CAPACITY, "quarter 0 at capacity")
    fill(1, 3, CAPACITY, "quarter 3 at capacity")
    fill(2, 1, CAPACITY + 1, "quarter 1 one over")
    fill(3, 2, 64, "quarter 2 all set")
    for q in range(4):
        fill(4, q, CAPACITY, "every quarter at capacity")
    fill(5, 0, 10, "special values")
    h[5, [1, 17, 35, 255]] = [-0.0, np.nan, np.inf, -np.inf]
    names["empty"] = 6
    h[7, :] = -0.0                                              # 256 stored values: all four quarters overflow
    names["all -0.0"] = 7
    fill(8, 0, 1, "one value")
    h[9, quarter_columns(2)[63]] = 5.0                          # the last bit of a mask alone
    names["last bit"] = 9
    h[10, quarter_columns(1)[:CAPACITY]] = np.arange(1, CAPACITY + 1, dtype=np.float32)   # the lowest bits
    names["low bits"] = 10
    h[11, quarter_columns(1)[64 - CAPACITY:]] = np.arange(1, CAPACITY + 1, dtype=np.float32)   # the highest bits
    names["high bits"] = 11
    return h, names
