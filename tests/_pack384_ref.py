"""NumPy reference of the pooled 384-byte packed row format (include/gcn_spmm.h, gcn_rows_pack384): pack and unpack
in plain NumPy on the CPU — what tests/test_pack384_cpu.py and tests/test_pack384_gpu.py agree on.

A 256-wide fp32 row becomes one 384-byte slot = 96 uint32 words:
    words 0..7   words 2q, 2q + 1 = the 64-bit mask of column quarter q: columns 16 cb + 4 q + j (cb 0..15, j 0..3) at
                 bit 4 cb + j, set where the element's BIT PATTERN is non-zero (-0.0 is a stored value)
    word 8       the header: byte 0 = c0, byte 1 = c0 + c1, byte 2 = c0 + c1 + c2, byte 3 = min(total, 255)
                 (cq = the number of set bits of quarter q)
    words 9..95  ONE pool of values: quarter 0's in bit order, then quarters 1, 2 and 3
A row with more than CAPACITY = 87 values is overflowed: masks and header are valid, the value words undefined.  Words
past 9 + total are undefined."""
import numpy as np

CAPACITY = 87
WIDTH = 256
WORDS = 96
HEADER = 8
FIRST_VALUE = 9


def quarter_columns(q):
    """The 64 columns of quarter q in bit order."""
    return np.array([16 * cb + 4 * q + j for cb in range(16) for j in range(4)])


POOL_ORDER = np.concatenate([quarter_columns(q) for q in range(4)])       # the columns in the order of the pool


def overflowed(h):
    """bool [m]: the rows of h float32 [m, 256] that hold more than CAPACITY non-zero bit patterns."""
    return (np.ascontiguousarray(h, np.float32).view(np.uint32) != 0).sum(1) > CAPACITY


def pack384(h):
    """h float32 [m, 256] -> (slots uint32 [m, 96] with undefined words 0, defined bool [m, 96], overflow bool [m])."""
    h = np.ascontiguousarray(h, np.float32)
    assert h.ndim == 2 and h.shape[1] == WIDTH
    v = h.view(np.uint32)[:, POOL_ORDER]                          # [m, 256] in pool order
    nz = v != 0
    m = h.shape[0]
    slots = np.zeros((m, WORDS), np.uint32)
    defined = np.zeros((m, WORDS), bool)
    defined[:, :FIRST_VALUE] = True
    sh = np.arange(32, dtype=np.uint64)
    for w in range(8):                                            # mask word w = bits 32 w .. 32 w + 31 of the pool order
        slots[:, w] = (nz[:, 32 * w:32 * w + 32].astype(np.uint64) << sh).sum(1, dtype=np.uint64).astype(np.uint32)
    c = nz.reshape(m, 4, 64).sum(2).astype(np.uint32)             # [m, 4] quarter counts
    total = c.sum(1)
    slots[:, HEADER] = (c[:, 0] | ((c[:, 0] + c[:, 1]) << 8) | ((c[:, 0] + c[:, 1] + c[:, 2]) << 16)
                        | (np.minimum(total, 255) << 24)).astype(np.uint32)
    overflow = overflowed(h)
    for r in np.flatnonzero(~overflow):
        t = int(total[r])
        slots[r, FIRST_VALUE:FIRST_VALUE + t] = v[r][nz[r]]
        defined[r, FIRST_VALUE:FIRST_VALUE + t] = True
    return slots, defined, overflow


def unpack384(slots):
    """slots uint32 [m, 96] -> (h float32 [m, 256], overflow bool [m]).  Overflowed rows come back as zeros: a reader
    must take their dense row.  Checks the header against the masks."""
    slots = np.asarray(slots).view(np.uint32).reshape(-1, WORDS)
    m = slots.shape[0]
    sh = np.arange(32, dtype=np.uint32)
    nz = ((slots[:, :8, None] >> sh) & 1).astype(bool).reshape(m, WIDTH)           # pool order
    c = nz.reshape(m, 4, 64).sum(2).astype(np.uint32)
    total = c.sum(1)
    hdr = slots[:, HEADER]
    assert np.array_equal(hdr & 0xFF, c[:, 0]) and np.array_equal((hdr >> 8) & 0xFF, c[:, 0] + c[:, 1]) \
        and np.array_equal((hdr >> 16) & 0xFF, c[:, 0] + c[:, 1] + c[:, 2]) \
        and np.array_equal(hdr >> 24, np.minimum(total, 255)), "header != counts of the masks"
    overflow = total > CAPACITY
    pooled = np.zeros((m, WIDTH), np.uint32)
    for r in np.flatnonzero(~overflow):
        pooled[r, nz[r]] = slots[r, FIRST_VALUE:FIRST_VALUE + int(total[r])]
    bits = np.zeros((m, WIDTH), np.uint32)
    bits[:, POOL_ORDER] = pooled
    return bits.view(np.float32), overflow


def row_with_counts(counts, rng, high=False):
    """One float32 [256] row with counts[q] non-zeros in quarter q, at random bits (high: the highest bits)."""
    row = np.zeros(WIDTH, np.float32)
    for q, k in enumerate(counts):
        pick = np.arange(64 - k, 64) if high else np.sort(rng.permutation(64)[:k])
        row[quarter_columns(q)[pick]] = rng.random(k).astype(np.float32) + 0.5
    return row


def special_rows():
    """float32 [10, 256]: the edge rows of the format, and (name -> row)."""
    rng = np.random.default_rng(384)
    rows, names = [], {}

    def add(name, row):
        names[name] = len(rows)
        rows.append(row)
    add("total 86", row_with_counts((22, 21, 22, 21), rng))
    add("total 87", row_with_counts((22, 22, 22, 21), rng))
    add("total 88", row_with_counts((22, 22, 22, 22), rng))
    add("64 0 0 23", row_with_counts((64, 0, 0, 23), rng))
    add("0 0 23 64", row_with_counts((0, 0, 23, 64), rng))
    add("all set", (rng.random(WIDTH).astype(np.float32) + 0.5))
    add("all zero", np.zeros(WIDTH, np.float32))
    s = row_with_counts((10, 10, 10, 10), rng)
    s[[1, 17, 35, 255, 100, 101]] = np.array([0x80000000, 0x7FC00000, 0x7F800000, 0xFF800000, 1, 0x807FFFFF],
                                             np.uint32).view(np.float32)     # -0.0, NaN, +-inf, two denormals
    add("special values", s)
    add("87 in the highest bits", row_with_counts((22, 22, 22, 21), rng, high=True))
    add("all -0.0", np.full(WIDTH, -0.0, np.float32))
    return np.stack(rows), names
