"""Tables past 4 GiB and past 2^23 rows for the kernel tests (tests/test_large_tables.py, tests/test_large_tables_host.py).

The low-level entries take a table as (pointer, rows, row stride), so the largest offsets and ids are reached with the
smallest work:

SPARSE-GIANT.  One float32 buffer filled with NaN; every table of a case is an ``as_strided((n_rows, k_int), (LD, 1))`` view
of it at its own column offset (COL).  LD = 2^19 + 4 floats = 2 097 168 bytes per row, so 8200 rows span 16.02 GiB and cross
bytes 2^31, 2^32, 2^33, 2^34 between rows 1023|1024, 2047|2048, 4095|4096, 8191|8192 (4104 rows: the first three).  A read
through a wrong address returns NaN; a store through one lands on a NaN cell and changes ``count_written``.

MANY-NARROW.  2^24 + 2^23 + 5 rows of 4 floats (400 MB), values a function of (row, column), filled on the device.

COMPACT TWIN.  The same rows in an ordinary ``alloc_table`` table and the same call: entries that read every row keep all rows
and the identical ids; entries that touch only some rows gather them in ascending id order (``Remap``), a monotone remap, which
keeps destination order, segment order and therefore the float summation order.

This module imports torch only inside the functions that need a device: the arithmetic (spans, probes, truncations, the
grouping workspace's layout, the remap) is plain integers and numpy, and the host tests use it without a GPU."""
import numpy as np

F32 = np.float32

LD = (1 << 19) + 4                    # floats per arena row: 2 097 168 bytes, 16-byte aligned
SPAN_LARGE, SPAN_SMALL = 8200, 4104   # rows: 16.02 GiB / 8.02 GiB
# column offsets of the tables inside an arena row; every table is at most 2048 floats wide
COL = {"ent": 0, "rel": 2048, "ent_s0": 4096, "ent_s1": 6144, "rel_s0": 8192, "rel_s1": 10240, "img": 12288, "img2": 14336}
TABLE_WIDTH = 2048
ARENA_COLS = 16384                    # the columns any table may own; [ARENA_COLS, LD) is never written
# a case may initialise any table on EVERY row (the entries that read every row; Adam's dense pass walks the states too)
DENSE_TABLES = tuple(COL)
MARK_ROWS = (0, 1, 1023, 1024, 2047, 2048, 4095, 4096, 8191, 8192)
COUNT_CHUNK = 1 << 24                 # floats per chunk of count_written: 64 MB, its temporaries 16 MB + 8 bytes


def padded(k_int):
    """row width of training.alloc_table: a multiple of 4 floats"""
    return (k_int + 3) // 4 * 4


def arena_floats(n_rows):
    return (n_rows - 1) * LD + ARENA_COLS


def arena_bytes(n_rows):
    return 4 * arena_floats(n_rows)


def probe_rows(n_rows, n_random=50, seed=20):
    """ascending distinct rows: the marks on both sides of every 2^31 / 2^32 / 2^33 / 2^34 byte crossing inside the span, the
    last row, and ``n_random`` seeded rows"""
    rows = {r for r in MARK_ROWS if r < n_rows} | {n_rows - 1}
    rows |= set(np.random.RandomState(seed).randint(0, n_rows, n_random).tolist())
    return np.array(sorted(rows), np.int64)


# ---- the four truncations the probes must expose (plain integers) ----------------------------------------------------------
TRUNCATIONS = ("u32_byte", "i32_byte", "u32_elem", "i32_elem")


def _wrap(v, signed):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if signed and v >= (1 << 31) else v


def truncated_element(row, col, how):
    """the element offset (from the arena's first float) a kernel would reach for cell (row, col) if it cut the row offset as
    ``how`` says; None where the cut byte offset is no whole element (never, at LD a multiple of 4 bytes)"""
    elem = row * LD + col
    if how.endswith("byte"):
        b = _wrap(4 * elem, how.startswith("i"))
        return b // 4 if b % 4 == 0 else None
    return _wrap(elem, how.startswith("i"))


def cell_of(elem):
    """(row, column) of an element offset inside the arena; None outside it (before the buffer)"""
    if elem is None or elem < 0:
        return None
    return divmod(elem, LD)


def may_be_initialised(cell, probes):
    """whether some case may have written the cell: a dense table's columns on any row, any table's columns on a probe row"""
    if cell is None:
        return False
    row, col = cell
    if col >= ARENA_COLS:
        return False
    dense = any(COL[t] <= col < COL[t] + TABLE_WIDTH for t in DENSE_TABLES)
    return dense or int(row) in set(int(r) for r in probes)


# ---- the monotone remap ----------------------------------------------------------------------------------------------------
class Remap:
    """ids of the big table <-> rows of the compact twin that holds ``kept`` (ascending, distinct) in that order"""

    def __init__(self, kept):
        self.kept = np.asarray(kept, np.int64)
        assert np.all(np.diff(self.kept) > 0)

    def __len__(self):
        return len(self.kept)

    def to_small(self, ids):
        ids = np.asarray(ids)
        j = np.searchsorted(self.kept, ids)
        assert np.all(j < len(self.kept)) and np.array_equal(self.kept[j], ids), "an id outside the kept rows"
        return j.astype(ids.dtype)

    def to_big(self, rows):
        rows = np.asarray(rows)
        return self.kept[rows].astype(rows.dtype)

    def triples(self, x, rel=None):
        """[n, 3] (s, p, o) with s, o through this remap and p through ``rel`` (a Remap; None: kept)"""
        x = np.asarray(x)
        out = x.copy()
        out[:, 0], out[:, 2] = self.to_small(x[:, 0]), self.to_small(x[:, 2])
        if rel is not None:
            out[:, 1] = rel.to_small(x[:, 1])
        return out

    def codes(self, codes):
        """corruption codes (bit 31 = the side, the rest the entity id) through the remap"""
        c = np.asarray(codes).astype(np.int64) & 0xFFFFFFFF
        return ((c & 0x80000000) | self.to_small(c & 0x7FFFFFFF)).astype(np.uint32).view(np.int32)


def stable_order(dest, n_rows):
    """(order, number valid): the grouping contract of csrc/emg_group.hip — ascending destination, equal destinations in
    ascending slot order, ids outside the table dropped"""
    dest = np.asarray(dest)
    valid = (dest >= 0) & (dest < n_rows)
    nv = int(valid.sum())
    return np.argsort(np.where(valid, dest, np.iinfo(np.int64).max).astype(np.int64), kind="stable")[:nv], nv


def segment_sums_f32(contrib, dest, order, block=64):
    """{destination: the float32 sum of its contributions in the order the apply adds them}.  ``block`` = 64: sequentially up
    to 64 rows, else 64-row blocks left to right and then the block sums left to right (the long-segment tree of
    csrc/emg_apply.hip; the reference of tests/test_hip_kernels.py::test_counting_grouping_edge_shapes).  ``block`` None: the
    whole segment sequentially (rows of at most 16 chunks: apply_rows_sub_kernel adds a segment in contribution order)."""
    out = {}
    if len(order) == 0:
        return out
    contrib = np.asarray(contrib, F32)
    k = contrib.shape[1]
    bounds = np.flatnonzero(np.diff(dest[order])) + 1
    starts = np.concatenate([[0], bounds])
    lens = np.diff(np.concatenate([starts, [len(order)]]))

    def run_sums(first, length):
        """float32 sums of the runs order[first[i] : first[i] + length[i]], each added left to right from +0 (all runs at once)"""
        acc = np.zeros((len(first), k), F32)
        for j in range(int(length.max())):
            live = np.flatnonzero(length > j)
            acc[live] = acc[live] + contrib[order[first[live] + j]]
        return acc

    if block is None:
        sums = run_sums(starts, lens)
    else:
        nblk = -(-lens // block)
        seg_of = np.repeat(np.arange(len(starts)), nblk)
        blk_in = np.arange(int(nblk.sum())) - np.repeat(np.cumsum(nblk) - nblk, nblk)
        first = starts[seg_of] + blk_in * block
        length = np.minimum(block, lens[seg_of] - blk_in * block)
        parts = run_sums(first, length)
        sums = np.zeros((len(starts), k), F32)
        head = np.cumsum(nblk) - nblk
        single = nblk == 1
        sums[single] = parts[head[single]]
        for s_ in np.flatnonzero(~single):         # (few: the segments longer than a block)
            g = np.zeros(k, F32)
            for p_ in parts[head[s_]:head[s_] + nblk[s_]]:
                g = g + p_
            sums[s_] = g
    for s_, st in enumerate(starts):
        out[int(dest[order[st]])] = sums[s_]
    return out


# ---- the grouping workspace's layout (csrc/emg_group.hip::layout_impl) in Python integers ----------------------------------
K_SCAN_TILE, K_LONG_SEGMENT, K_BUCKET_CHUNKS_MAX, K_BUCKET_MAX_NB = 4096, 64, 512, 4096
K_DENSE_HERE_MAX_ROWS = 131072
K_BUCKET_MIN_ROWS = 2 * K_DENSE_HERE_MAX_ROWS


def _al(x):
    return (x + 255) // 256 * 256


def _cdiv(a, b):
    return -(-a // b)


def counting_backend(N, R):
    """csrc/emg_group.hip::group_backend_counting with EMG_GROUPING unset"""
    return R <= 16 * N + (1 << 20)


def bucket_geometry(N, R):
    """csrc/emg_group.hip::bucket_geometry: (sh, nb, chunk_log) or None"""
    if N <= 0 or R <= 0:
        return None
    want = max(1, (1024 * R) // N)
    sh = 0
    while sh < 11 and (2 << sh) <= want:
        sh += 1
    while sh < 11 and _cdiv(R, 1 << sh) > K_BUCKET_MAX_NB:
        sh += 1
    nb = _cdiv(R, 1 << sh)
    cl = 10
    while cl < 30 and _cdiv(N, 1 << cl) > K_BUCKET_CHUNKS_MAX:
        cl += 1
    if nb > K_BUCKET_MAX_NB or cl > 16:
        return None
    return sh, nb, cl


def counting_layout(N, R):
    """byte offsets of the counting backend's workspace for N contributions on R rows (no long-segment scratch): a dict with
    'cnt', 'off', 'bmat' (None without a bucket geometry) and 'total' = what emg_apply_workspace_bytes returns"""
    assert counting_backend(N, R)
    kb = _al(4 * N)
    at = 6 * kb                                   # keys vals tmpv srcrow pos_of_slot coef
    at += _al(12 * (N // 2 + 1))                  # multi
    at += kb                                      # single
    at += _al(12 * (N // 8 + 2))                  # tasks
    at += _al(4 * (N // K_LONG_SEGMENT + 2))      # arrive
    at += _al(4 * 64)                             # counters
    at += _al(8 * _cdiv(R + 1, K_SCAN_TILE))      # status
    out = {"cnt": at}
    at += _al(4 * (R + 1))
    out["off"] = at
    at += _al(4 * (R + 1))
    geo = bucket_geometry(N, R)
    out["bmat"] = None
    if geo is not None:
        at += kb                                  # tmpv2
        out["bmat"] = at
        at += _al(4 * K_BUCKET_CHUNKS_MAX * (geo[1] + 1))
    out["total"] = at + 256
    return out


# ---- many-narrow -----------------------------------------------------------------------------------------------------------
NARROW_ROWS = (1 << 24) + (1 << 23) + 5
NARROW_K = 4
BUCKET_EDGE = 4096 * 2048            # the largest table with a bucket geometry; one row more has none


def narrow_marked(n_ent=NARROW_ROWS, n_random=40, seed=21):
    """ascending distinct ids: both sides of 2^23 and 2^24 (an odd id above 2^24 does not survive a trip through a float), the
    ends, and seeded ids of which half lie above 2^24 where the table reaches there"""
    ids = {0, n_ent - 1}
    ids |= {i for i in ((1 << 23) - 1, 1 << 23, (1 << 24) - 1, 1 << 24, (1 << 24) + 1) if i < n_ent}
    rs = np.random.RandomState(seed)
    ids |= set(rs.randint(0, n_ent, n_random // 2).tolist())
    if n_ent > (1 << 24) + 2:
        ids |= set((rs.randint((1 << 24) + 2, n_ent, n_random // 2) | 1).clip(max=n_ent - 1).tolist())
    return np.array(sorted(ids), np.int64)


def _narrow_hash(ids, cols, xp):
    """int64 [n, k] in [0, 2^16): column 0 the low 16 bits of the row, column 1 its bits from 16 up (so no two rows are equal),
    the other columns a multiplicative hash"""
    h = (ids * 2654435761 + cols * 40503 >> 5) & 0xFFFF
    h = xp.where(cols == 0, ids & 0xFFFF, h)
    return xp.where(cols == 1, ids >> 16, h)


def narrow_values_host(ids, k_int=NARROW_K):
    """the many-narrow table's rows ``ids`` on the host: a 16-bit integer function of (row, column) / 2^17 - 0.25, exact in
    float32"""
    ids = np.asarray(ids, np.int64)[:, None]
    h = _narrow_hash(ids, np.arange(k_int, dtype=np.int64)[None, :] + 0 * ids, np)
    return (h.astype(np.float64) / 131072.0 - 0.25).astype(F32)


def narrow_table(n_ent=NARROW_ROWS, k_int=NARROW_K):
    """the many-narrow table on the device, filled there in slices (temporaries of 2^22 rows)"""
    import torch
    t = torch.empty((n_ent, k_int), dtype=torch.float32, device="cuda")
    cols = torch.arange(k_int, dtype=torch.int64, device="cuda")[None, :]
    for r0 in range(0, n_ent, 1 << 22):
        r1 = min(n_ent, r0 + (1 << 22))
        ids = torch.arange(r0, r1, dtype=torch.int64, device="cuda")[:, None]
        h = _narrow_hash(ids, cols + 0 * ids, torch)
        t[r0:r1] = (h.to(torch.float64) / 131072.0 - 0.25).to(torch.float32)
    return t


# ---- the arena -------------------------------------------------------------------------------------------------------------
def choose_span(free_bytes):
    """the span a device with ``free_bytes`` free takes: the large one if twice its size is free, else the small one, else None"""
    for n in (SPAN_LARGE, SPAN_SMALL):
        if free_bytes >= 2 * arena_bytes(n):
            return n
    return None


class Arena:
    """the sparse-giant buffer; ``owned`` counts the cells the running case has written through ``write`` / ``own``"""

    def __init__(self, n_rows):
        self.n_rows = n_rows
        self.buf = None
        self.probes = probe_rows(n_rows)
        self.owned = 0
        self.reset()

    def reset(self):
        """all NaN, nothing owned (allocates the buffer if ``free`` has released it)"""
        import torch
        if self.buf is None:
            self.buf = torch.empty(arena_floats(self.n_rows), dtype=torch.float32, device="cuda")
        self.buf.fill_(float("nan"))
        self.owned = 0

    def free(self):
        import torch
        self.buf = None
        torch.cuda.empty_cache()

    def table(self, name, k_int):
        """the [n_rows, k_int] view at the table's column offset, row stride LD"""
        assert padded(k_int) <= TABLE_WIDTH
        return self.buf.as_strided((self.n_rows, k_int), (LD, 1), COL[name])

    def write(self, name, rows, values):
        """rows (ascending distinct ids, or None = every row) of table ``name`` <- values [n, k_int] (host), at alloc_table's
        padded width with the pad columns zero; returns the [n_rows, k_int] view"""
        import torch
        values = np.ascontiguousarray(values, dtype=F32)
        k_int = values.shape[1]
        kp = padded(k_int)
        full = np.zeros((values.shape[0], kp), F32)
        full[:, :k_int] = values
        wide = self.buf.as_strided((self.n_rows, kp), (LD, 1), COL[name])
        src = torch.from_numpy(full).cuda()
        if rows is None:
            assert values.shape[0] == self.n_rows
            wide.copy_(src)
        else:
            wide[torch.from_numpy(np.asarray(rows, np.int64)).cuda()] = src
        self.owned += full.size
        return self.table(name, k_int)

    def read(self, name, rows, k_int):
        """host copy of the padded rows (None = every row) of table ``name``"""
        import torch
        wide = self.buf.as_strided((self.n_rows, padded(k_int)), (LD, 1), COL[name])
        if rows is None:
            return wide.cpu().numpy()
        return wide[torch.from_numpy(np.asarray(rows, np.int64)).cuda()].cpu().numpy()

    def count_written(self):
        """the arena's non-NaN elements, counted in chunks of COUNT_CHUNK floats"""
        import torch
        total = torch.zeros((), dtype=torch.int64, device="cuda")
        n = self.buf.numel()
        for a in range(0, n, COUNT_CHUNK):
            c = self.buf[a:min(n, a + COUNT_CHUNK)]
            total += torch.count_nonzero(c == c)
        return int(total.item())

    def check_no_stray_write(self):
        """after a case: every written cell is one the case owns (and every owned cell still holds a number)"""
        got = self.count_written()
        assert got == self.owned, "the arena holds %d numbers, the case owns %d cells: a stray store" % (got, self.owned)


def compact(values):
    """the twin: an alloc_table table holding ``values`` [n, k_int]"""
    import torch
    from emgraph_amd.training import alloc_table
    values = np.ascontiguousarray(values, dtype=F32)
    return alloc_table(values.shape[0], values.shape[1], torch.device("cuda"), init=values)


def bits(t):
    """host uint32 / uint16 view of a device tensor or host array, for comparisons to the bit"""
    a = t.detach().cpu().contiguous() if hasattr(t, "detach") else None
    if a is not None:
        if a.element_size() == 2:
            import torch
            return a.view(torch.int16).numpy().view(np.uint16)
        a = a.numpy()
    else:
        a = np.ascontiguousarray(t)
    return a.view(np.uint32) if a.dtype.itemsize == 4 and a.dtype.kind == "f" else a
