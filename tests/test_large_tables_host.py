"""Host side of the large-table tests (no device): the inputs of tests/test_large_tables.py expose a truncated row offset, the
host-only size functions neither wrap nor shrink past 2^23 rows, and the helper's monotone remap keeps the grouping order."""
import numpy as np
import pytest

from tests import _large_tables as lt

SIZES = [lt.BUCKET_EDGE, lt.BUCKET_EDGE + 1, lt.NARROW_ROWS, (1 << 31) - 1]


# ---------------------------------------------------------------- the probe set detects truncation
def test_spans_cross_the_byte_marks_between_the_probed_rows():
    assert lt.LD * 4 == 2_097_168 and (lt.LD * 4) % 16 == 0
    for mark, (lo, hi) in {1 << 31: (1023, 1024), 1 << 32: (2047, 2048), 1 << 33: (4095, 4096), 1 << 34: (8191, 8192)}.items():
        assert 4 * (lo * lt.LD + lt.ARENA_COLS) <= mark <= 4 * hi * lt.LD, mark     # every table's row lo below, row hi at or past it
    assert lt.arena_bytes(lt.SPAN_LARGE) > (1 << 34) and (1 << 33) < lt.arena_bytes(lt.SPAN_SMALL) < (1 << 34)
    assert max(lt.COL.values()) + lt.TABLE_WIDTH <= lt.ARENA_COLS < lt.LD
    cols = sorted(lt.COL.values())
    assert all(b - a >= lt.TABLE_WIDTH for a, b in zip(cols, cols[1:]))           # disjoint column ranges
    for n in (lt.SPAN_LARGE, lt.SPAN_SMALL):
        p = lt.probe_rows(n)
        assert set(r for r in lt.MARK_ROWS if r < n) | {n - 1} <= set(p.tolist()) and np.all(np.diff(p) > 0) and p[-1] == n - 1


@pytest.mark.parametrize("table", sorted(lt.COL))
@pytest.mark.parametrize("how", lt.TRUNCATIONS)
@pytest.mark.parametrize("n_rows", [lt.SPAN_LARGE, lt.SPAN_SMALL])
def test_probe_rows_expose_a_truncated_row_offset(n_rows, how, table):
    """Plain integer arithmetic on the test's own inputs.  For each truncation of a row's offset (uint32 / int32 of the byte
    offset / of the element offset) some probe row of the span is reached at another address than its own.  Unsigned: that
    address lies inside the arena on a cell no case initialises (a read returns NaN, a store changes the count of written
    cells); signed: it differs, and where it is negative it lies before the buffer.  The 8.02 GiB span ends below element 2^32,
    so the uint32 cut of the ELEMENT offset changes nothing there: only the 16.02 GiB span shows that one."""
    probes = lt.probe_rows(n_rows)
    col = lt.COL[table]
    reaches = how != "u32_elem" or n_rows * lt.LD > (1 << 32)
    exposed = []
    for r in probes.tolist():
        true = r * lt.LD + col
        cut = lt.truncated_element(r, col, how)
        if cut == true:
            continue
        if how.startswith("u"):
            cell = lt.cell_of(cut)
            # the whole row of the table, not only its first cell, lands on cells nobody writes
            last = lt.cell_of(lt.truncated_element(r, col + lt.TABLE_WIDTH - 1, how))
            if not lt.may_be_initialised(cell, probes) and not lt.may_be_initialised(last, probes) and cut < lt.arena_floats(n_rows):
                exposed.append(r)
        else:
            exposed.append(r)
    assert bool(exposed) == reaches, (how, table, exposed)
    if not reaches:
        assert n_rows == lt.SPAN_SMALL and all(lt.truncated_element(r, col, how) == r * lt.LD + col for r in probes.tolist())


def test_span_choice_and_owned_cells():
    assert lt.choose_span(2 * lt.arena_bytes(lt.SPAN_LARGE)) == lt.SPAN_LARGE
    assert lt.choose_span(2 * lt.arena_bytes(lt.SPAN_LARGE) - 1) == lt.SPAN_SMALL
    assert lt.choose_span(2 * lt.arena_bytes(lt.SPAN_SMALL) - 1) is None
    assert lt.padded(1) == 4 and lt.padded(4) == 4 and lt.padded(50) == 52
    assert lt.COUNT_CHUNK * 4 <= 64 << 20


# ---------------------------------------------------------------- workspace sizing past 2^23 rows
def _lib():
    from emgraph_amd import device
    return device


def _size(fn, *args):
    """the entry's answer.  None of the sizes of this file is one an entry refuses (all are at most INT32_MAX rows, which the
    discovery entries accept too), so an error of any kind, a zero or a negative value — a size that wrapped — fails the test."""
    v = fn(*args)
    assert isinstance(v, int) and v > 0, (fn.__name__, args, v)
    return v


def test_bucket_geometry_edge_in_python_integers():
    """4096 buckets x 2048 rows = 8 388 608 rows is the last table with a bucket geometry (csrc/emg_group.hip::bucket_geometry)"""
    N = 22 * 70000
    assert lt.bucket_geometry(N, lt.BUCKET_EDGE) == (11, 4096, 12)
    assert lt.bucket_geometry(N, lt.BUCKET_EDGE + 1) is None
    assert lt.bucket_geometry(N, lt.NARROW_ROWS) is None
    assert lt.counting_backend(N, lt.BUCKET_EDGE) and lt.counting_backend(N, lt.BUCKET_EDGE + 1)
    assert not lt.counting_backend(700, lt.NARROW_ROWS) and lt.counting_backend(42 * 70000, lt.NARROW_ROWS)


@pytest.mark.parametrize("n_ent", SIZES)
def test_apply_workspace_bytes_is_the_layout_formula_without_a_32_bit_wrap(n_ent):
    """emg_apply_workspace_bytes in the counting backend (R <= 16 N + 2^20) against the same layout in Python integers: the
    bucket matrix is there up to 8 388 608 rows and gone one row later, so the size DROPS across the edge — and nothing else
    may.  (The sort backend's size comes from rocPRIM's query, which needs a device: tests/test_large_tables.py.)"""
    d = _lib()
    sizes = []
    for N in (1_540_000, 2_940_000, 140_000_000):
        if not lt.counting_backend(N, n_ent):
            continue
        want = lt.counting_layout(N, n_ent)
        got = _size(d.apply_workspace_bytes, N, n_ent)
        assert got == want["total"], (N, n_ent, got, want)
        assert got > 8 * n_ent                                     # cnt + off alone: no 32-bit wrap of 4 (R + 1)
        assert (want["bmat"] is not None) == (n_ent <= lt.BUCKET_EDGE and N <= 512 << 16)
        sizes.append(got)
        k = _size(d.apply_workspace_bytes, N, n_ent, 200)       # + the long-segment scratch: 2 (N / 64 + 2) rows of 200 floats
        assert k == got + 2 * (N // 64 + 2) * 200 * 4
    assert sizes and sizes == sorted(sizes)                        # monotone in the contributions


@pytest.mark.parametrize("n_ent", SIZES)
def test_train_step_workspace_bytes_grows_with_its_arguments(n_ent):
    d = _lib()
    prev = 0
    for B, eta in ((70000, 20), (70000, 40), (140000, 40)):
        if not lt.counting_backend((2 + eta) * B, n_ent):
            continue
        got = _size(d.train_step_workspace_bytes, B, eta, 4, n_ent, 7)
        assert got >= prev
        # it holds at least the entity grouping workspace and the contribution rows (4 floats wide here)
        assert got >= lt.counting_layout((2 + eta) * B, n_ent)["total"] + (2 + eta) * B * 16
        prev = got
    if prev:      # (2^31 - 1 rows: every batch here is grouped by the sort backend, whose size query needs a device)
        assert _size(d.train_step_workspace_bytes, 140000, 40, 200, n_ent, 7) > prev
    else:
        assert n_ent == (1 << 31) - 1


@pytest.mark.parametrize("n_ent", SIZES)
def test_evaluation_and_discovery_workspace_sizes_do_not_wrap(n_ent):
    """every host-only size function at n_ent rows.  No refusal is expected at any of these sizes.  Where the formula is one line
    of the source it is restated in Python integers and must be met exactly (emg_eval_rescore_tiles_ws_bytes: three words per
    32-row tile + 64 tiles + 256; emg_calib_ws_bytes: a 256-byte header + six doubles per four rows); the carved workspaces
    (top-N, grid, DBSCAN, k-means) must hold at least the bytes of their own per-row arrays — so no 32-bit wrap — and must not
    shrink when an argument grows."""
    d = _lib()
    smaller = SIZES[SIZES.index(n_ent) - 1] if SIZES.index(n_ent) else 1 << 20

    def grows(fn, args_small, args_big, floor):
        a, b = _size(fn, *args_small), _size(fn, *args_big)
        assert b >= floor, (fn.__name__, args_big, b, floor)
        assert a <= b, (fn.__name__, args_small, a, args_big, b)

    assert _size(d.rescore_tiles_ws_bytes, n_ent) == 12 * (-(-n_ent // 32) + 64) + 256
    assert _size(d.calib_ws_bytes, n_ent) == 256 + -(-n_ent // 4) * 48
    # emg_eval_topn: per row and per 4096-candidate chunk, top_n (id, score) pairs
    grows(d.eval_topn_ws_bytes, (8, smaller, 10), (8, n_ent, 10), 8 * (n_ent // 4096) * 8)
    grows(d.eval_topn_ws_bytes, (8, n_ent, 10), (16, n_ent, 10), 16 * (n_ent // 4096) * 8)
    grows(d.eval_topn_ws_bytes, (8, n_ent, 10), (8, n_ent, 100), 8 * (n_ent // 4096) * 8)
    # emg_eval_grid_count: query rows x thresholds
    grows(d.eval_grid_ws_bytes, (smaller, 16), (n_ent, 16), n_ent * 16 * 4)
    grows(d.eval_grid_ws_bytes, (n_ent, 16), (n_ent, 256), n_ent * 256 * 4)
    # emg_rows_dbscan: labels, parents and counts per row
    grows(d.rows_dbscan_ws_bytes, (smaller, 5), (n_ent, 5), n_ent * 12)
    grows(d.rows_dbscan_ws_bytes, (n_ent, 5), (n_ent, 50), n_ent * 12)
    # emg_rows_kmeans: a label and a distance per row
    grows(d.rows_kmeans_ws_bytes, (smaller, 8, 4), (n_ent, 8, 4), n_ent * 8)
    grows(d.rows_kmeans_ws_bytes, (n_ent, 8, 4), (n_ent, 64, 4), n_ent * 8)
    grows(d.rows_kmeans_ws_bytes, (n_ent, 8, 4), (n_ent, 8, 200), n_ent * 8)


def test_size_functions_refuse_what_they_document():
    """the refusals themselves: the entry's own error or its documented 0, nothing else"""
    from emgraph_amd import _lib as L
    d = _lib()
    with pytest.raises(ValueError, match="out of range"):
        d.rows_dbscan_ws_bytes((1 << 31), 5)                       # past INT32_MAX rows: the documented 0
    with pytest.raises(ValueError, match="out of range"):
        d.rows_kmeans_ws_bytes((1 << 31), 8, 4)
    with pytest.raises(L.EmgError, match="top_n"):
        d.eval_topn_ws_bytes(8, 1 << 20, 0)
    with pytest.raises(L.EmgError, match="n_thr"):
        d.eval_grid_ws_bytes(8, 257)
    with pytest.raises(ValueError, match="negative"):
        d.calib_ws_bytes(-1)


# ---------------------------------------------------------------- the helper's remap
def test_monotone_remap_keeps_the_stable_grouping_order_and_the_summation_order():
    rs = np.random.RandomState(12)
    kept = lt.narrow_marked()
    m = lt.Remap(kept)
    assert kept[0] == 0 and kept[-1] == lt.NARROW_ROWS - 1 and {(1 << 24) - 1, 1 << 24, (1 << 24) + 1} <= set(kept.tolist())
    assert np.any((kept > (1 << 24)) & (kept % 2 == 1))                     # odd ids above 2^24: lost in a float
    assert np.any(kept.astype(np.float32).astype(np.int64) != kept)
    dest = kept[rs.randint(0, len(kept), 5000)].astype(np.int32)
    dest[:300] = kept[-1]                                                   # a long segment: block tasks
    small = m.to_small(dest)
    np.testing.assert_array_equal(m.to_big(small), dest)
    o_big, nv = lt.stable_order(dest, lt.NARROW_ROWS)
    o_small, nv2 = lt.stable_order(small, len(kept))
    assert nv == nv2 == len(dest)
    np.testing.assert_array_equal(o_big, o_small)                           # same slots at the same sorted positions
    np.testing.assert_array_equal(np.flatnonzero(np.diff(dest[o_big])), np.flatnonzero(np.diff(small[o_small])))   # same segments
    contrib = rs.randn(len(dest), 4).astype(np.float32)
    a, b = lt.segment_sums_f32(contrib, dest, o_big), lt.segment_sums_f32(contrib, small, o_small)
    assert len(a) == len(b) == len(set(dest.tolist()))
    for big_id, g in a.items():
        np.testing.assert_array_equal(g.view(np.uint32), b[int(m.to_small(np.array([big_id]))[0])].view(np.uint32))
    # codes: the side bit survives, the id is remapped; triples: s and o remapped, p kept
    codes = (dest[:64].astype(np.int64) | (np.arange(64) % 2 << 31)).astype(np.uint32).view(np.int32)
    cs = m.codes(codes)
    np.testing.assert_array_equal(cs < 0, codes < 0)
    np.testing.assert_array_equal(cs & 0x7FFFFFFF, small[:64])
    x = np.stack([dest[:9], np.arange(9, dtype=np.int32), dest[9:18]], 1)
    xs = m.triples(x)
    np.testing.assert_array_equal(xs[:, 1], x[:, 1])
    np.testing.assert_array_equal(kept[xs[:, 0]], x[:, 0])
    with pytest.raises(AssertionError):
        m.to_small(np.array([3 if 3 not in kept else 5]))


def test_narrow_values_are_exact_and_differ_between_neighbouring_marked_rows():
    ids = lt.narrow_marked()
    v = lt.narrow_values_host(ids)
    assert v.dtype == np.float32 and v.shape == (len(ids), lt.NARROW_K) and np.all(np.abs(v) <= 0.25)
    assert len({tuple(r) for r in v.tolist()}) == len(ids)                  # a read of a neighbouring row would show
