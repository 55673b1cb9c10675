"""The exact re-scoring kernels of the exact-fast mode (csrc/emg_rank.hip) on pair lists made by hand (tests/_rescore_ref.py), every
form: rescore_pairs_kernel scalar and staged-vector, rescore_segment_kernel with 8 and 4 waves, staged and unstaged, the tile form
(tile_sort_kernel, tile_scan_kernel, rescore_tile_kernel with 8 and 4 waves), the three chain kinds, with and without a score link.
Every comparison is == on int32 counters against the host's explicit-fmaf chain; tests/test_rescore_host.py shows that the cases
hold the segment sizes, spans, wraps, duplicates and ties they are meant to.

Shapes: 130 query rows (four 32-row blocks, a part, the sentinel), 200 entities (a last 32-row tile of 8), 27 segments of capacity
1600.  k_int 4 (one 16-byte piece: the refill's clamp), 20 (less than a 32-float slice), 32 (one slice), 36 (a slice and a tail), 64
(the two slices in flight), 68 (one past them), 200 (the workload), 576 (the first width of the 4-wave image: long segments from 256
pairs), 864 (no image fits: the per-pair kernel takes all); 37, 36 with stride 39 and 36 on rows 4 bytes past a 16-byte boundary for
the scalar form.  Counters start at 7 and 3 between guard words; the sentinel row's counters must not move."""
import numpy as np
import pytest

from tests import _rescore_ref as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 64
GT0, EQ0 = 7, 3


def _libs():
    from emgraph_amd import _lib as L
    from emgraph_amd import device as D
    D.require_gpu()
    return L, D


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_table(host, ld_extra=0, skew=0, lead_rows=0):
    """a [n, k] table on the device as a view into a larger NaN-filled buffer: row stride k + ld_extra, `skew` floats past a
    16-byte boundary, `lead_rows` rows of the buffer in front of it (a slab of a larger table)"""
    n, k = host.shape
    ld = k + ld_extra
    buf = torch.full(((lead_rows + n) * ld + 8,), float("nan"), dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[skew:skew + (lead_rows + n) * ld].view(lead_rows + n, ld)[lead_rows:, :k]
    t.copy_(torch.from_numpy(host))
    assert t.stride() == (ld, 1) and t.data_ptr() % 16 == (4 * (skew + lead_rows * ld)) % 16
    return t


class Counters:
    """cnt_gt / cnt_eq of n rows, pre-filled with 7 and 3, between guard words"""

    def __init__(self, n):
        self.n = n
        self.bufs = [torch.full((n + 2 * GUARD,), -77, dtype=torch.int32, device="cuda") for _ in range(2)]
        self.gt, self.eq = (b[GUARD:GUARD + n] for b in self.bufs)
        self.gt.fill_(GT0)
        self.eq.fill_(EQ0)

    def added(self):
        """(gt, eq) added so far, int64, after checking the guards"""
        out = []
        for b, base in zip(self.bufs, (GT0, EQ0)):
            h = b.cpu().numpy()
            assert (h[:GUARD] == -77).all() and (h[GUARD + self.n:] == -77).all(), "written outside the counters"
            out.append(h[GUARD:GUARD + self.n].astype(np.int64) - base)
        return out

    def untouched(self):
        gt, eq = self.added()
        return not gt.any() and not eq.any()


class DevCase:
    """a case's buffers on the device"""

    def __init__(self, case, ldq_extra=0, lde_extra=0, q_skew=0, e_skew=0, lead_rows=0):
        self.case = case
        self.Q = dev_table(case.Q, ldq_extra, q_skew)
        self.E = dev_table(case.E, lde_extra, e_skew, lead_rows)
        self.pos = cu(case.pos_int)
        self.pairs = cu(case.pairs.reshape(-1))
        self.pcount = cu(case.pair_count)

    def raw(self, cnt):
        """the leading arguments every entry point shares after (model[, link]), and the trailing ones"""
        c = self.case
        head = (self.Q.data_ptr(), self.Q.stride(0), self.pos.data_ptr(), self.E.data_ptr(), self.E.stride(0), c.ent_offset)
        mid = (c.k_int, c.scale, self.pairs.data_ptr(), self.pairs.numel(), self.pcount.data_ptr(), c.n_seg)
        return head, mid, (cnt.gt.data_ptr(), cnt.eq.data_ptr())


def _stream(D):
    return D._stream()


def rescore(L, D, dc, entry, spb=4, rps=0, link=0, cnt=None):
    """one call of a segment entry point on fresh (or the given) counters"""
    c, lib = dc.case, L.load()
    cnt = cnt or Counters(c.n_rows)
    head, mid, tail = dc.raw(cnt)
    if entry == "rows":
        D.eval_rescore_pairs(c.model, dc.Q, dc.pos, dc.E, c.ent_offset, c.k_int, c.scale, dc.pairs, dc.pcount, c.n_seg, cnt.gt, cnt.eq,
                             spb, rps, link=link)
    elif entry == "pairs":
        L.check(lib.emg_eval_rescore_pairs(c.model, *head, *mid, *tail, _stream(D)), "emg_eval_rescore_pairs")
    elif entry == "ex":
        L.check(lib.emg_eval_rescore_pairs_ex(c.model, *head, *mid, spb, *tail, _stream(D)), "emg_eval_rescore_pairs_ex")
    else:
        L.check(lib.emg_eval_rescore_pairs_link(c.model, link, *head, *mid, spb, rps, *tail, _stream(D)), "emg_eval_rescore_pairs_link")
    return cnt


def tiles(D, dc, cnt=None, sorted_pairs=None, ws=None):
    c = dc.case
    cnt = cnt or Counters(c.n_rows)
    if sorted_pairs is None:
        sorted_pairs = torch.empty(dc.pairs.numel(), dtype=torch.int64, device="cuda")
    if ws is None:
        ws = torch.zeros(D.rescore_tiles_ws_bytes(dc.E.shape[0]), dtype=torch.uint8, device="cuda")
    assert sorted_pairs.numel() == dc.pairs.numel()
    D.eval_rescore_pairs_tiles(c.model, dc.Q, dc.pos, dc.E, c.ent_offset, c.k_int, c.scale, dc.pairs, dc.pcount, c.n_seg, sorted_pairs, ws,
                               cnt.gt, cnt.eq)
    return cnt, ws


def same(cnt, want, case, what, times=1):
    gt, eq = cnt.added()
    assert gt[case.sentinel] == 0 and eq[case.sentinel] == 0, (what, "an entry behind a segment's count was read")
    for name, got, exp in (("gt", gt, want[0]), ("eq", eq, want[1])):
        bad = np.flatnonzero(got != times * exp)
        assert len(bad) == 0, (what, name, "rows", bad[:8], "got", got[bad[:8]], "want", times * exp[bad[:8]])


# (ldq - k_int, ld_ent - k_int, ent_offset, rows of the buffer in front of the slab)
LAYOUTS = ((0, 0, 0, 0), (12, 12, 1000, 3), (12, 0, 1000, 0), (0, 12, 0, 5))
# (entry point, segments_per_block, rows_per_segment)
CALLS = (("rows", 4, 0), ("rows", 4, 32), ("rows", 8, 0), ("rows", 8, 32), ("rows", 64, 32), ("pairs", 4, 0), ("ex", 4, 0), ("ex", 8, 32),
         ("link", 8, 0), ("link", 8, 32))


# ---- 1. the segment forms against the host chain ----------------------------------------------------------------------------------
@pytest.mark.parametrize("k_int", ref.WIDTHS)
@pytest.mark.parametrize("model_name", sorted(ref.MODELS))
def test_segment_forms_equal_the_host_chain(model_name, k_int):
    """the four entry points, segments_per_block 4 / 8 / 64, rows_per_segment 0 (everything through the per-pair kernel) and 32 (long
    segments through the LDS form), both row strides, an offset slab: the counters of the host chain, and so of each other"""
    L, D = _libs()
    base = ref.segment_case(model_name, k_int)
    want = ref.expected(base)
    n = 0
    for ldq_x, lde_x, off, lead in LAYOUTS:
        dc = DevCase(ref.with_offset(base, off), ldq_x, lde_x, lead_rows=lead)
        for entry, spb, rps in CALLS:
            same(rescore(L, D, dc, entry, spb, rps), want, base, (entry, spb, rps, ldq_x, lde_x, off))
            n += 1
    print("%s k_int=%d: %d calls, %d pairs in %d segments, %d added to gt, %d to eq" % (
        model_name, k_int, n, sum(len(s[0]) for s in ref.counted(base)), base.n_seg, want[0].sum(), want[1].sum()))


@pytest.mark.parametrize("k_int,ld,skew", ref.SCALAR_SHAPES)
@pytest.mark.parametrize("model_name", sorted(ref.MODELS))
def test_scalar_forms_equal_the_host_chain(model_name, k_int, ld, skew):
    """rows the 16-byte loads cannot read — a width or a stride that is no multiple of 4, a table that starts 4 bytes past a 16-byte
    boundary (the query rows, the slab, both) — take the scalar per-pair kernel whatever rows_per_segment says"""
    L, D = _libs()
    base = ref.segment_case(model_name, k_int)
    want = ref.expected(base)
    n = 0
    for q_skew, e_skew in (((skew, 0), (0, skew), (skew, skew)) if skew else ((0, 0),)):
        dc = DevCase(ref.with_offset(base, 1000), ld - k_int, ld - k_int, q_skew, e_skew)
        for entry, spb, rps in CALLS:
            same(rescore(L, D, dc, entry, spb, rps), want, base, (entry, spb, rps, q_skew, e_skew))
            n += 1
    print("%s k_int=%d ld=%d skew=%d: %d calls equal the host chain" % (model_name, k_int, ld, skew, n))


# ---- 2. a second call accumulates -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_int", (36, 576, 864))
@pytest.mark.parametrize("model_name", sorted(ref.MODELS))
def test_second_call_adds_the_same_again(model_name, k_int):
    L, D = _libs()
    base = ref.segment_case(model_name, k_int)
    want = ref.expected(base)
    dc = DevCase(base)
    for rps in (0, 32):
        cnt = rescore(L, D, dc, "rows", 8, rps)
        same(rescore(L, D, dc, "rows", 8, rps, cnt=cnt), want, base, ("twice", rps), times=2)
    print("%s k_int=%d: two calls add twice %d / %d" % (model_name, k_int, want[0].sum(), want[1].sum()))


# ---- 3. the linked forms ------------------------------------------------------------------------------------------------------------------
def filter_count(L, D, dc, link):
    """what the exact linked kernel (tests/test_link_ranking.py) adds for the same pairs given as its per-row CSR"""
    c = dc.case
    ptr, idx = ref.as_csr(c)
    cnt = Counters(c.n_rows)
    D.eval_filter_count(c.model, dc.Q, dc.pos, dc.E, c.ent_offset, c.k_int, c.scale, cu(ptr), cu(idx), cnt.gt, cnt.eq, link=link)
    return cnt.added()


@pytest.mark.parametrize("link", ref.LINKS[1:])
@pytest.mark.parametrize("k_int", ref.LINK_WIDTHS)
@pytest.mark.parametrize("model_name", ref.LINK_MODELS)
def test_linked_forms_equal_the_linked_filter_count(model_name, k_int, link):
    """tanh, sigmoid, softplus: the host cannot name libm's bits, so the counters must be emg_eval_filter_count_link's on the same pairs;
    under the linear link the same cross-check must also agree with the host chain.  Tables at a scale where the link saturates for
    part of every row's candidates, positives compared through the link: linked ties"""
    L, D = _libs()
    lk = L.LINK_IDS[link]
    base = ref.SimpleNamespace(**vars(ref.segment_case(model_name, k_int, link)))
    # the positives through the DEVICE's link: phi(raw score of the row's true entity) from emg_link_scores, whose bits link_cmp_int shares
    phi, dummy = cu(base.true_score), torch.zeros(base.n_rows, dtype=torch.float32, device="cuda")
    D.link_scores(lk, None, 1.0, phi, dummy, base.n_rows, 1)
    base.pos_int = ref.cmp_int(phi.cpu().numpy())
    base.pos_int[base.sentinel] = np.iinfo(np.int32).min
    tied = 0
    for (ldq_x, lde_x, off, lead) in LAYOUTS[:2]:
        dc = DevCase(ref.with_offset(base, off), ldq_x, lde_x, lead_rows=lead)
        want = filter_count(L, D, dc, lk)
        assert (want[1] > 0).sum() >= 5 and want[0].sum() > 0
        tied = int((want[1] > 0).sum())
        for entry, spb, rps in (("rows", 8, 0), ("rows", 8, 32), ("rows", 4, 32), ("link", 8, 32), ("link", 64, 0)):
            same(rescore(L, D, dc, entry, spb, rps, link=lk), want, base, (link, entry, spb, rps, off))
        lin = ref.expected(base)
        flin = filter_count(L, D, dc, L.LINK_LINEAR)
        assert np.array_equal(flin[0], lin[0]) and np.array_equal(flin[1], lin[1])
        for rps in (0, 32):
            same(rescore(L, D, dc, "link", 8, rps, link=L.LINK_LINEAR), lin, base, ("linear", rps, off))
    print("%s k_int=%d %s: rows with linked ties %d, added %d / %d" % (model_name, k_int, link, tied, want[0].sum(), want[1].sum()))


# ---- 4. the tile form -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_int", ref.TILE_WIDTHS)
@pytest.mark.parametrize("model_name", sorted(ref.MODELS))
def test_tile_form_equals_the_host_chain(model_name, k_int):
    """8-wave and 4-wave tile kernels, a last tile of 8 entity rows; the workspace zeroed once: a second call on it adds the same again,
    the scan having returned the tile counts to zero"""
    L, D = _libs()
    base = ref.segment_case(model_name, k_int)
    want = ref.expected(base)
    for ldq_x, lde_x, off, lead in LAYOUTS[:2]:
        dc = DevCase(ref.with_offset(base, off), ldq_x, lde_x, lead_rows=lead)
        cnt, ws = tiles(D, dc)
        same(cnt, want, base, ("tiles", off))
        n_tiles = -(-base.E.shape[0] // 32)
        assert not ws[:4 * n_tiles].any(), "tile counts left behind"
        cnt, ws = tiles(D, dc, cnt=cnt, ws=ws)
        same(cnt, want, base, ("tiles twice", off), times=2)
        assert not ws[:4 * n_tiles].any()
    print("%s k_int=%d: tile form equals the host chain, %d / %d" % (model_name, k_int, want[0].sum(), want[1].sum()))


def test_tile_form_refuses_what_it_cannot_hold():
    """k_int 864 (no 32-row image fits LDS) and a table 4 bytes past a 16-byte boundary: EMG_ENOSUP, nothing written"""
    L, D = _libs()
    for k_int, ld, skew in ((864, 864, 0), (36, 48, 1), (36, 39, 0)):
        dc = DevCase(ref.segment_case("DistMult", k_int), ld - k_int, ld - k_int, 0, skew)
        cnt = Counters(dc.case.n_rows)
        sorted_pairs = torch.full((dc.pairs.numel(),), -1, dtype=torch.int64, device="cuda")
        ws = torch.zeros(D.rescore_tiles_ws_bytes(dc.E.shape[0]), dtype=torch.uint8, device="cuda")
        with pytest.raises(L.EmgError, match=r"code %d\)" % L.ENOSUP):
            tiles(D, dc, cnt, sorted_pairs, ws)
        assert cnt.untouched() and not ws.any() and bool((sorted_pairs == -1).all())
    print("tile form: EMG_ENOSUP at k_int 864, on a skewed table and on stride 39")


def test_tile_form_past_8192_tiles():
    """262184 entities at k_int 4 (a 4 MB table): pairs in tiles 0, 8191, 8192 and the last, partial one — the second trip of
    tile_scan_kernel's loop and its carry"""
    L, D = _libs()
    base = ref.big_tile_case()
    want = ref.expected(base)
    dc = DevCase(base)
    cnt, ws = tiles(D, dc)
    same(cnt, want, base, "big tiles")
    n_tiles = -(-ref.BIG_N_LOCAL // 32)
    assert not ws[:4 * n_tiles].any()
    same(rescore(L, D, dc, "rows", 8, 32), want, base, "big rows")
    print("tile form at %d tiles: %d pairs, added %d / %d" % (n_tiles, sum(len(s[0]) for s in ref.counted(base)), want[0].sum(), want[1].sum()))


# ---- 5. refusals write nothing ------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    L, D = _libs()
    lib = L.load()
    dc = DevCase(ref.segment_case("DistMult", 36))
    c = dc.case
    cnt = Counters(c.n_rows)
    sorted_pairs = torch.full((dc.pairs.numel(),), -1, dtype=torch.int64, device="cuda")
    ws_bytes = D.rescore_tiles_ws_bytes(dc.E.shape[0])
    assert ws_bytes == int(lib.emg_eval_rescore_tiles_ws_bytes(c.E.shape[0])) and ws_bytes >= 3 * 4 * 7
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
    head, mid, tail = dc.raw(cnt)
    st = _stream(D)

    def link_args(model=c.model, link=0, spb=8, rps=32, cap=None, n_seg=c.n_seg, null=None):
        a = [model, link, *head, *mid, spb, rps, *tail, st]
        if cap is not None:
            a[11] = cap
        a[13] = n_seg
        if null is not None:
            a[null] = None
        return a

    def tile_args(model=c.model, cap=None, n_seg=c.n_seg, scap=None, wsb=ws_bytes, null=None):
        a = [model, *head, c.E.shape[0], *mid, sorted_pairs.data_ptr(), sorted_pairs.numel() if scap is None else scap, ws.data_ptr(), wsb,
             *tail, st]
        if cap is not None:
            a[11] = cap
        a[13] = n_seg
        if null is not None:
            a[null] = None
        return a

    assert link_args()[11] == dc.pairs.numel() and tile_args()[11] == dc.pairs.numel()
    refused = []

    def refuse(what, rc):
        torch.cuda.synchronize()
        assert rc == -1, (what, rc)     # EMG_EINVAL
        assert cnt.untouched() and not ws.any() and bool((sorted_pairs == -1).all()), what
        refused.append(what)

    for model in (L.TRANSE_P, 7, -1, 99):
        refuse(("link model", model), lib.emg_eval_rescore_pairs_link(*link_args(model=model)))
        refuse(("rows model", model), lib.emg_eval_rescore_pairs_rows(*[a for i, a in enumerate(link_args(model=model)) if i != 1]))
    for model in (L.TRANSE_P, L.ROTATE, 7, -1):
        refuse(("tiles model", model), lib.emg_eval_rescore_pairs_tiles(*tile_args(model=model)))
    for link in (4, -1):
        refuse(("link", link), lib.emg_eval_rescore_pairs_link(*link_args(link=link)))
    for spb in (0, 6, 68):
        refuse(("spb", spb), lib.emg_eval_rescore_pairs_link(*link_args(spb=spb)))
        refuse(("ex spb", spb), lib.emg_eval_rescore_pairs_ex(c.model, *head, *mid, spb, *tail, st))
    refuse("capacity", lib.emg_eval_rescore_pairs_link(*link_args(cap=c.n_seg - 1)))
    refuse("tiles capacity", lib.emg_eval_rescore_pairs_tiles(*tile_args(cap=c.n_seg - 1)))
    refuse("sorted capacity", lib.emg_eval_rescore_pairs_tiles(*tile_args(scap=dc.pairs.numel() - 1)))
    refuse("workspace one byte short", lib.emg_eval_rescore_pairs_tiles(*tile_args(wsb=ws_bytes - 1)))
    for i in (2, 4, 5, 10, 12, 16, 17):           # Q, pos_int, ent, pairs, pair_count, cnt_gt, cnt_eq
        refuse(("link null", i), lib.emg_eval_rescore_pairs_link(*link_args(null=i)))
    for i in (1, 3, 4, 10, 12, 14, 16, 18, 19):   # Q, pos_int, ent, pairs, pair_count, sorted, tile_ws, cnt_gt, cnt_eq
        refuse(("tiles null", i), lib.emg_eval_rescore_pairs_tiles(*tile_args(null=i)))
    # no segments: fine, and nothing is launched
    assert lib.emg_eval_rescore_pairs_link(*link_args(n_seg=0)) == 0
    assert lib.emg_eval_rescore_pairs_tiles(*tile_args(n_seg=0)) == 0
    assert lib.emg_eval_rescore_pairs(c.model, *head, *mid[:5], 0, *tail, st) == 0
    torch.cuda.synchronize()
    assert cnt.untouched() and not ws.any() and bool((sorted_pairs == -1).all())
    # and the same arguments, unrefused, count
    L.check(lib.emg_eval_rescore_pairs_link(*link_args()), "emg_eval_rescore_pairs_link")
    same(cnt, ref.expected(c), c, "after the refusals")
    print("%d refused calls wrote nothing" % len(refused))


# ---- 6. agreement with the emitting path ---------------------------------------------------------------------------------------------------
def test_forms_agree_on_the_prefilters_own_pairs():
    """ComplEx k = 100 against 7000 entities, 150 triples, both sides: the pairs emg_eval_prefilter_f16 emits, re-scored by the per-pair
    kernel, the LDS segment form and the tile form — one set of counters, the host chain's on those pairs"""
    L, D = _libs()
    from emgraph_amd.evaluation import ranking as RK
    k, n_ent, nq = 100, 7000, 150
    ki = 2 * k
    rs = np.random.RandomState(11)
    E, R = (rs.randn(n_ent, ki) * 0.2).astype(np.float32), (rs.randn(4, ki) * 0.2).astype(np.float32)
    T = np.stack([rs.randint(0, n_ent, nq), rs.randint(0, 4, nq), rs.randint(0, n_ent, nq)], 1).astype(np.int32)
    Et = cu(E)
    Q, pos = D.eval_build_queries(L.COMPLEX, Et, cu(R), ki, 1.0, cu(T), L.EVAL_S_O)
    n_rows = Q.shape[0]
    ldh = D.prefilter_ld(ki)
    Eh, Qh = D.to_f16(Et, ki, ld_dst=ldh), D.to_f16(Q, ki, ld_dst=ldh)
    band = RK.prefilter_band(Q, Qh, ki, RK.table_norm_bounds(Et, Eh, ki))
    n_seg = D.eval_prefilter_segments(n_rows, n_ent, ki)
    cap = 2048
    pairs = torch.zeros(n_seg * cap, dtype=torch.int64, device="cuda")      # (row 0, entity 0) behind the counts: in range
    pcount = torch.zeros(n_seg + 1, dtype=torch.int32, device="cuda")
    decided = torch.zeros(n_rows, dtype=torch.int32, device="cuda")
    D.eval_prefilter_f16(L.COMPLEX, Qh, pos, band, Eh, 0, ki, 1.0, decided, pairs, pcount)
    pc = pcount.cpu().numpy()
    assert pc[n_seg] == 0 and pc[:n_seg].max() <= cap and pc[:n_seg].sum() > 0
    case = ref.SimpleNamespace(model=L.COMPLEX, k_int=ki, scale=1.0, link="linear", E=E, Q=np.ascontiguousarray(Q.cpu().numpy()[:, :ki]),
                               pos_int=pos.cpu().numpy(), pairs=pairs.cpu().numpy().reshape(n_seg, cap), pair_count=pc, ent_offset=0,
                               cap=cap, n_seg=n_seg, n_rows=n_rows, sentinel=None)
    want = ref.expected(case)
    waves = D.prefilter_waves(ki)
    got = []
    for rps in (0, 32):
        cnt = Counters(n_rows)
        D.eval_rescore_pairs(L.COMPLEX, Q, pos, Et, 0, ki, 1.0, pairs, pcount, n_seg, cnt.gt, cnt.eq, waves, rps)
        got.append(cnt.added())
    cnt = Counters(n_rows)
    D.eval_rescore_pairs_tiles(L.COMPLEX, Q, pos, Et, 0, ki, 1.0, pairs, pcount, n_seg, torch.empty_like(pairs),
                               torch.zeros(D.rescore_tiles_ws_bytes(n_ent), dtype=torch.uint8, device="cuda"), cnt.gt, cnt.eq)
    got.append(cnt.added())
    for g in got:
        assert np.array_equal(g[0], want[0]) and np.array_equal(g[1], want[1])
        assert np.array_equal(g[0], got[0][0]) and np.array_equal(g[1], got[0][1])
    print("ComplEx k=100, %d rows x %d entities: %d segments, %d pairs, %d segments reached 512 pairs (largest %d); added %d / %d" % (
        n_rows, n_ent, n_seg, pc[:n_seg].sum(), (pc[:n_seg] >= 512).sum(), pc[:n_seg].max(), want[0].sum(), want[1].sum()))
