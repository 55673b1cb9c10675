"""What rank_triples_device LAUNCHES, pinned (no GPU): every device wrapper it reaches is replaced, by name on
emgraph_amd.device, with a recording fake that returns CPU tensors of the right shape; torch.cuda.Event records an "event"
marker into the same trace.  The expected traces and the returned ``stats`` live in tests/golden/rank_call_traces.json, written
by THIS module run as a script (``python tests/test_rank_trace_host.py --record OUT``) at the commit before the host-side
refactor of the ranking driver: the recorder and the test are the same code.  A refactor that quietly sent a fast mode to the
exact kernel, moved an event pair or dropped a probe fails here; the ranks themselves are checked to the bit on the GPU."""
import inspect
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from emgraph_amd import _lib as L                        # noqa: E402
from emgraph_amd import device as D                      # noqa: E402
from emgraph_amd.evaluation import ranking as R          # noqa: E402
from emgraph_amd.type_constraints import TypeConstraints  # noqa: E402

GOLDEN_FILE = os.path.join(ROOT, "tests", "golden", "rank_call_traces.json")
K, N_REL, N_TEST, CHUNK = 40, 5, 200, 128


def _describe(v):
    if isinstance(v, torch.Tensor):
        return ["tensor", str(v.dtype).replace("torch.", ""), list(v.shape)]
    if v is None or isinstance(v, (bool, str)):
        return v
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return float(v)
    if isinstance(v, (tuple, list)):
        return [_describe(x) for x in v]
    return {"object": type(v).__name__}


class Fakes:
    """the recording fakes of one scenario; ``steer``: what the prefilter fakes do, call by call — ("pairs", n), ("frac", f) (f
    of the call's rows x candidates left undecided), ("overflow",), ("raise",); past the list: ``then``"""

    SIZE_HELPERS = ("prefilter_ld", "eval_prefilter_segments", "eval_sad_segments", "eval_prefilter_rotate_segments",
                    "prefilter_waves", "bf16_ld", "prefilter_max_cols", "link_order_w", "rescore_tiles_ws_bytes")

    def __init__(self, steer=(), then=("pairs", 3), rotate_refuses=False):
        self.trace, self.steer, self.then, self.n_prefilter, self.rotate_refuses = [], list(steer), then, 0, rotate_refuses

    def install(self, monkeypatch):
        for name in dir(self):
            if name.startswith("f_"):
                real, fake = getattr(D, name[2:]), getattr(self, name)
                monkeypatch.setattr(D, name[2:], fake if name[2:] in self.SIZE_HELPERS else self._recorded(name[2:], real, fake))
        trace = self.trace

        class Event:
            def __init__(self, enable_timing=False):
                pass

            def record(self):
                trace.append("event")

            def elapsed_time(self, other):
                return 0.0

        monkeypatch.setattr(torch.cuda, "Event", Event)
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)

    def _recorded(self, name, real, fake):
        sig = inspect.signature(real)   # every argument by name, defaults filled in: positional or keyword is the same call

        def call(*args, **kwargs):
            bound = sig.bind(*args, **kwargs)
            bound.apply_defaults()
            self.trace.append([name, {k: _describe(v) for k, v in bound.arguments.items()}])
            return fake(*args, **kwargs)
        return call

    # ---- size helpers: faked, not recorded (their call order may move) ----
    def f_prefilter_ld(self, k_cols):
        return ((k_cols + 31) // 32) * 32

    def f_eval_prefilter_segments(self, n_rows, n_cand, k_cols=400):
        return (n_rows + 31) // 32

    def f_eval_sad_segments(self, n_rows, n_cand):
        return (n_rows + 63) // 64

    def f_eval_prefilter_rotate_segments(self, n_rows, n_cand):
        return (n_rows + 127) // 128

    def f_prefilter_waves(self, k_cols):
        return 8

    def f_bf16_ld(self, k_int):
        return ((k_int + 63) // 64) * 64

    def f_prefilter_max_cols(self):
        return 512

    def f_link_order_w(self, link):
        return 0 if link == L.LINK_LINEAR else 64

    def f_rescore_tiles_ws_bytes(self, n_local):
        return 64

    # ---- queries, exact counts ----
    def f_eval_build_queries(self, model_id, ent, rel, k_int, scale, test_spo, side_mode, ldq=None, link=L.LINK_LINEAR):
        n_rows = (2 if side_mode >= L.EVAL_SPO else 1) * test_spo.shape[0]
        return torch.zeros((n_rows, ((k_int + 3) // 4) * 4)), torch.zeros(n_rows, dtype=torch.int32)

    def f_eval_count(self, model_id, Q, pos_int, ent, k_int, scale, cnt_gt, cnt_eq, **kw):
        cnt_gt.add_(1)   # (the counters tell in the ranks which kernels counted a tile, and whether a redone tile was zeroed)

    def f_eval_filter_count(self, *a, **kw):
        pass

    def f_eval_count_grouped(self, model_id, Q, pos_int, row_group, ent, k_int, scale, pool_ptr, pool_idx, cnt_gt, cnt_eq):
        cnt_gt.add_((row_group >= 0).to(torch.int32) * 4)

    def f_eval_count_lists(self, model_id, Q, pos_int, ent, k_int, scale, cand, cnt_gt, cnt_eq, **kw):
        cnt_gt.add_(8)

    def f_eval_draw_candidates(self, n_q, q_offset, side_mode, n_cand, n_ent, seed, device, ld_cand=None):
        return torch.zeros(((2 if side_mode >= L.EVAL_SPO else 1) * n_q, n_cand), dtype=torch.int32)

    # ---- bf16 mode ----
    def f_to_bf16(self, table, k_int, ld_dst=None):
        return torch.zeros((table.shape[0], ld_dst or ((k_int + 7) // 8) * 8), dtype=torch.bfloat16)

    def f_eval_pos_int_bf16(self, model_id, ent_bf16, k_int, scale, test_spo, side_mode, q_bf16):
        n = q_bf16.shape[0]
        return torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32)

    def f_eval_count_bf16(self, model_id, q_bf16, pos_int, self_ent, ent_bf16, k_int, scale, cnt_gt, cnt_eq, **kw):
        cnt_gt.add_(16)
        cnt_eq.add_(1)

    def f_eval_filter_count_bf16(self, *a, **kw):
        pass

    # ---- the prefilters ----
    def _prefilter(self, q, ent_tab, cnt_gt, pair_count):
        i, self.n_prefilter = self.n_prefilter, self.n_prefilter + 1
        what = self.steer[i] if i < len(self.steer) else self.then
        if what[0] == "raise":
            raise L.EmgError("shape outside the kernel (steered)")
        pair_count.zero_()
        if what[0] == "overflow":
            pair_count[-1] = 1
        else:
            pair_count[0] = what[1] if what[0] == "pairs" else int(math.ceil(what[1] * q.shape[0] * ent_tab.shape[0]))
        cnt_gt.add_(2)

    def f_eval_prefilter_f16(self, model_id, q_f16, pos_int, band, ent_f16, ent_offset, k_int, scale, cnt_gt, pairs, pair_count,
                             cnt_eq=None):
        self._prefilter(q_f16, ent_f16, cnt_gt, pair_count)

    def f_eval_prefilter_f16_thr(self, q_f16, thr, ent_f16, ent_offset, k_cols, cnt_gt, pairs, pair_count):
        self._prefilter(q_f16, ent_f16, cnt_gt, pair_count)

    def f_eval_prefilter_f16_thr4(self, q_f16, thr4, ent_f16, ent_offset, k_cols, cnt_gt, cnt_eq, pairs, pair_count):
        self._prefilter(q_f16, ent_f16, cnt_gt, pair_count)

    def f_eval_prefilter_sad(self, q_u16, thresholds, ent_u16, ent_offset, k_int, cnt_gt, pairs, pair_count):
        self._prefilter(q_u16, ent_u16, cnt_gt, pair_count)

    def f_eval_prefilter_rotate(self, q_f16, thresholds, ent_f16, ent_offset, k_int, cnt_gt, pairs, pair_count):
        self._prefilter(q_f16, ent_f16, cnt_gt, pair_count)

    def f_eval_rescore_pairs(self, *a, **kw):
        pass

    def f_eval_rescore_pairs_tiles(self, *a, **kw):
        pass

    # ---- what the prefilters read ----
    def f_to_f16(self, table, k_int, ld_dst=None):
        return torch.zeros((table.shape[0], ld_dst or ((k_int + 7) // 8) * 8), dtype=torch.float16)

    def f_to_f16_l2(self, src, k_int, is_query, ld_dst=None):
        rows = torch.zeros((src.shape[0], self.f_prefilter_ld(k_int + 2)), dtype=torch.float16)
        return (rows, torch.zeros_like(src)) if is_query else (rows, torch.zeros(1, dtype=torch.float64))

    def f_eval_prefilter_bounds(self, ent, ent_f16, k_int):
        return torch.zeros(3, dtype=torch.float64)

    def f_eval_prefilter_band(self, Q, Q_f16, k_int, bounds):
        return torch.zeros(Q.shape[0])

    def f_eval_link_thresholds(self, link, pos_int, band, scale, want_score=False):
        n = pos_int.numel()
        return torch.zeros(2 * n), torch.zeros(4 * n), None

    def f_eval_l2_thresholds(self, Q, pos_int, band, bounds4, k_int):
        return torch.zeros(2 * Q.shape[0])

    def f_eval_sad_range(self, ent, rel, k_int):
        return torch.ones(2, dtype=torch.float64)

    def f_eval_sad_quantize(self, src, k_int, rng):
        return torch.zeros((src.shape[0], ((k_int + 7) // 8) * 8), dtype=torch.int16)

    def f_eval_sad_thresholds(self, pos_int, k_int, rng):
        return torch.zeros((2, pos_int.numel()), dtype=torch.int32)

    def f_eval_rotate_image(self, src, k_int, scale=1.0, check=False, image=True):
        if check and self.rotate_refuses:
            return None
        stats = torch.tensor([1.0, 1.0, 0.0], dtype=torch.float64)
        if not image:
            return None, None, stats
        return torch.zeros((src.shape[0], ((k_int + 7) // 8) * 8), dtype=torch.float16), torch.zeros(src.shape[0]), stats

    def f_eval_rotate_thresholds(self, pos_int, rho_q, k_int, scale, q_stats, ent_stats):
        return torch.zeros((2, pos_int.numel()))


# ------------------------------------------------------------------------------------------------
# the scenarios
# ------------------------------------------------------------------------------------------------
def _inputs(n_ent, n_test=N_TEST):
    rng = np.random.RandomState(7)
    T = np.stack([rng.randint(0, 64, n_test), rng.randint(0, N_REL, n_test), rng.randint(0, 64, n_test)], 1)
    F = np.stack([rng.randint(0, 64, 300), rng.randint(0, N_REL, 300), rng.randint(0, 64, 300)], 1)
    return torch.zeros((n_ent, K)), torch.zeros((N_REL, K)), T, F


def _pools(relations):
    return TypeConstraints.from_pools({p: (np.arange(0, 40), np.arange(20, 64)) for p in relations}, (64, N_REL), from_idx=True)


def _lists(T):
    rng = np.random.RandomState(11)
    return {"s": rng.randint(0, 64, (len(T), 4)), "o": rng.randint(-1, 64, (len(T), 4))}


_TIES = [("frac", 0.05), ("frac", 0.001)]   # the probe leaves 5 % undecided, the ties probe 0.1 %

# name -> (model, n_ent, keyword arguments of the call ('filter' / 'tables' / 'tc' / 'lists' are resolved below), fakes' arguments,
#          environment, number of calls)
SCENARIOS = {
    "01_complex_exact_filter": (L.COMPLEX, 64, dict(precision=0, filter=True), {}, {}, 1),
    "02_complex_exact_subset": (L.COMPLEX, 64, dict(precision=0, filter=True, entities_subset=np.arange(3, 50)), {}, {}, 1),
    "03_complex_bf16_worst": (L.COMPLEX, 64, dict(precision=1, strategy="worst", filter=True), {}, {}, 1),
    "04_complex_bf16_middle": (L.COMPLEX, 64, dict(precision=1, strategy="middle"), {}, {}, 1),
    "05_complex_fast_tables_twice": (L.COMPLEX, 64, dict(precision=2, tables=R.PrefilterTables, filter=True), {}, {}, 2),
    "06_complex_fast_no_tables": (L.COMPLEX, 64, dict(precision=2), {}, {}, 1),
    "07_complex_fast_prove_ties": (L.COMPLEX, 64, dict(precision=2, tables=R.PrefilterTables), dict(steer=_TIES), {}, 1),
    "08_complex_fast_ties_off": (L.COMPLEX, 64, dict(precision=2, tables=R.PrefilterTables), dict(steer=_TIES[:1]),
                                 {"EMG_PREFILTER_TIES": "0"}, 1),
    "09_complex_fast_probe_off": (L.COMPLEX, 64, dict(precision=2, tables=R.PrefilterTables), {}, {"EMG_PREFILTER_PROBE": "0"}, 1),
    "10_complex_fast_second_chunk_uncovered": (L.COMPLEX, 64, dict(precision=2, tables=R.PrefilterTables, filter=True),
                                               dict(steer=[("pairs", 3), ("pairs", 3), ("raise",)]), {}, 1),
    "11_complex_fast_first_chunk_overflows": (L.COMPLEX, 64, dict(precision=2, tables=R.PrefilterTables, filter=True),
                                              dict(steer=[("pairs", 3), ("overflow",)]), {}, 1),
    "12_complex_fast_tanh": (L.COMPLEX, 64, dict(precision=2, tables=R.PrefilterTables, link=L.LINK_TANH, filter=True), {}, {}, 1),
    "13_complex_fast_tanh_prove_ties": (L.COMPLEX, 64, dict(precision=2, tables=R.PrefilterTables, link=L.LINK_TANH),
                                        dict(steer=_TIES), {}, 1),
    "14_transe_l1_fast_tables": (L.TRANSE_L1, 64, dict(precision=2, tables=R.SadTables, filter=True), {}, {}, 1),
    "15_transe_l1_fast_no_tables": (L.TRANSE_L1, 64, dict(precision=2), {}, {}, 1),
    "16_transe_l2_fast": (L.TRANSE_L2, 64, dict(precision=2, filter=True), {}, {}, 1),
    "17_transe_l2_fast_uncovered": (L.TRANSE_L2, 64, dict(precision=2, tables=R.L2Tables), dict(then=("raise",)), {}, 1),
    "18_rotate_auto": (L.ROTATE, 32768, dict(precision="auto", tables=R.RotateTables, filter=True), {}, {}, 2),
    "19_rotate_auto_range_refused": (L.ROTATE, 32768, dict(precision="auto"), dict(rotate_refuses=True), {}, 1),
    "20_rotate_auto_probe_above": (L.ROTATE, 32768, dict(precision="auto"), dict(steer=[("frac", 0.05)]), {}, 1),
    "21_transe_l1_fast_tanh_exact_only": (L.TRANSE_L1, 64, dict(precision=2, link=L.LINK_TANH), {}, {}, 1),
    "22_typed_every_row": (L.COMPLEX, 64, dict(precision="auto", tc=range(N_REL), filter=True), {}, {}, 1),
    "23_typed_no_row": (L.COMPLEX, 64, dict(precision=0, tc=()), {}, {}, 1),
    "24_typed_mixed": (L.COMPLEX, 64, dict(precision=2, tc=(0, 1), filter=True, corrupt_side="s+o"), {}, {}, 1),
    "25_lists_dict": (L.COMPLEX, 64, dict(precision=0, lists=True), {}, {}, 1),
    "26_lists_drawn_filter": (L.DISTMULT, 64, dict(precision="auto", candidates=8, candidates_seed=5, filter=True), {}, {}, 1),
    "27_complex_fast_side_s_128": (L.COMPLEX, 64, dict(precision=2, tables=R.PrefilterTables, corrupt_side="s", n_test=128), {}, {}, 1),
}


def run_scenario(name, monkeypatch):
    """{'trace': [...], 'calls': [{'stats', 'ranks_shape', 'ranks'} per call]} of one scenario under the fakes"""
    model_id, n_ent, kw, fake_kw, env, n_calls = SCENARIOS[name]
    kw = dict(kw)
    for var in ("EMG_PREFILTER_PROBE", "EMG_PREFILTER_TIES", "EMG_RESCORE", "EMG_PAIR_CAP", "EMG_PAIR_LOG2"):
        monkeypatch.delenv(var, raising=False)
    for var, value in env.items():
        monkeypatch.setenv(var, value)
    fakes = Fakes(**fake_kw)
    fakes.install(monkeypatch)
    ent, rel, T, F = _inputs(n_ent, kw.pop("n_test", N_TEST))
    if kw.pop("filter", False):
        kw["filter_triples"] = R.FilterIndex(F)
    if "tables" in kw:
        cls = kw.pop("tables")
        kw["ent_f16"] = cls(ent, K) if cls in (R.PrefilterTables, R.L2Tables) else cls(ent, rel, K)
    if "tc" in kw:
        kw["type_constraints"] = _pools(kw.pop("tc"))
    if kw.pop("lists", False):
        kw["candidates"] = _lists(T)
    calls = []
    for _ in range(n_calls):
        fakes.trace.append("call")
        stats = {}
        ranks = R.rank_triples_device(model_id, ent, rel, K, 1.0, T, query_chunk=CHUNK, stats=stats, **kw)
        stats.pop("count_ms")
        calls.append({"stats": {k: _describe(v) for k, v in sorted(stats.items())}, "ranks_dtype": str(ranks.dtype),
                      "ranks_shape": list(ranks.shape), "ranks": ranks.reshape(-1).tolist()})
    return {"trace": fakes.trace, "calls": calls}


def _as_json(result):
    return json.loads(json.dumps(result))


@pytest.fixture(scope="module")
def golden_traces():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


def test_golden_holds_every_scenario(golden_traces):
    assert sorted(golden_traces) == sorted(SCENARIOS)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_rank_call_trace(name, golden_traces, monkeypatch):
    got, want = _as_json(run_scenario(name, monkeypatch)), golden_traces[name]
    assert got["calls"] == want["calls"]
    for i, (g, w) in enumerate(zip(got["trace"], want["trace"])):
        assert g == w, "record %d of the trace differs" % i
    assert len(got["trace"]) == len(want["trace"])


def _record(path):
    out = {}
    for name in sorted(SCENARIOS):
        mp = pytest.MonkeyPatch()
        try:
            out[name] = _as_json(run_scenario(name, mp))
        finally:
            mp.undo()
    with open(path, "w") as f:
        f.write("{\n")
        for j, name in enumerate(sorted(out)):
            r = out[name]
            f.write(' "%s": {\n  "calls": %s,\n  "trace": [\n' % (name, json.dumps(r["calls"], separators=(",", ":"))))
            f.write(",\n".join("   " + json.dumps(rec, separators=(",", ":")) for rec in r["trace"]))
            f.write("\n  ]\n }%s\n" % ("," if j + 1 < len(out) else ""))
        f.write("}\n")
    print("wrote %d scenarios to %s" % (len(out), path))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--record":
        _record(sys.argv[2])
    else:
        sys.exit("usage: python tests/test_rank_trace_host.py --record OUT")
