"""Negative sampling on the device — Bernoulli side choice and filtered negatives (include/emgraph_hip.h, emg_sampler_bind;
csrc/emg_sampler.hpp) — against the host reference sampler (tests/_negsample_ref.py), to the bit: the three producers of
corruption ids (emg_corrupt_codes_sampled, emg_prepare_batch in its counting and its bucket form), the unbound library against
emg_corrupt_codes, and fit() end to end (every step's negatives, the step updates against the oracle with
tests/_fit_steps.py's bars, the three counts).  Graph A: 97 entities, 3 relations, 898 triples with a saturated (s, p);
B = 300 (no multiple of 256), eta = 3, three batches of which the last is short.  tests/test_negative_sampling_host.py shows, on
the CPU, that the reference itself redraws and leaves known rows on this graph.

Graph B (tests/_negsample_ref.py::graph_b; from test_graph_b_standalone_producer_equals_the_reference on): 1024, 1025, 2049, 5403 and
60001 known triples over the lowest and highest ids of a table of 262149 rows — the bind's shift is 0, 1, 2, 3 and 6, so past
1024 keys the membership test leaves the coarse index in LDS and bisects the run behind its entry in global memory
(csrc/emg_sampler.hpp, sampler_known), the last run short (at 1025: one key), with keys on both sides of 2^32; the corner
bindings of one known key and of the pool's extreme combinations; a fit() on a dense 60-entity graph of 5403 triples (shift 3).
ref.check_not_vacuous states on the reference's side of every comparison what test_negative_sampling_host.py shows on the CPU."""
import os

import numpy as np
import pytest
import torch

from oracle import emgraph_oracle as orc
from tests import _fit_steps as fs
from tests import _negsample_ref as ref

pytestmark = pytest.mark.gpu

B, ETA, SEED, COUNTER0 = 300, 3, 11, 6
BIG_ENT = 262144 + 5           # an entity table just tall enough for the bucket form of emg_prepare_batch
SETTINGS = [("uniform", False, 4), ("bernoulli", False, 4), ("uniform", True, 1), ("uniform", True, 4), ("bernoulli", True, 1),
            ("bernoulli", True, 4)]
SIDE_LISTS = [["s,o"], ["s+o"], ["s", "o"]]
POOLS = ["all", "list", "batch"]


def dev():
    from emgraph_amd import device as d
    d.require_gpu()
    return d


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def graph():
    X = ref.graph_a()
    return dict(X=X, known=ref.known_set(X), thr=ref.keep_thresholds(X, ref.N_REL))


class Bound:
    """a sampler bound for the duration of a ``with`` block; .stats() reads the three counts"""

    def __init__(self, d, graph, side, flt, retries, n_ent=None, known=True):
        from emgraph_amd import negative_sampling as NS
        n_ent = graph.get("n_ent", ref.N_ENT) if n_ent is None else n_ent
        self.d = d
        self.thr = cu(graph["thr"].view(np.int32)) if side == "bernoulli" else None
        self.keys = cu(NS.known_triple_keys(graph["X"], n_ent, ref.N_REL)) if (flt and known) else None
        self.st = torch.zeros(3, dtype=torch.int64, device="cuda")
        self.args = (n_ent, ref.N_REL)
        self.retries = retries

    def __enter__(self):
        self.d.sampler_bind(*self.args, keep_thr=self.thr, known_keys=self.keys, retries=self.retries, stats=self.st)
        return self

    def __exit__(self, *exc):
        self.d.sampler_unbind()

    def stats(self):
        torch.cuda.synchronize()
        r = self.st.cpu().numpy()
        self.st.zero_()
        return {"rows": int(r[0]), "redrawn": int(r[1]), "known_left": int(r[2])}


def pool_of(kind, xb):
    """(n_choices, entities_list or None) of a corruption pool for the batch xb"""
    if kind == "all":
        return None, None
    if kind == "list":
        return None, np.array([e for e in range(ref.N_ENT) if e % 3 != 1], np.int32)[::-1].copy()   # (not the identity, not sorted)
    return None, orc.batch_unique_entities(xb)


def prepare(d, pos, sides, n_ent, n_choices, elist, grouping=None, eta=None):
    """emg_prepare_batch on the batch: codes, destination arrays and the sorted keys of the entity grouping"""
    from emgraph_amd import _lib as L
    eta = ETA if eta is None else eta
    et = eta * len(sides)
    n_ce = (2 + et) * len(pos)
    codes = torch.full((len(pos) * et,), -7, dtype=torch.int32, device="cuda")
    de = torch.full((n_ce,), -7, dtype=torch.int32, device="cuda")
    dr = torch.full((len(pos),), -7, dtype=torch.int32, device="cuda")
    we = torch.zeros(d.apply_workspace_bytes(n_ce, n_ent), dtype=torch.uint8, device="cuda")
    wr = torch.zeros(d.apply_workspace_bytes(len(pos), ref.N_REL), dtype=torch.uint8, device="cuda")
    if grouping:
        os.environ["EMG_GROUPING"] = grouping
    try:
        d.prepare_batch(cu(pos.astype(np.int32)), eta, [L.SIDE_IDS[s] for s in sides], n_choices, codes, de, dr, n_ent, ref.N_REL, we, wr,
                        entities_list=cu(elist) if elist is not None else None, seed=SEED, counter0=COUNTER0)
        torch.cuda.synchronize()
    finally:
        os.environ.pop("EMG_GROUPING", None)
    # the last row of the bucket form's chunk x bucket offset matrix (512 words in front of the workspace's final 256 bytes,
    # csrc/emg_group.hip::layout_impl): the contributions of every chunk — written by bucket_ids_kernel, by no other form
    tail = we[-2304:-256].cpu().numpy().view(np.uint32)
    return codes.cpu().numpy(), de.cpu().numpy(), dr.cpu().numpy(), we[:4 * n_ce].cpu().numpy().view(np.uint32), tail


def check_prepared(got, want_codes, pos, what, bucket=None):
    codes, de, dr, keys, tail = got
    if bucket is not None:          # the form that ran: the bucket form leaves its chunks' counts, the counting form nothing there
        assert int(tail.sum()) == (len(de) if bucket else 0), (what, "bucket form" if bucket else "counting form", int(tail.sum()))
    n = len(pos)
    np.testing.assert_array_equal(codes, want_codes, err_msg=what)
    np.testing.assert_array_equal(de[:n], pos[:, 0], err_msg=what)
    np.testing.assert_array_equal(de[n:2 * n], pos[:, 2], err_msg=what)
    np.testing.assert_array_equal(de[2 * n:], want_codes & 0x7FFFFFFF, err_msg=what)      # dest_ent agrees with the codes
    np.testing.assert_array_equal(dr, pos[:, 1], err_msg=what)
    np.testing.assert_array_equal(keys, np.sort(de).astype(np.uint32), err_msg=what)      # and the grouping with dest_ent


@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("sides", SIDE_LISTS, ids=lambda s: "|".join(s))
def test_producers_equal_the_reference(graph, sides, pool):
    from emgraph_amd import _lib as L
    d = dev()
    xb = graph["X"][:B]
    pos_t = cu(xb.astype(np.int32))
    _, elist = pool_of(pool, xb)
    elist_t = cu(elist) if elist is not None else None
    for side, flt, T in SETTINGS:
        what = str((sides, pool, side, flt, T))
        kt, known = (graph["thr"] if side == "bernoulli" else None), (graph["known"] if flt else None)
        for n_ent, grouping in ((ref.N_ENT, None), (BIG_ENT, None)):
            n_choices = len(elist) if elist is not None else n_ent
            if n_ent == BIG_ENT and pool == "all" and not flt:
                continue            # (the tall table with the whole table as pool: covered once, by the settings with a filter)
            want = ref.sample_batch(xb, ETA, sides, SEED, COUNTER0, n_choices, elist, kt, known, T)
            with Bound(d, graph, side, flt, T, n_ent=n_ent) as b:
                if n_ent == ref.N_ENT:
                    for sd, s in enumerate(sides):      # the stand-alone producer, one call per side
                        got = d.corrupt_codes_sampled(pos_t, ETA, L.SIDE_IDS[s], n_choices, entities_list=elist_t, seed=SEED,
                                                      counter=COUNTER0 + sd)
                        np.testing.assert_array_equal(got.cpu().numpy(), want["parts"][sd]["codes"], err_msg=what)
                        neg = d.corrupt_expand(pos_t, ETA, got).cpu().numpy()
                        np.testing.assert_array_equal(neg, want["parts"][sd]["neg"], err_msg=what)
                    assert b.stats() == want["stats"], what
                # emg_prepare_batch: the counting form on the small table, the bucket form on the tall one
                check_prepared(prepare(d, xb, sides, n_ent, n_choices, elist, grouping="bucket" if n_ent == BIG_ENT else None),
                               want["codes"], xb, what + " prepare %d" % n_ent, bucket=n_ent == BIG_ENT)
                assert b.stats() == want["stats"], what
                if n_ent == BIG_ENT:    # the same tall table through the counting form: the two forms agree with the sampler bound
                    check_prepared(prepare(d, xb, sides, n_ent, n_choices, elist, grouping="count"), want["codes"], xb, what + " count",
                                   bucket=False)
                    assert b.stats() == want["stats"], what
    assert not d.sampler_bound()


def test_bucket_form_with_wide_chunks_equals_the_reference(graph):
    """more than 512 chunks of 1024 contribution slots (here 594 000 slots: chunks of 2048) take the bucket id kernel's other
    instantiation: its codes equal the counting form's on the same batch, and the reference's on a sample of the rows"""
    d = dev()
    rs = np.random.RandomState(77)
    Bw, eta, sides = 27000, 10, ["s", "s,o"]
    xb = graph["X"][rs.randint(0, len(graph["X"]), Bw)]
    _, elist = pool_of("list", xb)
    with Bound(d, graph, "bernoulli", True, 2, n_ent=BIG_ENT) as b:
        got = prepare(d, xb, sides, BIG_ENT, len(elist), elist, grouping="bucket", eta=eta)
        st = b.stats()
        cnt = prepare(d, xb, sides, BIG_ENT, len(elist), elist, grouping="count", eta=eta)
        assert b.stats() == st and st["rows"] == Bw * eta * 2 and st["redrawn"] > 1000 and st["known_left"] > 10
    assert (2 + 2 * eta) * Bw > 512 * 1024
    check_prepared(got, cnt[0], xb, "wide chunks, bucket form", bucket=True)
    check_prepared(cnt, got[0], xb, "wide chunks, counting form", bucket=False)
    rows = np.sort(rs.choice(Bw * eta, 3000, replace=False))
    for sd, s in enumerate(sides):
        want = ref.sample_side(xb, eta, s, SEED, COUNTER0 + sd, len(elist), elist, graph["thr"], graph["known"], 2, rows=rows)
        np.testing.assert_array_equal(got[0][sd * Bw * eta + rows], want["codes"], err_msg=s)
        assert (want["attempt"] > 0).sum() > 10


def test_unbound_and_empty_sampler_equal_the_plain_draw(graph):
    from emgraph_amd import _lib as L
    d = dev()
    xb = graph["X"][:B]
    pos_t = cu(xb.astype(np.int32))
    assert not d.sampler_bound()
    for sides in SIDE_LISTS:
        plain = [d.corrupt_codes(B, ETA, L.SIDE_IDS[s], ref.N_ENT, "cuda", seed=SEED, counter=COUNTER0 + i).cpu().numpy()
                 for i, s in enumerate(sides)]
        for i, s in enumerate(sides):
            got = d.corrupt_codes_sampled(pos_t, ETA, L.SIDE_IDS[s], ref.N_ENT, seed=SEED, counter=COUNTER0 + i)
            np.testing.assert_array_equal(got.cpu().numpy(), plain[i])
        unbound = prepare(d, xb, sides, ref.N_ENT, ref.N_ENT, None)
        np.testing.assert_array_equal(unbound[0], np.concatenate(plain))
        assert int(unbound[4].sum()) == 0          # (the small table: the counting form)
        # a sampler with no known triple and the uniform side: the same codes through the sampled kernels
        with Bound(d, graph, "uniform", True, 4, known=False) as b:
            for i, s in enumerate(sides):
                got = d.corrupt_codes_sampled(pos_t, ETA, L.SIDE_IDS[s], ref.N_ENT, seed=SEED, counter=COUNTER0 + i)
                np.testing.assert_array_equal(got.cpu().numpy(), plain[i])
            assert b.stats() == {"rows": B * ETA * len(sides), "redrawn": 0, "known_left": 0}
            bound = prepare(d, xb, sides, ref.N_ENT, ref.N_ENT, None)
            for a, c in zip(unbound, bound):
                np.testing.assert_array_equal(a, c)
        # injected draws bypass the sampler
        with Bound(d, graph, "bernoulli", True, 4):
            inj_r = cu((np.arange(B * ETA) % ref.N_ENT).astype(np.int32))
            inj_m = cu((np.arange(B * ETA) % 2).astype(np.int32))
            a = d.corrupt_codes(B, ETA, L.SIDE_IDS[sides[0]], ref.N_ENT, "cuda", inj_mask=inj_m, inj_repl=inj_r).cpu().numpy()
            c = d.corrupt_codes_sampled(pos_t, ETA, L.SIDE_IDS[sides[0]], ref.N_ENT, inj_mask=inj_m, inj_repl=inj_r).cpu().numpy()
            np.testing.assert_array_equal(a, c)


def test_protocol_keywords_agree_with_the_reference(graph):
    from emgraph_amd.evaluation.protocol import generate_corruptions_for_fit
    dev()
    xb = graph["X"][300:598]
    want = ref.sample_side(xb, ETA, "s,o", SEED, 4, ref.N_ENT, None, graph["thr"], graph["known"], 4)
    got = generate_corruptions_for_fit(xb, eta=ETA, corrupt_side="s,o", entities_size=ref.N_ENT, rnd=SEED, draw_counter=4,
                                       side_thresholds=graph["thr"], known_triples=graph["X"], retries=4)
    np.testing.assert_array_equal(got, want["neg"])
    plain = generate_corruptions_for_fit(xb, eta=ETA, corrupt_side="s,o", entities_size=ref.N_ENT, rnd=SEED, draw_counter=4)
    np.testing.assert_array_equal(plain, orc.generate_corruptions_for_fit_philox(xb, eta=ETA, corrupt_side="s,o", entities_size=ref.N_ENT,
                                                                                 seed=SEED, counter=4))


# ---- fit() end to end ----------------------------------------------------------------------------------------------------------
def fit_cfg(graph, name, loss, opt, emp_extra, seed=3, epochs=2):
    """a configuration in tests/_fit_steps.py's form: k = 8, eta = 3, three batches (on Graph A: 300, 300, 298)"""
    X = graph["X"]
    n_ent = graph.get("n_ent", ref.N_ENT)
    rs = np.random.RandomState(50 + seed)
    k = 8
    ent0 = (rs.randn(n_ent, k) * 0.3).astype(np.float32)
    rel0 = (rs.randn(ref.N_REL, k) * 0.3).astype(np.float32)
    emp = {"corrupt_side": "s,o"}
    if name == "TransE":
        emp["norm"] = 1
    emp.update(emp_extra)
    lr = 0.05
    kw = dict(k=k, eta=ETA, epochs=epochs, batches_count=3, seed=seed, loss=loss, optimizer=opt, optimizer_params={"lr": lr},
              embedding_model_params=emp, initializer="constant", initializer_params={"entity": ent0, "relation": rel0})
    return dict(seed=seed, name=name, norm=1, k=k, eta=ETA, loss=loss, opt=opt, sides=("s,o",), n_ent=n_ent, n_rel=ref.N_REL,
                n=len(X), bc=3, epochs=epochs, lr=lr, X=X, ent0=ent0, rel0=rel0, emp=emp, reg=None, reg_kw={}, kw=kw,
                omodel="TransE_L1" if name == "TransE" else name, what=str((name, loss, opt, emp_extra)))


BOTH = {"negative_side_sampling": "bernoulli", "filter_negatives": True}


@pytest.mark.parametrize("name,loss,opt", [("DistMult", "pairwise", "sgd"), ("TransE", "nll", "adam")])
def test_fit_steps_pass_the_oracle_with_the_sampled_negatives(graph, monkeypatch, name, loss, opt):
    """check_step_by_step with the oracle's negatives replaced by the reference sampler's: every step's update and loss inside
    the same intervals as for the plain draw; the recorded path and the default path give the same bits; the three counts"""
    dev()
    cfg = fit_cfg(graph, name, loss, opt, BOTH)

    def sampled(xb, entities_list=None, eta=1, corrupt_side="s,o", entities_size=0, seed=0, counter=0):
        return ref.sample_side(xb, eta, corrupt_side, seed, counter, entities_size, None, graph["thr"], graph["known"], 4)["neg"]

    monkeypatch.setattr(orc, "generate_corruptions_for_fit_philox", sampled)
    out = fs.check_step_by_step(cfg, monkeypatch)
    assert out["steps"] == 6 and not out["diverged"]
    m, err = fs._fit(cfg)
    assert err is None
    _, tot = ref.fit_reference(cfg["X"], ETA, ["s,o"], cfg["seed"], 3, 2, ref.N_ENT, None, graph["thr"], graph["known"], 4)
    assert m.negative_sampling_stats == tot and tot["redrawn"] >= 400 and tot["known_left"] >= 10


def record_negatives(monkeypatch):
    """Trainer.run_batches as tests/_fit_steps.py::record_steps patches it, one step() per batch without look-ahead (the step then
    prepares into the plan's first slot), keeping every step's codes and positives"""
    from emgraph_amd.training import Trainer
    rec = []

    def run_batches(self, specs):
        for s in [s for s in specs if s is not None and s[1] > 0]:
            self.step(s[0], s[1], epoch=s[2], batch=s[3], n_choices=s[4] if len(s) > 4 else None, entities_list=s[5] if len(s) > 5 else None)
            torch.cuda.synchronize()
            rec.append((tuple(int(v) for v in s[:4]), self.slots[0]["codes"][:s[1] * self.eta_total].cpu().numpy().copy()))

    monkeypatch.setattr(Trainer, "run_batches", run_batches)
    return rec


@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("setting", [("bernoulli", True, 4), ("uniform", True, 1), ("bernoulli", False, 4)], ids=str)
def test_fit_trains_on_the_reference_negatives(graph, monkeypatch, setting, pool):
    """every step's codes are the reference sampler's — so no negative is a known triple except the rows the reference counts as
    left —, the counts are the reference's, a fit on the default path gives the recorded fit's bits, and so does a second one"""
    dev()
    side, flt, T = setting
    extra = {"negative_side_sampling": side, "filter_negatives": flt, "filter_negatives_retries": T, "corrupt_side": ["s", "o"]}
    plist = None
    if pool == "list":
        plist = [e for e in range(ref.N_ENT) if e % 3 != 1]
        extra["negative_corruption_entities"] = plist
    elif pool == "batch":
        extra["negative_corruption_entities"] = "batch"
    cfg = fit_cfg(graph, "DistMult", "pairwise", "sgd", extra)
    cfg["sides"] = ("s", "o")
    with monkeypatch.context() as mp:
        rec = record_negatives(mp)
        m1, err = fs._fit(cfg)
    assert err is None
    ref_pool = orc.batch_unique_entities if pool == "batch" else (np.array(plist, np.int32) if plist else None)
    steps, tot = ref.fit_reference(cfg["X"], ETA, ["s", "o"], cfg["seed"], 3, 2, len(plist) if plist else ref.N_ENT, ref_pool,
                                   graph["thr"] if side == "bernoulli" else None, graph["known"] if flt else None, T)
    assert len(rec) == len(steps) == 6
    left = 0
    for (spec, codes), (epoch, batch, start, Bn, sb) in zip(rec, steps):
        assert spec == (start, Bn, epoch, batch)
        np.testing.assert_array_equal(codes, sb["codes"], err_msg=str(spec))
        xb = cfg["X"][start:start + Bn]
        rows = np.arange(len(codes)) % Bn
        keep, repl = codes < 0, codes & 0x7FFFFFFF
        neg = np.stack([np.where(keep, xb[rows, 0], repl), xb[rows, 1], np.where(keep, repl, xb[rows, 2])], 1)
        inside = np.array([tuple(r) in graph["known"] for r in neg.tolist()])
        if flt:
            np.testing.assert_array_equal(inside, np.concatenate([p["left"] for p in sb["parts"]]), err_msg=str(spec))
        left += int(inside.sum())
    assert m1.negative_sampling_stats == tot
    assert not flt or left == tot["known_left"]
    for _ in range(2):              # the default path, twice
        m2, err2 = fs._fit(cfg)
        assert err2 is None and m2.negative_sampling_stats == tot
        np.testing.assert_array_equal(m1.trained_model_params[0], m2.trained_model_params[0])
        np.testing.assert_array_equal(m1.trained_model_params[1], m2.trained_model_params[1])
        assert m1.epoch_losses == m2.epoch_losses


def test_default_keys_change_nothing_and_bad_ones_are_refused(graph):
    dev()
    base = fit_cfg(graph, "DistMult", "pairwise", "sgd", {})
    dflt = fit_cfg(graph, "DistMult", "pairwise", "sgd", {"negative_side_sampling": "uniform", "filter_negatives": False,
                                                          "filter_negatives_retries": 4})
    filt = fit_cfg(graph, "DistMult", "pairwise", "sgd", {"filter_negatives": True})
    ma, mb, mc = fs._fit(base)[0], fs._fit(dflt)[0], fs._fit(filt)[0]
    np.testing.assert_array_equal(ma.trained_model_params[0], mb.trained_model_params[0])
    np.testing.assert_array_equal(ma.trained_model_params[1], mb.trained_model_params[1])
    assert ma.epoch_losses == mb.epoch_losses
    rows = 2 * 898 * ETA
    assert ma.negative_sampling_stats == mb.negative_sampling_stats == {"rows": rows, "redrawn": 0, "known_left": 0}
    assert mc.negative_sampling_stats["rows"] == rows and mc.negative_sampling_stats["redrawn"] > 0
    assert not np.array_equal(ma.trained_model_params[0], mc.trained_model_params[0])      # the filter is not ignored
    from emgraph_amd import models
    for extra, exc in (({"negative_side_sampling": "bern"}, ValueError), ({"filter_negatives_retries": 0}, ValueError),
                       ({"filter_negatives": True, "sharding": "batch"}, NotImplementedError),
                       ({"negative_side_sampling": "uniform", "sharding": "k"}, NotImplementedError)):
        cfg = fit_cfg(graph, "DistMult", "pairwise", "sgd", extra)
        with pytest.raises(exc):
            getattr(models, cfg["name"])(**cfg["kw"]).fit(cfg["X"])
    from emgraph_amd import device as d
    assert not d.sampler_bound()


# ---- Graph B: the filter's second level (shift >= 1) and keys past 2^32 ------------------------------------------------------------
def standalone(d, g, sides, bern, T, what):
    """the stand-alone producer over the case ``g`` against the reference, codes, negatives and counts; returns the reference"""
    from emgraph_amd import _lib as L
    pool, n = g["pool"], len(g["pool"])
    want = ref.sample_batch(g["xb"], ETA, sides, SEED, COUNTER0, n, pool, g["thr"] if bern else None, g["known"], T)
    pos_t, pool_t = cu(g["xb"].astype(np.int32)), cu(pool)
    with Bound(d, g, "bernoulli" if bern else "uniform", True, T) as b:
        for sd, s in enumerate(sides):
            got = d.corrupt_codes_sampled(pos_t, ETA, L.SIDE_IDS[s], n, entities_list=pool_t, seed=SEED, counter=COUNTER0 + sd)
            np.testing.assert_array_equal(got.cpu().numpy(), want["parts"][sd]["codes"], err_msg=what)
            np.testing.assert_array_equal(d.corrupt_expand(pos_t, ETA, got).cpu().numpy(), want["parts"][sd]["neg"], err_msg=what)
        assert b.stats() == want["stats"], what
    return want


@pytest.mark.parametrize("n_known,n_ids", ref.SIZES_B)
def test_graph_b_standalone_producer_equals_the_reference(n_known, n_ids):
    d = dev()
    g = ref.case_b(n_known, n_ids)
    for sides in (["s,o"], ["s", "o"]):
        for bern in (False, True):
            for T in (1, 4):
                what = str((n_known, sides, bern, T))
                ref.check_not_vacuous(g, standalone(d, g, sides, bern, T, what), T)
    assert not d.sampler_bound()


@pytest.mark.parametrize("n_known,n_ids", [c for c in ref.SIZES_B if c[0] in (1025, 5403, 60001)])
def test_graph_b_prepare_batch_in_both_forms_equals_the_reference(n_known, n_ids):
    d = dev()
    g = ref.case_b(n_known, n_ids)
    xb, pool = g["xb"], g["pool"]
    for sides in (["s,o"], ["s", "o"]):
        for bern, T in ((True, 4), (False, 1)):
            what = str((n_known, sides, bern, T))
            want = ref.sample_batch(xb, ETA, sides, SEED, COUNTER0, n_ids, pool, g["thr"] if bern else None, g["known"], T)
            ref.check_not_vacuous(g, want, T)
            with Bound(d, g, "bernoulli" if bern else "uniform", True, T) as b:
                bucket = prepare(d, xb, sides, ref.N_ENT_B, n_ids, pool, grouping="bucket")
                check_prepared(bucket, want["codes"], xb, what + " bucket", bucket=True)
                assert b.stats() == want["stats"], what
                count = prepare(d, xb, sides, ref.N_ENT_B, n_ids, pool, grouping="count")
                check_prepared(count, want["codes"], xb, what + " count", bucket=False)
                assert b.stats() == want["stats"], what
                check_prepared(count, bucket[0], xb, what + " count against bucket", bucket=False)
    assert not d.sampler_bound()


def test_graph_b_bucket_form_with_wide_chunks_equals_the_reference():
    """test_bucket_form_with_wide_chunks_equals_the_reference with the 60001 keys of Graph B bound (shift 6)"""
    d = dev()
    g = ref.case_b(60001, 200)
    rs = np.random.RandomState(77)
    Bw, eta, sides, pool = 27000, 10, ["s", "s,o"], g["pool"]
    xb = g["X"][rs.randint(0, len(g["X"]), Bw)]
    with Bound(d, g, "bernoulli", True, 2) as b:
        got = prepare(d, xb, sides, ref.N_ENT_B, len(pool), pool, grouping="bucket", eta=eta)
        st = b.stats()
        cnt = prepare(d, xb, sides, ref.N_ENT_B, len(pool), pool, grouping="count", eta=eta)
        assert b.stats() == st and st["rows"] == Bw * eta * 2 and st["redrawn"] > 1000 and st["known_left"] > 10
    assert (2 + 2 * eta) * Bw > 512 * 1024
    check_prepared(got, cnt[0], xb, "wide chunks, bucket form", bucket=True)
    check_prepared(cnt, got[0], xb, "wide chunks, counting form", bucket=False)
    rows = np.sort(rs.choice(Bw * eta, 3000, replace=False))
    parts = []
    for sd, s in enumerate(sides):
        want = ref.sample_side(xb, eta, s, SEED, COUNTER0 + sd, len(pool), pool, g["thr"], g["known"], 2, rows=rows)
        np.testing.assert_array_equal(got[0][sd * Bw * eta + rows], want["codes"], err_msg=s)
        assert (want["attempt"] > 0).sum() >= 150 and want["left"].sum() > 0
        parts.append(want)
    assert all(v > 0 for v in ref.examined_counts(parts, ref.N_ENT_B, ref.N_REL).values())


@pytest.mark.parametrize("name", ["one_low", "one_high", "absent", "present"])
def test_graph_b_corner_bindings_equal_the_reference(name):
    """one known key — the smallest ('one_low') / the largest ('one_high') a candidate of the pool can have: a search hits entry
    0, passes it, or falls off the low end —, and 2049 keys without / 2051 keys with the pool's two extreme combinations"""
    d = dev()
    g = ref.corner_cases_b()[name]
    kmin, kmax = (f(ref.triple_keys(g["X"], ref.N_ENT_B, ref.N_REL)) for f in (min, max))
    for sides in (["s,o"], ["s", "o"]):
        for bern in (False, True):
            for T in (1, 4):
                what = str((name, sides, bern, T))
                want = standalone(d, g, sides, bern, T, what)
                ex = np.concatenate([p["examined"] for p in want["parts"]])
                keys = np.array(ref.triple_keys(ex, ref.N_ENT_B, ref.N_REL))
                assert name in ("one_low", "present") or (keys < kmin).any(), what
                assert name in ("one_high", "present") or (keys > kmax).any(), what
                for t in (g["lo"], g["hi"]):        # both extreme combinations are looked up, with the answer the set gives
                    hit = np.all(ex[:, :3] == np.array(t), 1)
                    assert hit.any() and np.all(ex[hit, 3] == (t in g["known"])), what
                assert want["stats"]["redrawn"] > 0, what
    assert not d.sampler_bound()


def test_graph_b_fit_trains_on_the_reference_negatives_and_passes_the_oracle(monkeypatch):
    """fit() on the dense graph of 60 entities and 5403 known triples (shift 3), Bernoulli side and filter: every step's codes
    and the three counts are the reference's, every step's update passes tests/_fit_steps.py's bars with the reference's
    negatives, and the recorded path gives the default path's bits"""
    dev()
    X = ref.graph_fit_b()
    g = dict(X=X, known=ref.known_set(X), thr=ref.keep_thresholds(X, ref.N_REL), n_ent=60)
    assert ref.coarse_index(len(g["known"]))[0] == 3
    cfg = fit_cfg(g, "DistMult", "pairwise", "sgd", BOTH)
    steps, tot = ref.fit_reference(X, ETA, ["s,o"], cfg["seed"], 3, 2, 60, None, g["thr"], g["known"], 4)
    attempt = np.concatenate([p["attempt"] for s in steps for p in s[4]["parts"]])
    assert 20 * tot["redrawn"] >= tot["rows"] and tot["known_left"] > 0 and set(attempt.tolist()) == set(range(5))
    with monkeypatch.context() as mp:
        rec = record_negatives(mp)
        m1, err = fs._fit(cfg)
    assert err is None and len(rec) == len(steps) == 6
    for (spec, codes), (epoch, batch, start, Bn, sb) in zip(rec, steps):
        assert spec == (start, Bn, epoch, batch)
        np.testing.assert_array_equal(codes, sb["codes"], err_msg=str(spec))
    assert m1.negative_sampling_stats == tot

    def sampled(xb, entities_list=None, eta=1, corrupt_side="s,o", entities_size=0, seed=0, counter=0):
        return ref.sample_side(xb, eta, corrupt_side, seed, counter, entities_size, None, g["thr"], g["known"], 4)["neg"]

    monkeypatch.setattr(orc, "generate_corruptions_for_fit_philox", sampled)
    out = fs.check_step_by_step(cfg, monkeypatch)
    assert out["steps"] == 6 and not out["diverged"]
    m2, err2 = fs._fit(cfg)
    assert err2 is None and m2.negative_sampling_stats == tot
    np.testing.assert_array_equal(m1.trained_model_params[0], m2.trained_model_params[0])
    np.testing.assert_array_equal(m1.trained_model_params[1], m2.trained_model_params[1])
