"""Type constraints, host side (no GPU): the CSR layout of TypeConstraints on a hand-written graph, the filter-pool intersection
against brute force, every refusal (raised before the device is asked for), the declared interface, and — from the host reference
alone — the conditions under which the device comparisons of tests/test_type_constraints.py are not vacuous."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from emgraph_amd import _lib as L
from emgraph_amd import negative_sampling as NS
from emgraph_amd.evaluation import FilterIndex, TypeConstraints, evaluate_performance, ranks_from_counts
from emgraph_amd.evaluation.ranking import rank_triples_device
from emgraph_amd.models import ComplEx
from emgraph_amd.type_constraints import DOMAIN, RANGE
from tests import _typed_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Model:
    """what TypeConstraints reads of a model"""
    ent_to_idx = {"ann": 0, "bob": 1, "cid": 2, "rome": 3, "oslo": 4, "acme": 5}
    rel_to_idx = {"born_in": 0, "works_for": 1, "knows": 2, "unused": 3}


# (zed, born_in, rome) and (ann, born_in, mars) hold labels the model has not seen; "unused" has no triple
X = np.array([["ann", "born_in", "rome"], ["bob", "born_in", "oslo"], ["ann", "born_in", "rome"], ["cid", "born_in", "rome"],
              ["zed", "born_in", "rome"], ["ann", "born_in", "mars"], ["bob", "works_for", "acme"], ["ann", "knows", "bob"],
              ["bob", "knows", "ann"], ["cid", "knows", "ann"]])


def groups_of(tc):
    assert tc.pool_ptr.dtype == np.int64 and tc.pool_idx.dtype == np.int32 and len(tc.pool_ptr) == 2 * tc.n_rel + 1
    assert tc.pool_ptr[0] == 0 and tc.pool_ptr[-1] == len(tc.pool_idx)
    return [tc.pool_idx[tc.pool_ptr[g]:tc.pool_ptr[g + 1]].tolist() for g in range(2 * tc.n_rel)]


def test_from_triples_layout():
    tc = TypeConstraints.from_triples(X, _Model)
    assert (tc.n_ent, tc.n_rel, tc.n_groups) == (6, 4, 8)
    #                        born_in            works_for  knows                unused
    assert groups_of(tc) == [[0, 1, 2], [3, 4], [1], [5], [0, 1, 2], [0, 1], [], []]
    assert tc.pool(0, RANGE).tolist() == [3, 4] and tc.pool(3, DOMAIN) is None
    Xi = np.array([[0, 0, 3], [1, 0, 4], [0, 0, 3], [2, 0, 3], [1, 1, 5], [0, 2, 1], [1, 2, 0], [2, 2, 0]])
    for model in (_Model, (6, 4)):
        np.testing.assert_array_equal(TypeConstraints.from_triples(Xi, model, from_idx=True).pool_idx, tc.pool_idx)
    ptr, idx = ref.pools_from_triples(Xi, 4)
    np.testing.assert_array_equal(tc.pool_ptr, ptr)
    np.testing.assert_array_equal(tc.pool_idx, idx)
    np.testing.assert_array_equal(tc.row_groups([0, 3, 2, 7, -1], RANGE), [1, -1, 5, -1, -1])
    for bad in ([[0, 0, 6]], [[-1, 0, 1]], [[0, 4, 1]]):
        with pytest.raises(ValueError, match="outside"):
            TypeConstraints.from_triples(np.array(bad), (6, 4), from_idx=True)
    with pytest.raises(ValueError, match="from_idx"):
        TypeConstraints.from_triples(X, (6, 4))


def test_from_pools_layout_and_refusals():
    tc = TypeConstraints.from_pools({"born_in": (["cid", "ann"], ["oslo", "rome"]), "knows": (None, ["bob"])}, _Model)
    assert groups_of(tc) == [[0, 2], [3, 4], [], [], [], [1], [], []]          # sorted into place; missing / None: no constraint
    same = TypeConstraints.from_pools({0: ([2, 0], [4, 3]), 2: (None, [1])}, (6, 4), from_idx=True)
    np.testing.assert_array_equal(same.pool_ptr, tc.pool_ptr)
    np.testing.assert_array_equal(same.pool_idx, tc.pool_idx)
    with pytest.raises(ValueError, match="duplicate"):
        TypeConstraints.from_pools({"born_in": (["ann", "ann"], None)}, _Model)
    with pytest.raises(ValueError, match="empty"):
        TypeConstraints.from_pools({"born_in": ([], ["rome"])}, _Model)
    with pytest.raises(ValueError, match="outside"):
        TypeConstraints.from_pools({0: ([6], None)}, (6, 4), from_idx=True)
    with pytest.raises(ValueError, match="outside"):
        TypeConstraints.from_pools({4: ([1], None)}, (6, 4), from_idx=True)
    with pytest.raises(ValueError, match="unknown"):
        TypeConstraints.from_pools({"born_in": (["zed"], None)}, _Model)
    with pytest.raises(ValueError, match="unknown"):
        TypeConstraints.from_pools({"lives_in": (["ann"], None)}, _Model)
    with pytest.raises(ValueError, match="pair"):
        TypeConstraints.from_pools({"born_in": ["ann"]}, _Model)
    # the constructor validates a finished CSR
    with pytest.raises(ValueError, match="ascending and distinct"):
        TypeConstraints([0, 2, 2], [1, 1], 3, 1)
    with pytest.raises(ValueError, match="ascending and distinct"):
        TypeConstraints([0, 2, 2], [2, 1], 3, 1)
    with pytest.raises(ValueError, match="outside"):
        TypeConstraints([0, 1, 1], [3], 3, 1)
    with pytest.raises(ValueError, match="pool_ptr"):
        TypeConstraints([0, 1], [0], 3, 1)


def test_filter_intersection_against_brute_force():
    case = ref.parity_case()
    ptr, idx = ref.pools_csr(case["groups"])
    tc = TypeConstraints(ptr, idx, ref.P_N_ENT, ref.P_N_REL)
    T, F = case["T"][:97], case["F"]
    fi = FilterIndex(F)
    changed = 0
    for side_mode, sides in ((L.EVAL_O, "o"), (L.EVAL_S, "s"), (L.EVAL_S_O, "os"), (L.EVAL_SPO, "os")):
        rg = np.concatenate([ref.row_groups(T[:, 1], RANGE if sd == "o" else DOMAIN, ptr) for sd in sides])
        np.testing.assert_array_equal(rg, np.concatenate([tc.row_groups(T[:, 1], RANGE if sd == "o" else DOMAIN) for sd in sides]))
        fptr, fidx = fi.csr(T, side_mode, ref.P_N_ENT)
        gptr, gidx = tc.intersect_filter(fptr, fidx, rg)
        assert gptr.dtype == np.int64 and gidx.dtype == np.int32 and len(gptr) == len(rg) + 1 and gptr[-1] == len(gidx)
        row = 0
        for sd in sides:
            for s, p, o in T.tolist():
                known = {(b if sd == "o" else a) for a, q, b in F.tolist() if q == p and (a == s if sd == "o" else b == o)}
                known.add(o if sd == "o" else s)
                g = int(rg[row])
                want = sorted(known if g < 0 else known & set(case["groups"][g]))
                assert gidx[gptr[row]:gptr[row + 1]].tolist() == want, (side_mode, row)
                changed += len(want) != fptr[row + 1] - fptr[row]
                row += 1
    assert changed > 20   # (the intersection removed something: true entities outside their pool, known ones outside it)


def _fitted_stub():
    m = ComplEx(k=4, epochs=1, batches_count=1)
    m.ent_to_idx = {"a": 0, "b": 1, "c": 2}
    m.rel_to_idx = {"r": 0, "q": 1}
    m.is_fitted = True
    return m


def test_every_refusal_comes_before_the_device():
    tc = TypeConstraints.from_pools({0: ([0, 1], None)}, (3, 2), from_idx=True)
    T = np.array([[0, 0, 1]])
    call = lambda **kw: rank_triples_device(L.COMPLEX, None, None, 8, 1.0, T, type_constraints=tc, **kw)   # noqa: E731
    with pytest.raises(ValueError, match="entities_subset"):
        call(entities_subset=[0, 1])
    with pytest.raises(NotImplementedError, match="precision 1"):
        call(precision=1)
    with pytest.raises(NotImplementedError, match="one GPU"):
        call(shard=(0, 2))
    with pytest.raises(NotImplementedError, match="rank_through_link"):
        call(link=L.LINK_TANH)
    with pytest.raises(ValueError, match="TypeConstraints"):
        rank_triples_device(L.COMPLEX, None, None, 8, 1.0, T, type_constraints={0: ([0], None)})
    with pytest.raises(ValueError, match="precision"):
        call(precision=3)
    # the model and the public function
    m = _fitted_stub()
    with pytest.raises(ValueError, match="entities_subset"):
        m.get_ranks_idx(T, corruption_entities=np.array([0, 1]), type_constraints=tc)
    with pytest.raises(ValueError, match="entities_subset"):
        evaluate_performance(np.array([["a", "r", "b"]]), m, entities_subset=["a", "b"], type_constraints=tc)
    m.embedding_model_params["eval_precision"] = 1
    with pytest.raises(NotImplementedError, match="precision 1"):
        m.get_ranks_idx(T, type_constraints=tc)
    with pytest.raises(NotImplementedError, match="precision 1"):
        evaluate_performance(np.array([["a", "r", "b"]]), m, type_constraints=tc)
    m = _fitted_stub()
    m.embedding_model_params["sharding"] = "rows"
    with pytest.raises(NotImplementedError, match="one GPU"):
        m.get_ranks_idx(T, type_constraints=tc)
    m = _fitted_stub()
    m.embedding_model_params.update(non_linearity="tanh", rank_through_link=True)
    with pytest.raises(NotImplementedError, match="rank_through_link"):
        m.get_ranks_idx(T, type_constraints=tc)


def test_header_and_signatures_declare_the_typed_count():
    with open(os.path.join(ROOT, "include", "emgraph_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"#define\s+EMG_ABI_VERSION\s+9\b", hdr) and L.ABI_VERSION == 9
    m = re.search(r"\bint\s+emg_eval_count_grouped\s*\(([^;]*)\)\s*;", hdr)
    assert m and len(m.group(1).split(",")) == 17 == len(L.SIGNATURES["emg_eval_count_grouped"][1])
    comment = hdr[:m.start()]
    assert "EMG_ABI_VERSION stays 9" in comment[comment.rindex("/*"):]
    with open(os.path.join(ROOT, "emgraph_amd", "csrc", "build.sh")) as f:
        assert re.search(r"\bemg_rank_typed\b", f.read())
    if os.path.exists(L.LIB_PATH):
        assert hasattr(L.load(), "emg_eval_count_grouped")


# ---- the device comparisons are not vacuous: from the host reference alone ----------------------------------------------------------
@pytest.mark.parametrize("model_id", [L.COMPLEX, L.TRANSE_L1])
def test_parity_table_tells_typed_from_untyped_and_filtered_from_unfiltered(model_id):
    """On the parity table of tests/test_type_constraints.py the host chain alone gives: typed ranks that differ from the untyped
    ones on at least a quarter of the rows, and a filter that changes a typed rank."""
    case = ref.parity_case()
    n = len(case["T"])
    rank = {}
    for typed in (False, True):
        for filtered in (False, True):
            c = np.concatenate([ref.host_side_counts(model_id, case, sd, typed, filtered) for sd in "os"], axis=1)
            rank[typed, filtered] = ranks_from_counts(c[0], c[1], c[2], c[3], n, "s,o", "worst")
    assert (rank[True, False] != rank[False, False]).mean() >= 0.25
    assert (rank[True, True] != rank[True, False]).any()
    assert rank[True, True].min() >= 1
    outside = sum(int(o) not in set(case["groups"][2 * int(p) + RANGE]) for _, p, o in case["T"].tolist() if case["groups"][2 * int(p) + RANGE])
    assert outside >= 10   # true objects deliberately outside their pool
    assert len(set(np.diff(case["T"][:, 1]).tolist())) > 2   # relations in shuffled order


# ---- typed negatives: the parameter and the grown structure ----------------------------------------------------------------------------
def test_negative_type_constraints_parameter():
    tc = TypeConstraints.from_pools({0: ([0, 1], None)}, (97, 3), from_idx=True)
    assert "negative_type_constraints" in NS.KEYS
    assert NS.type_constraints_param({}) is None and NS.type_constraints_param({"negative_type_constraints": True}) is True
    assert NS.type_constraints_param({"negative_type_constraints": tc}) is tc
    assert NS.parse_params({"negative_type_constraints": tc}) == ("uniform", False, 4)
    assert NS.check_fit({"negative_type_constraints": True, "filter_negatives": True}, None, 97, 3) == ("uniform", True, 4)
    assert NS.check_fit({"negative_type_constraints": tc, "negative_corruption_entities": "all"}, None, 97, 3) == ("uniform", False, 4)
    for bad in (False, None, 1, "observed", {0: ([0], None)}):
        with pytest.raises(ValueError, match="negative_type_constraints"):
            NS.parse_params({"negative_type_constraints": bad})
        with pytest.raises(ValueError, match="negative_type_constraints"):
            NS.check_fit({"negative_type_constraints": bad}, None, 97, 3)
    for sharding in ("k", "batch"):
        with pytest.raises(NotImplementedError):
            NS.check_fit({"negative_type_constraints": True}, sharding, 97, 3)
    for pool in ("batch", ["a", "b"], 50):
        with pytest.raises(ValueError, match="negative_corruption_entities"):
            NS.check_fit({"negative_type_constraints": True, "negative_corruption_entities": pool}, None, 97, 3)
    with pytest.raises(ValueError, match="built for"):
        NS.check_fit({"negative_type_constraints": tc}, None, 98, 3)


def test_sampler_structure_grew_at_its_end_and_the_old_size_is_accepted():
    names = [f for f, _ in L.Sampler._fields_]
    assert names[:9] == ["size", "keep_thr", "known_keys", "n_known", "n_ent", "n_rel", "retries", "reserved0", "stats"]
    assert names[9:] == ["pool_ptr", "pool_idx"] and L.SAMPLER_SIZE_V1 == L.Sampler.pool_ptr.offset == 64
    with open(os.path.join(ROOT, "include", "emgraph_hip.h")) as f:
        hdr = f.read()
    body = hdr[hdr.index("typedef struct emg_sampler {"):hdr.index("} emg_sampler;")]
    assert body.index("uint64_t* stats;") < body.index("const int64_t* pool_ptr; const int32_t* pool_idx;")
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("library not built")
    lib = L.load()     # (the binding is host state: no device needed)
    a = L.Sampler()
    a.n_ent, a.n_rel, a.retries = 97, 3, 4
    assert lib.emg_sampler_bound() == 0
    for size, ok in ((L.SAMPLER_SIZE_V1, True), (C.sizeof(L.Sampler), True), (L.SAMPLER_SIZE_V1 + 8, False), (L.SAMPLER_SIZE_V1 - 8, False)):
        a.size = size
        assert (lib.emg_sampler_bind(C.byref(a)) == 0) == ok, size
        assert lib.emg_sampler_bound() == int(ok)
        assert lib.emg_sampler_bind(None) == 0
    a.size, a.pool_ptr, a.pool_idx = C.sizeof(L.Sampler), 4096, None            # (never dereferenced on the host)
    assert lib.emg_sampler_bind(C.byref(a)) != 0 and b"pool_idx" in lib.emg_last_error()
    a.size, a.pool_idx = L.SAMPLER_SIZE_V1, None                                 # the old size: the fields behind it are not read
    assert lib.emg_sampler_bind(C.byref(a)) == 0 and lib.emg_sampler_bind(None) == 0
    assert lib.emg_sampler_bound() == 0
