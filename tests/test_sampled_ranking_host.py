"""Sampled ranking, host side (no GPU): the declared interface, the host restatement of the draw against values worked out by hand
from the published Philox4x32-10 known-answer vectors, the two statements of the semantics on a numpy model, every refusal (raised
before the device is asked for), and the label mapping of evaluate_performance's lists."""
import os
import re

import numpy as np
import pytest

from emgraph_amd import _lib as L
from emgraph_amd.evaluation import evaluate_performance
from emgraph_amd.evaluation.protocol import map_candidates
from emgraph_amd.evaluation.ranking import check_list_ranking, rank_triples_device
from emgraph_amd.models import ComplEx
from tests import _sampled_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_signatures_declare_the_two_entry_points():
    with open(os.path.join(ROOT, "include", "emgraph_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"#define\s+EMG_ABI_VERSION\s+9\b", hdr) and L.ABI_VERSION == 9
    for name, n_args in (("emg_eval_count_lists", 18), ("emg_eval_draw_candidates", 9)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m and len(m.group(1).split(",")) == n_args == len(L.SIGNATURES[name][1]), name
    comment = hdr[:hdr.index("int emg_eval_count_lists")]
    assert "EMG_ABI_VERSION stays 9" in comment[comment.rindex("/*"):]
    with open(os.path.join(ROOT, "emgraph_amd", "csrc", "build.sh")) as f:
        assert re.search(r"\bemg_rank_lists\b", f.read())
    assert os.path.exists(os.path.join(ROOT, "emgraph_amd", "csrc", "emg_rank_lists.hip"))
    if os.path.exists(L.LIB_PATH):
        lib = L.load()
        assert hasattr(lib, "emg_eval_count_lists") and hasattr(lib, "emg_eval_draw_candidates")
    from emgraph_amd import device as D
    assert callable(D.eval_count_lists) and callable(D.eval_draw_candidates)


def test_draw_restatement_equals_hand_checked_values():
    """Random123's known-answer vector: counter (0, 0, 0, 0), key (0, 0) -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8.  That is the draw
    of test triple 0, column 0, subject side, seed 0: r64 = 0xbc57ac4c_e169c58d = 0.73571... x 2^64, so id = floor(0.73571... n)."""
    r64 = 0xbc57ac4ce169c58d
    assert [int(ref.draw_ids(0, 0, 0, 0, n)) for n in (1, 2, 300, 2 ** 31 - 1)] == [0, 1, 220, 1579931173]
    assert [(r64 * n) >> 64 for n in (1, 2, 300, 2 ** 31 - 1)] == [0, 1, 220, 1579931173]
    # a second point, every argument non-zero: philox(5, 0, 3, 1; 89abcdef, 01234567) = 99128c40 03e6c69c c113229f fffc877f
    assert int(ref.draw_ids(5, 3, 1, 0x0123456789abcdef, 300)) == (0xc113229f03e6c69c * 300) >> 64 == 226
    # the high word of the position reaches the generator: positions 2^32 apart draw differently
    assert (ref.draw_ids(np.array([7, 7 + (1 << 32)]), 0, 1, 9, 1 << 30)[0] != ref.draw_ids(np.array([7, 7 + (1 << 32)]), 0, 1, 9, 1 << 30)[1])
    # ranges: one entity draws only it; the largest table never draws n_ent
    assert not ref.draw_rows(9, 4, ref.EVAL_S_O, 7, 1, 3).any()
    big = ref.draw_rows(50, 0, ref.EVAL_S_O, 64, 2 ** 31 - 1, 3)
    assert big.dtype == np.int32 and big.min() >= 0 and big.max() <= 2 ** 31 - 2 and big.max() > 2 ** 30
    # row order and keys: object-side rows first; the two sides, two seeds and two columns differ; a chunk is a slice of the whole
    whole = ref.draw_rows(20, 0, ref.EVAL_SPO, 5, 300, 11)
    np.testing.assert_array_equal(whole[:20], ref.draw_rows(20, 0, ref.EVAL_O, 5, 300, 11))
    np.testing.assert_array_equal(whole[20:], ref.draw_rows(20, 0, ref.EVAL_S, 5, 300, 11))
    np.testing.assert_array_equal(whole[[6, 7, 26, 27]], ref.draw_rows(2, 6, ref.EVAL_S_O, 5, 300, 11))
    assert (whole[:20] != whole[20:]).any() and (whole != ref.draw_rows(20, 0, ref.EVAL_SPO, 5, 300, 12)).any()
    d = ref.draw_candidates(20, "s,o", 5, 300, 11)
    np.testing.assert_array_equal(d["o"], whole[:20])
    np.testing.assert_array_equal(d["s"], whole[20:])
    assert set(ref.draw_candidates(3, "s", 2, 300, 0)) == {"s"}


@pytest.mark.parametrize("filtered", [False, True])
def test_reference_ranks_equal_the_entities_subset_semantics(filtered):
    """on a numpy model: for lists of distinct in-range ids the walk over the entries that are not excluded gives the rank of the
    entities_subset rule (list counters minus the counters of the list's filtered members) — always under 'worst' and 'best'; under
    'middle' whenever the rule's two roundings agree with the single one, which is stated and counted here"""
    model = ref.NumpyModel(40, 3, 6, seed=2)
    rs = np.random.RandomState(4)
    T = np.stack([rs.randint(0, 40, 30), rs.randint(0, 3, 30), rs.randint(0, 40, 30)], 1)
    (a, b) = model.copies[0]
    T[0], T[1] = (5, 0, a), (b, 1, 5)             # true object a / true subject b: entities with an exact copy
    F = np.concatenate([T, np.stack([rs.randint(0, 40, 200), rs.randint(0, 3, 200), rs.randint(0, 40, 200)], 1)]) if filtered else None
    lists = {sd: np.stack([rs.permutation(40)[:25] for _ in range(30)]) for sd in "so"}
    lists["o"][0, :2], lists["s"][1, :2] = (a, b), (a, b)     # the true entity AND its copy: a tie that survives the filter
    lists["o"][0, 2:] = [e for e in range(40) if e not in (a, b)][:23]
    lists["s"][1, 2:] = [e for e in range(40) if e not in (a, b)][:23]
    agree = differ = 0
    for strategy in ("worst", "best", "middle"):
        got = ref.sampled_ranks(model, T, lists, F, "s,o", strategy)
        for col, side in enumerate("so"):
            for i in range(30):
                want = ref.subset_rank(model, T[i], lists[side][i], F, side, strategy)
                _, c = ref.side_counters(model, T[i:i + 1], lists[side][i:i + 1], F, side)
                same_rounding = (c[1, 0] - c[3, 0] + 1) // 2 == (c[1, 0] + 1) // 2 - (c[3, 0] + 1) // 2
                if strategy != "middle" or same_rounding:
                    assert got[i, col] == want, (strategy, side, i)
                    agree += 1
                else:
                    assert abs(got[i, col] - want) == 1
                    differ += 1
        np.testing.assert_array_equal(ref.sampled_ranks(model, T, lists, F, "s", strategy), got[:, 0])
        np.testing.assert_array_equal(ref.sampled_ranks(model, T, lists, F, "o", strategy), got[:, 1])
        spo = ref.sampled_ranks(model, T, lists, F, "s+o", strategy)
        if strategy != "middle":
            np.testing.assert_array_equal(spo, got[:, 0] + got[:, 1] - 1)
    assert agree >= 150 and (differ >= 2 if filtered else differ == 0)   # the two planted ties: eq = 2 of which the filter removes one
    # without a filter the true entity in its list ties with itself
    if not filtered:
        w, _ = ref.side_counters(model, T[:1], lists["o"][:1], None, "o")
        assert w[1, 0] == 2


def _fitted_stub():
    m = ComplEx(k=4, epochs=1, batches_count=1)
    m.ent_to_idx = {"a": 0, "b": 1, "c": 2}
    m.rel_to_idx = {"r": 0, "q": 1}
    m.is_fitted = True
    return m


def test_every_refusal_comes_before_the_device():
    from emgraph_amd.evaluation import TypeConstraints
    T = np.array([[0, 0, 1], [1, 1, 2]])
    ok = {"s": np.array([[0, 1], [2, 1]]), "o": np.array([[2, 2], [0, -1]])}
    call = lambda cands=ok, **kw: rank_triples_device(L.COMPLEX, None, None, 8, 1.0, T, candidates=cands, **kw)   # noqa: E731
    tc = TypeConstraints.from_pools({0: ([0, 1], None)}, (3, 2), from_idx=True)
    with pytest.raises(ValueError, match="entities_subset"):
        call(entities_subset=[0, 1])
    with pytest.raises(ValueError, match="type_constraints"):
        call(type_constraints=tc)
    with pytest.raises(NotImplementedError, match="rank_through_link"):
        call(link=L.LINK_TANH)
    with pytest.raises(NotImplementedError, match="one GPU"):
        call(shard=(0, 2))
    with pytest.raises(NotImplementedError, match="precision 1"):
        call(precision=1)
    with pytest.raises(ValueError, match="precision"):
        call(precision=3)
    for k in (0, -5):
        with pytest.raises(ValueError, match="at least 1"):
            call(k)
    with pytest.raises(ValueError, match="side 'o'"):
        call({"s": ok["s"]})
    with pytest.raises(ValueError, match="side 's'"):
        call({"o": ok["o"]}, corrupt_side="s+o")
    with pytest.raises(ValueError, match=r"\[2, K\]"):
        call({"s": ok["s"][:1], "o": ok["o"]})
    with pytest.raises(ValueError, match="integer"):
        call({"s": ok["s"].astype(float), "o": ok["o"]})
    with pytest.raises(ValueError, match="K < 1"):
        call({"o": np.zeros((2, 0), np.int32)}, corrupt_side="o")
    with pytest.raises(ValueError, match="same width"):
        call({"s": ok["s"], "o": ok["o"][:, :1]})
    with pytest.raises(ValueError, match="candidates must be"):
        call([0, 1])
    # one side is enough for a one-sided call; ids beyond int32 become padding
    out = check_list_ranking({"o": np.array([[1 << 40, 2], [0, -9]])}, "o", 2, None, None, "auto", None, L.LINK_LINEAR)
    assert out["o"].dtype == np.int32 and out["o"].tolist() == [[-1, 2], [0, -1]]
    assert check_list_ranking(np.int64(7), "s,o", 2, None, None, 0, (0, 1), L.LINK_LINEAR) == 7
    # the model and the public function
    m = _fitted_stub()
    X = np.array([["a", "r", "b"]])
    with pytest.raises(ValueError, match="entities_subset"):
        m.get_ranks_idx(T, corruption_entities=np.array([0, 1]), candidates=3)
    with pytest.raises(ValueError, match="type_constraints"):
        m.get_ranks_idx(T, type_constraints=tc, candidates=3)
    with pytest.raises(ValueError, match="entities_subset"):
        evaluate_performance(X, m, entities_subset=["a", "b"], candidates=3)
    with pytest.raises(ValueError, match="type_constraints"):
        evaluate_performance(X, m, type_constraints=tc, candidates=3)
    with pytest.raises(ValueError, match="at least 1"):
        evaluate_performance(X, m, candidates=0)
    with pytest.raises(ValueError, match="side 's'"):
        evaluate_performance(X, m, candidates={"o": np.array([["a", "b"]])})
    m.embedding_model_params["eval_precision"] = 1
    with pytest.raises(NotImplementedError, match="precision 1"):
        m.get_ranks_idx(T, candidates=3)
    with pytest.raises(NotImplementedError, match="precision 1"):
        evaluate_performance(X, m, candidates=3)
    m = _fitted_stub()
    m.embedding_model_params["sharding"] = "rows"
    with pytest.raises(NotImplementedError, match="one GPU"):
        m.get_ranks_idx(T, candidates=3)
    m = _fitted_stub()
    m.embedding_model_params.update(non_linearity="tanh", rank_through_link=True)
    with pytest.raises(NotImplementedError, match="rank_through_link"):
        m.get_ranks_idx(T, candidates=3)


def test_early_stopping_candidates_parameter_is_checked():
    m = _fitted_stub()
    xv = np.array([["a", "r", "b"]])
    for bad, msg in ((0, "at least 1"), (-3, "at least 1"), ({"s": [[0]]}, "int K"), (True, "int K"), (2.5, "int K")):
        m.early_stopping_params = {"x_valid": xv, "candidates": bad}
        with pytest.raises(ValueError, match=msg):
            m._initialize_early_stopping()
    m.early_stopping_params = {"x_valid": xv, "candidates": 4, "corruption_entities": ["a", "b"]}
    with pytest.raises(ValueError, match="corruption_entities"):
        m._initialize_early_stopping()
    m.early_stopping_params = {"x_valid": xv, "candidates": 4, "corruption_entities": "all", "candidates_seed": 9}
    es = m._initialize_early_stopping()
    assert es["candidates"] == 4 and es["candidates_seed"] == 9 and es["subset"] is None
    m.early_stopping_params = {"x_valid": xv}
    es = m._initialize_early_stopping()
    assert es["candidates"] is None and es["candidates_seed"] == 0


def test_label_mapping_and_filter_unseen_row_alignment():
    m = _fitted_stub()
    X = np.array([["a", "r", "b"], ["zed", "r", "b"], ["c", "q", "a"], ["b", "q", "mars"], ["b", "r", "c"]])
    cands = {"s": np.array([["a", "b"], ["c", "c"], ["nobody", "c"], ["a", "a"], ["b", "zed"]]),
             "o": np.array([["c", "mars"], ["a", "a"], ["b", "b"], ["c", "c"], ["a", "c"]])}
    out = map_candidates(cands, X, m, filter_unseen=True)      # rows 1 and 3 of X hold an unseen entity: dropped from the lists too
    assert out["s"].dtype == np.int32 and out["s"].tolist() == [[0, 1], [-1, 2], [1, -1]]
    assert out["o"].tolist() == [[2, -1], [1, 1], [0, 2]]
    out = map_candidates(cands, X, m, filter_unseen=False)
    assert out["s"].tolist() == [[0, 1], [2, 2], [-1, 2], [0, 0], [1, -1]] and out["o"].shape == (5, 2)
    assert map_candidates(7, X, m) == 7 and map_candidates(None, X, m) is None
    with pytest.raises(ValueError, match=r"\[5, K\]"):
        map_candidates({"s": cands["s"][:4]}, X, m)
    with pytest.raises(ValueError, match="keys"):
        map_candidates({"p": cands["s"]}, X, m)
    with pytest.raises(ValueError, match="candidates must be"):
        map_candidates([["a"]], X, m)
    # integer labels map through the same dictionaries
    m.ent_to_idx = {10: 0, 20: 1, 30: 2}
    Xi = np.array([[10, 0, 20], [30, 0, 99]])
    m.rel_to_idx = {0: 0}
    assert map_candidates({"o": np.array([[20, 99], [10, 10]])}, Xi, m)["o"].tolist() == [[1, -1]]
