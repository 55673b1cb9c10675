"""resolve_rank_mode: the decision table of rank_triples_device, one row per rule and every pinned quirk (no GPU).  The expected
values are the rules as the ranking driver applied them before the decision became one function — written down by hand, not
taken from the function."""
import numpy as np
import pytest

from emgraph_amd import _lib as L
from emgraph_amd import device as D
from emgraph_amd.evaluation import ranking as R
from emgraph_amd.type_constraints import TypeConstraints


@pytest.fixture(autouse=True)
def _size_helpers(monkeypatch):
    """the two facts of the library the decision reads, as the library states them (include/emgraph_hip.h): widths up to 512
    columns, an order slack for every non-linear link"""
    monkeypatch.setattr(D, "prefilter_max_cols", lambda: 512)
    monkeypatch.setattr(D, "link_order_w", lambda link: 0 if link == L.LINK_LINEAR else 64)


BIG = dict(k_int=200, n_test=8192, n_ent=1 << 20)       # where 'auto' pays
SMALL = dict(k_int=200, n_test=200, n_ent=1000)
TC = TypeConstraints.from_pools({0: (np.arange(4), None)}, (10, 2), from_idx=True)
PRECISION_MSG = "precision must be 0 (exact f32), 1 (bf16 MFMA)"

# (rule, model, sizes, keyword arguments) -> (path, form, link_exact_only)  |  (exception type, fragment of its message)
ROWS = [
    ("1 link id", L.COMPLEX, SMALL, dict(link=17), (ValueError, "link must be one of the L.LINK_* ids")),
    ("1 link id first", L.COMPLEX, SMALL, dict(link=-1, candidates=0, precision=1), (ValueError, "link must be one of")),
    ("2 lists", L.COMPLEX, SMALL, dict(candidates=8, precision="auto"), ("lists", None, False)),
    ("2 lists before typed", L.COMPLEX, SMALL, dict(candidates=8, type_constraints=TC), (ValueError, "candidates and type_constraints")),
    ("2 lists refuse bf16", L.COMPLEX, SMALL, dict(candidates=8, precision=1), (NotImplementedError, "candidate lists is exact")),
    ("2 lists refuse shard", L.COMPLEX, SMALL, dict(candidates=8, shard=(0, 2)), (NotImplementedError, "candidate lists runs on one GPU")),
    ("2 lists then strategy", L.COMPLEX, SMALL, dict(candidates=8, strategy="median"), (AssertionError, "Invalid score comparision")),
    ("2 lists RotatE precision 2", L.ROTATE, SMALL, dict(candidates=8, precision=2), ("lists", None, False)),
    ("3 typed", L.COMPLEX, BIG, dict(type_constraints=TC, precision="auto"), ("typed", None, False)),
    ("3 typed refuse subset", L.COMPLEX, SMALL, dict(type_constraints=TC, entities_subset=[1, 2]), (ValueError, "both name the candidates")),
    ("3 typed refuse link", L.COMPLEX, SMALL, dict(type_constraints=TC, link=L.LINK_TANH), (NotImplementedError, "typed ranking through")),
    ("3 typed then side", L.COMPLEX, SMALL, dict(type_constraints=TC, corrupt_side="x"), (ValueError, "corruption side")),
    ("4 auto pays", L.COMPLEX, BIG, dict(precision="auto"), ("exact_fast", R.PrefilterTables, False)),
    ("4 auto small", L.DISTMULT, dict(BIG, n_test=127), dict(precision="auto"), ("exact", None, False)),
    ("4 auto few entities", L.COMPLEX, dict(BIG, n_ent=32767), dict(precision="auto"), ("exact", None, False)),
    ("4 auto subset", L.COMPLEX, BIG, dict(precision="auto", entities_subset=[1, 2]), ("exact", None, False)),
    ("4 auto narrow", L.COMPLEX, dict(BIG, k_int=32), dict(precision="auto"), ("exact", None, False)),
    ("4 auto TransE-L1", L.TRANSE_L1, BIG, dict(precision="auto"), ("exact_fast", R.SadTables, False)),
    ("4 auto TransE-L2", L.TRANSE_L2, BIG, dict(precision="auto"), ("exact_fast", R.L2Tables, False)),
    ("4 auto TransE-p", L.TRANSE_P, BIG, dict(precision="auto"), ("exact", None, False)),
    ("4 auto RotatE", L.ROTATE, BIG, dict(precision="auto"), ("exact_fast", R.RotateTables, False)),
    ("4 auto RotatE small", L.ROTATE, SMALL, dict(precision="auto"), ("exact", None, False)),
    ("4+7 auto RotatE sharded", L.ROTATE, BIG, dict(precision="auto", shard=(1, 2)), (NotImplementedError, "RotatE is ranked on one GPU")),
    ("4 auto RotatE one rank", L.ROTATE, BIG, dict(precision="auto", shard=(0, 1)), ("exact_fast", R.RotateTables, False)),
    ("4 auto RotatE tanh", L.ROTATE, BIG, dict(precision="auto", link=L.LINK_TANH), ("exact", None, True)),
    ("4 auto ComplEx tanh", L.COMPLEX, BIG, dict(precision="auto", link=L.LINK_TANH), ("exact_fast", R.PrefilterTables, False)),
    ("5 bf16 under a link", L.COMPLEX, SMALL, dict(precision=1, link=L.LINK_SIGMOID), (NotImplementedError, "does not rank through a non-linear link")),
    ("5 TransE-L1 fast tanh", L.TRANSE_L1, SMALL, dict(precision=2, link=L.LINK_TANH), ("exact", None, True)),
    ("5 TransE-L1 exact tanh", L.TRANSE_L1, SMALL, dict(precision=0, link=L.LINK_TANH), ("exact", None, True)),
    ("5 ComplEx fast tanh", L.COMPLEX, SMALL, dict(precision=2, link=L.LINK_TANH), ("exact_fast", R.PrefilterTables, False)),
    ("5 ComplEx exact tanh", L.COMPLEX, SMALL, dict(precision=0, link=L.LINK_TANH), ("exact", None, False)),
    ("5 before 6: TransE-p bf16 tanh", L.TRANSE_P, SMALL, dict(precision=1, link=L.LINK_TANH), (NotImplementedError, "non-linear link")),
    ("6 TransE-p bf16", L.TRANSE_P, SMALL, dict(precision=1), ("exact", None, False)),
    ("6 TransE-p out of range", L.TRANSE_P, SMALL, dict(precision=7), ("exact", None, False)),
    ("6 TransE-p fast", L.TRANSE_P, BIG, dict(precision=2), ("exact", None, False)),
    ("7 RotatE explicit 2", L.ROTATE, BIG, dict(precision=2), (NotImplementedError, "precision 2 has no RotatE form")),
    ("7 RotatE explicit 1", L.ROTATE, BIG, dict(precision=1), (NotImplementedError, "precision 1 has no RotatE form")),
    ("7 RotatE sharded", L.ROTATE, SMALL, dict(precision=0, shard=(0, 4)), (NotImplementedError, "RotatE is ranked on one GPU")),
    ("7 RotatE exact", L.ROTATE, BIG, dict(precision=0), ("exact", None, False)),
    ("7 before 9: RotatE out of range", L.ROTATE, SMALL, dict(precision=7), (ValueError, PRECISION_MSG)),
    ("8 SimplE sharded", L.SIMPLE, SMALL, dict(precision=0, shard=(0, 2)), (NotImplementedError, "SimplE is ranked on one GPU")),
    ("8 before 9: SimplE sharded out of range", L.SIMPLE, SMALL, dict(precision=5, shard=(0, 2)), (NotImplementedError, "SimplE")),
    ("8 SimplE one GPU", L.SIMPLE, SMALL, dict(precision=2), ("exact_fast", R.PrefilterTables, False)),
    ("9 out of range", L.COMPLEX, SMALL, dict(precision=3), (ValueError, PRECISION_MSG)),
    ("9 a string", L.COMPLEX, SMALL, dict(precision="fast"), (ValueError, PRECISION_MSG)),
    ("10 fast with a subset", L.COMPLEX, SMALL, dict(precision=2, entities_subset=[1, 2, 3]), ("exact", None, False)),
    ("11 SAD", L.TRANSE_L1, SMALL, dict(precision=2), ("exact_fast", R.SadTables, False)),
    ("11 L2", L.TRANSE_L2, SMALL, dict(precision=2), ("exact_fast", R.L2Tables, False)),
    ("11 half precision", L.HOLE, SMALL, dict(precision=2, shard=(1, 4)), ("exact_fast", R.PrefilterTables, False)),
    ("12 TransE-L1 bf16", L.TRANSE_L1, SMALL, dict(precision=1), (ValueError, "needs a contraction model")),
    ("12 ComplEx bf16", L.COMPLEX, SMALL, dict(precision=1), ("bf16", None, False)),
    ("12 before 13", L.TRANSE_L2, SMALL, dict(precision=1, corrupt_side="x"), (ValueError, "needs a contraction model")),
    ("13 side", L.COMPLEX, SMALL, dict(precision=0, corrupt_side="o,s"), (ValueError, "Invalid argument value for corruption side")),
    ("13 before 14", L.COMPLEX, SMALL, dict(corrupt_side="x", strategy="x"), (ValueError, "corruption side")),
    ("14 strategy", L.COMPLEX, SMALL, dict(precision=2, strategy="median"), (AssertionError, "Invalid score comparision type!")),
    ("defaults", L.DISTMULT, SMALL, dict(), ("exact", None, False)),
]


@pytest.mark.parametrize("rule,model_id,sizes,kw,want", ROWS, ids=[r[0] for r in ROWS])
def test_decision_table(rule, model_id, sizes, kw, want):
    args = (model_id, sizes["k_int"], sizes["n_test"], sizes["n_ent"])
    if isinstance(want[0], type):
        with pytest.raises(want[0]) as err:
            R.resolve_rank_mode(*args, **kw)
        assert type(err.value) is want[0] and want[1] in str(err.value)
        return
    mode = R.resolve_rank_mode(*args, **kw)
    assert (mode.path, mode.form, mode.link_exact_only) == want
    assert (mode.candidates is not None) == (want[0] == "lists")


def test_mode_is_immutable_and_carries_the_normalised_lists():
    lists = {"o": np.array([[1, 2], [3, 1 << 40]], dtype=np.int64)}
    mode = R.resolve_rank_mode(L.COMPLEX, 40, 2, 64, candidates=lists, corrupt_side="o")
    assert mode.candidates["o"].dtype == np.int32 and mode.candidates["o"].tolist() == [[1, 2], [3, -1]]
    with pytest.raises(AttributeError):
        mode.path = "exact"


def test_the_names_other_code_imports_stay():
    for name in ("resolve_auto_precision", "link_prefilter_applies", "check_list_ranking", "check_typed_ranking", "derived_tables",
                 "PrefilterTables", "L2Tables", "SadTables", "RotateTables", "_pair_buffer", "_acc_scale", "_PROBE_MAX_UNDECIDED",
                 "prefilter_band", "prefilter_band_reference", "table_norm_bounds", "rotate_image_scale", "ROTATE_ENT_MAX",
                 "ROTATE_FAST_AUTO", "CONTRACTION_MODELS", "_cmp", "_stable_argsort", "ranks_from_counts", "build_filter_csr"):
        assert hasattr(R, name), name
