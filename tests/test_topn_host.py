"""Top-N completions, host side (no GPU): the declared interface, the known-completions CSR, argument validation (every check
runs before the device is asked for) and the label mapping of padded results."""
import os
import re

import numpy as np
import pytest

from emgraph_amd import _lib as L
from emgraph_amd.evaluation import FilterIndex, topn_completions
from emgraph_amd.evaluation.protocol import idx_to_labels
from emgraph_amd.evaluation.ranking import topn_device
from emgraph_amd.models import ComplEx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_signatures_declare_topn():
    with open(os.path.join(ROOT, "include", "emgraph_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"int64_t\s+emg_eval_topn_ws_bytes\s*\(", hdr)
    assert re.search(r"\bint\s+emg_eval_topn\s*\(", hdr)
    assert "EmbeddingModel.py:1856-1866" in hdr[hdr.index("top-N completions"):hdr.index("emg_eval_topn(")]
    topn_max = int(re.search(r"#define\s+EMG_TOPN_MAX\s+(\d+)", hdr).group(1))
    assert topn_max >= 100 and topn_max == L.TOPN_MAX
    assert re.search(r"#define\s+EMG_ABI_VERSION\s+9\b", hdr) and L.ABI_VERSION == 9
    assert "emg_eval_topn" in L.SIGNATURES and "emg_eval_topn_ws_bytes" in L.SIGNATURES
    assert len(L.SIGNATURES["emg_eval_topn"][1]) == 20 and len(L.SIGNATURES["emg_eval_topn_ws_bytes"][1]) == 4


# a small graph: entity 0 is a hub subject of relation 0, entity 9 a hub object of relation 1
F = np.array([[0, 0, o] for o in (1, 2, 3, 5, 8, 9)] + [[s, 1, 9] for s in (0, 2, 4, 6)] +
             [[3, 0, 4], [3, 1, 4], [7, 2, 7], [0, 0, 2]], dtype=np.int64)   # (0, 0, 2) twice
N_ENT = 10


def _sets(queries, side, subset=None):
    out = []
    for a, b in queries:
        if side == "o":
            s = {int(o) for (s_, p_, o) in F if s_ == a and p_ == b}
        else:
            s = {int(s_) for (s_, p_, o) in F if p_ == a and o == b}
        out.append(sorted(s if subset is None else s & set(subset)))
    return out


@pytest.mark.parametrize("side,queries", [("o", [(0, 0), (3, 0), (3, 1), (5, 0), (0, 7), (7, 2), (0, 1)]),
                                          ("s", [(1, 9), (0, 4), (2, 7), (0, 0), (9, 9), (0, 9)])])
@pytest.mark.parametrize("subset", [None, [9, 2, 4, 2, 0]])
def test_known_csr_matches_set_construction(side, queries, subset):
    ptr, idx = FilterIndex(F).known_csr(np.array(queries), side, N_ENT, subset)
    assert ptr.dtype == np.int64 and idx.dtype == np.int32 and ptr[0] == 0 and len(ptr) == len(queries) + 1
    got = [idx[ptr[i]:ptr[i + 1]].tolist() for i in range(len(queries))]
    assert got == _sets(queries, side, subset)   # ascending, distinct, no "own entity", empty for an unknown relation


def _fitted_stub():
    m = ComplEx(k=4, epochs=1, batches_count=1)
    m.ent_to_idx = {"a": 0, "b": 1, "c": 2}
    m.rel_to_idx = {"r": 0}
    m.is_fitted = True
    return m


def test_validation_runs_before_the_device_is_needed():
    m = _fitted_stub()
    X = np.array([["a", "r"]])
    for bad in (0, L.TOPN_MAX + 1):
        with pytest.raises(ValueError, match=str(L.TOPN_MAX)):
            topn_completions(X, m, top_n=bad)
        with pytest.raises(ValueError, match=str(L.TOPN_MAX)):
            m.get_topn_idx(np.array([[0, 0]]), top_n=bad)
        with pytest.raises(ValueError, match=str(L.TOPN_MAX)):
            topn_device(L.COMPLEX, None, None, 8, 1.0, np.array([[0, 0]]), "o", bad)
    with pytest.raises(ValueError):
        topn_completions(np.array([["a", "r", "b"]]), m)
    with pytest.raises(ValueError):
        m.get_topn_idx(np.array([[0, 0, 1]]))
    with pytest.raises(ValueError):
        topn_completions(X, m, side="s,o")
    with pytest.raises(ValueError):
        m.get_topn_idx(np.array([[0, 0]]), side="x")
    with pytest.raises(ValueError, match="entities"):
        topn_completions(np.array([["zzz", "r"]]), m)
    with pytest.raises(ValueError, match="relations"):
        topn_completions(np.array([["a", "nope"]]), m)
    with pytest.raises(ValueError, match="entities"):
        topn_completions(np.array([["r", "zzz"]]), m, side="s")
    with pytest.raises(ValueError, match="entities"):
        topn_completions(np.array([[5, 0]]), m, from_idx=True)
    with pytest.raises(ValueError, match="entities"):
        topn_completions(X, m, entities_subset=["a", "zzz"])
    unfitted = ComplEx(k=4, epochs=1, batches_count=1)
    with pytest.raises(RuntimeError, match="not been fitted"):
        topn_completions(X, unfitted)
    with pytest.raises(RuntimeError, match="not been fitted"):
        unfitted.get_topn_idx(np.array([[0, 0]]))


def test_padded_ids_map_to_none():
    ent_to_idx = {"a": 0, "b": 1, "c": 2}
    got = idx_to_labels(np.array([[2, 0, -1], [1, -1, -1]], np.int32), ent_to_idx)
    assert got.shape == (2, 3) and got.tolist() == [["c", "a", None], ["b", None, None]]
