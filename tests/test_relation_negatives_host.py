"""Relation negatives, the part that needs no GPU: the side list's canonical order and refusals (raised before fit()
asks for a device), the ABI additions, and the draw idx -> p' restated on the Philox restatement of tests/_negsample_ref.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import _relneg_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

X_TOY = np.array([["a", "r", "b"], ["b", "r", "c"], ["c", "q", "a"], ["a", "q", "c"]])


def _sides(v, key="corrupt_sides"):
    from emgraph_amd.models import ComplEx
    return ComplEx(k=4, eta=2, epochs=1, batches_count=1, embedding_model_params={key: v})._corrupt_sides()


def test_corrupt_sides_canonical_order():
    """the entity sides in the order given, then 'p', wherever it stood (on the code before this feature 'p' is a ValueError)"""
    assert _sides(["p", "s"]) == ["s", "p"]
    assert _sides("p") == ["p"] and _sides(["p"]) == ["p"] and _sides("p", key="corrupt_side") == ["p"]
    assert _sides(["s,o", "p"]) == ["s,o", "p"]
    assert _sides(["s", "p", "o"]) == ["s", "o", "p"]
    assert _sides(["o", "s"]) == ["o", "s"] and _sides("s+o") == ["s+o"]          # entity sides: as ever
    for bad in (["p", "p"], ["s", "p", "o", "p"], ["r"], "x", ["s", "P"]):
        with pytest.raises(ValueError):
            _sides(bad)
    assert ref.canonical_sides(["p", "o", "s"]) == ["o", "s", "p"]
    from emgraph_amd import _lib as L
    assert L.SIDE_IDS["p"] == L.SIDE_P and L.SIDE_P not in (L.SIDE_S, L.SIDE_O, L.SIDE_SO)


@pytest.mark.parametrize("other,value", [("sharding", "k"), ("sharding", "batch"), ("shared_negatives", 4),
                                         ("negative_side_sampling", "bernoulli"), ("negative_side_sampling", "uniform"),
                                         ("filter_negatives", True), ("negative_type_constraints", True)])
def test_fit_refuses_by_name_before_it_asks_for_a_device(other, value):
    from emgraph_amd.models import ComplEx
    for sides in ("p", ["s,o", "p"]):
        with pytest.raises(NotImplementedError, match="relation negatives") as e:
            ComplEx(k=4, eta=2, epochs=1, batches_count=1, embedding_model_params={"corrupt_sides": sides, other: value}).fit(X_TOY)
        assert other in str(e.value)


def test_transe_norm_inf_is_refused():
    from emgraph_amd.models import TransE
    with pytest.raises(NotImplementedError, match="norm inf"):
        TransE(k=4, eta=2, epochs=1, batches_count=1, embedding_model_params={"corrupt_sides": ["s", "p"], "norm": np.inf}).fit(X_TOY)


def test_trainer_refusals():
    """Trainer(corrupt_sides=...) takes the same values and refuses the same combinations, before it asks for a device"""
    from emgraph_amd import _lib as L
    from emgraph_amd.training import Trainer
    E, R = np.zeros((5, 4), np.float32), np.zeros((3, 4), np.float32)
    mk = lambda **kw: Trainer(L.DISTMULT, 4, 1.0, E, kw.pop("rel", R), 2, corrupt_sides=kw.pop("sides", ["s", "p"]), **kw)  # noqa: E731
    for sharded in ("k", "batch", True):
        with pytest.raises(NotImplementedError, match="sharded"):
            mk(sharded=sharded)
    with pytest.raises(NotImplementedError, match="shared_negatives"):
        mk(shared_negatives=4)
    with pytest.raises(NotImplementedError, match="negative sampler"):
        mk(negative_sampler={"keep_thr": None, "known_keys": None, "retries": 4})
    with pytest.raises(NotImplementedError, match="norm inf"):
        Trainer(L.TRANSE_P, 4, float("inf"), E, R, 2, corrupt_sides=["p"])
    with pytest.raises(ValueError, match="at most once"):
        mk(sides=["p", "s", "p"])
    with pytest.raises(ValueError, match="two relations"):
        mk(rel=R[:1])


def test_abi_additions():
    from emgraph_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "emgraph_hip.h")).read()
    assert re.search(r"#define\s+EMG_ABI_VERSION\s+9\b", hdr) and L.ABI_VERSION == 9
    assert os.path.exists(L.LIB_PATH), "libemgraph_hip.so is not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(L.LIB_PATH)
    for sym in ("emg_relneg_forward", "emg_relneg_backward"):
        assert hasattr(lib, sym) and sym in L.SIGNATURES and re.search(r"\bint\s+%s\(const emg_relneg_args\* args, void\* stream\)" % sym, hdr), sym
    assert "p' = idx + (idx >= p)" in hdr                                  # the shift is part of the contract
    assert " emg_relneg " in open(os.path.join(ROOT, "emgraph_amd", "csrc", "build.sh")).read()
    # argument checks run on the host, before anything is launched
    lib = L.load()
    a = L.RelnegArgs()
    a.model, a.k_int, a.scale, a.eta, a.n_ent, a.n_rel, a.ld_ent, a.ld_rel, a.B = L.COMPLEX, 8, 1.0, 3, 50, 4, 8, 8, 0
    assert lib.emg_relneg_forward(ctypes.byref(a), None) == 0 and lib.emg_relneg_backward(ctypes.byref(a), None) == 0   # B == 0
    for field, bad in (("n_rel", 1), ("model", 7), ("model", 9), ("k_int", 7), ("eta", 0), ("ld_ent", 4), ("ld_rel", 6)):
        keep = getattr(a, field)
        setattr(a, field, bad)
        assert lib.emg_relneg_forward(ctypes.byref(a), None) == -1 and lib.emg_relneg_backward(ctypes.byref(a), None) == -1, field
        assert b"emg_relneg_" in lib.emg_last_error()
        setattr(a, field, keep)
    a.model = L.SIMPLE                                                      # every model id of emg_eval_rel_scores_dense
    assert lib.emg_relneg_forward(ctypes.byref(a), None) == 0
    a.B = 5                                                                 # a batch without its arrays
    assert lib.emg_relneg_forward(ctypes.byref(a), None) != 0 and b"null" in lib.emg_last_error()
    assert lib.emg_relneg_backward(ctypes.byref(a), None) != 0 and b"null" in lib.emg_last_error()


def test_args_structure_has_the_headers_layout(tmp_path):
    import shutil
    import subprocess
    from emgraph_amd import _lib as L
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "emgraph_hip.h"', "int main(void) {",
             'printf("sizeof %zu\\n", sizeof(emg_relneg_args));']
    lines += ['printf("%s %%zu\\n", offsetof(emg_relneg_args, %s));' % (f, f) for f, _ in L.RelnegArgs._fields_]
    (tmp_path / "layout.c").write_text("\n".join(lines + ["return 0; }"]))
    subprocess.run([gcc, "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {l.split()[0]: int(l.split()[1]) for l in out if l.strip()}
    assert got["sizeof"] == ctypes.sizeof(L.RelnegArgs)
    for f, _ in L.RelnegArgs._fields_:
        assert got[f] == getattr(L.RelnegArgs, f).offset, f


def test_shift_never_names_the_positive_and_is_uniform():
    """idx -> p' on the restated draw: p' != p always; p' uniform over the other relations (chi-square bound below); n_rel = 2: every
    draw is the other relation"""
    B, eta, seed = 400, 50, 12345
    rs = np.random.RandomState(0)
    for n_rel in (2, 3, 11):
        p = rs.randint(0, n_rel, size=B)
        p[0], p[1] = 0, n_rel - 1                                           # the two edges of the shift
        idx = ref.draw_idx(B, eta, n_rel, seed, counter=7)
        assert idx.min() >= 0 and idx.max() <= n_rel - 2
        pp = ref.shift(idx, p).reshape(eta, B)
        assert (pp != p[None, :]).all() and pp.min() >= 0 and pp.max() <= n_rel - 1
        if n_rel == 2:
            assert (pp == 1 - p[None, :]).all()
            continue
        # per true relation r: the draws of its positives over the n_rel - 1 others.  Pearson's statistic of n draws over m cells is
        # chi-square with m - 1 degrees of freedom under uniformity: mean m - 1, variance 2 (m - 1); the bound is the mean + 6 sigma
        for r in range(n_rel):
            got = pp[:, p == r].reshape(-1)
            others = [q for q in range(n_rel) if q != r]
            cnt = np.array([(got == q).sum() for q in others], dtype=np.float64)
            assert cnt.sum() == got.size and got.size > 100 * len(others)
            exp = got.size / len(others)
            chi2 = ((cnt - exp) ** 2 / exp).sum()
            m1 = len(others) - 1
            assert chi2 <= m1 + 6.0 * np.sqrt(2.0 * m1), (n_rel, r, chi2)
    # hand-made: p = 1 of 4 relations: idx 0, 1, 2 -> p' 0, 2, 3
    assert ref.shift([0, 1, 2], [1]).tolist() == [0, 2, 3]
    assert ref.shift([0, 1, 2], [0]).tolist() == [1, 2, 3] and ref.shift([0, 1, 2], [3]).tolist() == [0, 1, 2]
    assert ref.negatives([[5, 1, 6], [7, 0, 8]], [0, 0, 2, 2]).tolist() == [[5, 0, 6], [7, 1, 8], [5, 3, 6], [7, 3, 8]]
