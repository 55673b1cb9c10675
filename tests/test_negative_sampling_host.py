"""Negative sampling (Bernoulli side choice, filtered negatives), the part that needs no GPU: the host reference sampler against
the oracle's draws, the thresholds on hand-made relations, parameter validation and the refusals, the C-ABI additions — and the
conditions that keep tests/test_negative_sampling.py honest: on its graph the REFERENCE alone redraws hundreds of rows per epoch,
leaves known triples behind where it must, and chooses other sides than the fair coin."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import emgraph_oracle as orc
from tests import _negsample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_attempt_zero_is_the_oracles_draw():
    for seed, counter, n, n_choices in ((0, 0, 900, 97), (7, 12345678901, 257, 262149), (2 ** 63 + 5, 2 ** 40 + 3, 64, 1)):
        mask, idx = orc.philox_corruption_draws(seed, counter, n, n_choices)
        w = ref.attempt_words(seed, counter, np.arange(n, dtype=np.uint64), 0)
        np.testing.assert_array_equal((w[0] & np.uint32(1)).astype(np.int32), mask)
        np.testing.assert_array_equal(np.array(ref.attempt_index(w, n_choices), np.int32), idx)
        xb = np.stack([np.arange(n) % 50, np.arange(n) % 3, (np.arange(n) * 7) % 50], 1)
        got = ref.sample_side(xb, 1, "s,o", seed, counter, n_choices)
        np.testing.assert_array_equal(got["keep"], mask)
        np.testing.assert_array_equal(got["repl"], idx)
        np.testing.assert_array_equal(got["neg"], orc.generate_corruptions_for_fit_philox(xb, eta=1, corrupt_side="s,o",
                                                                                          entities_size=n_choices, seed=seed, counter=counter))
    # a later attempt is another draw, and only the top byte of the second counter word tells them apart
    a, b = ref.attempt_words(3, 4, np.arange(8, dtype=np.uint64), 0), ref.attempt_words(3, 4, np.arange(8, dtype=np.uint64), 1)
    assert not np.array_equal(a[1], b[1])
    np.testing.assert_array_equal(b[0], orc.philox4x32_10(np.arange(8, dtype=np.uint32), np.uint32(1 << 24), np.uint32(4), np.uint32(0), 3, 0)[0])


def _thr_both(X, n_rel):
    from emgraph_amd import negative_sampling as NS
    got = NS.bernoulli_thresholds(X, n_rel)
    assert got.dtype == np.uint32
    np.testing.assert_array_equal(got, ref.keep_thresholds(X, n_rel))
    return [int(v) for v in got]


def test_thresholds_on_hand_made_relations():
    one_to_n = [(0, 0, o) for o in range(10)]                        # |S| = 1, |O| = 10: the subject is mostly REPLACED
    n_to_one = [(s, 1, 0) for s in range(10)]                        # |S| = 10, |O| = 1: the subject is mostly KEPT
    one_to_one = [(i, 2, 50 + i) for i in range(7)]
    thr = _thr_both(np.array(one_to_n + n_to_one + one_to_one + one_to_n[:3]), 4)   # (repeated triples count once)
    assert thr[0] == (1 << 32) // 11 and thr[1] == (10 << 32) // 11 and thr[2] == 1 << 31
    assert thr[3] == 1 << 31                                         # a relation without triples: a fair coin nobody tosses
    wide = np.stack([np.zeros(1 << 20, np.int64), np.zeros(1 << 20, np.int64), np.arange(1 << 20)], 1)
    from emgraph_amd import negative_sampling as NS
    t = int(NS.bernoulli_thresholds(wide, 1)[0])
    assert t == (1 << 32) // ((1 << 20) + 1) and t > 0               # one subject, 2^20 objects: still kept now and then
    mirror = wide[:, ::-1].copy()
    assert int(NS.bernoulli_thresholds(mirror, 1)[0]) == ((1 << 20) << 32) // ((1 << 20) + 1) <= (1 << 32) - 1


def test_known_keys_are_sorted_distinct_and_packed_as_documented():
    from emgraph_amd import negative_sampling as NS
    X = ref.graph_a()
    keys = NS.known_triple_keys(np.concatenate([X, X[:40]]), ref.N_ENT, ref.N_REL)
    assert keys.dtype == np.int64 and len(keys) == 898 and np.all(np.diff(keys) > 0)
    assert set(keys.tolist()) == {(s * ref.N_REL + p) * ref.N_ENT + o for s, p, o in ref.known_set(X)}
    assert NS.keys_fit(2_000_000, 1000) and not NS.keys_fit(2 ** 31 - 1, 3) and not NS.keys_fit(3_037_000_500, 1)


def test_parameter_validation_and_refusals():
    from emgraph_amd import negative_sampling as NS
    assert NS.check_fit({}, None, 97, 3) == ("uniform", False, 4)
    assert NS.check_fit({"negative_side_sampling": "bernoulli", "filter_negatives": True, "filter_negatives_retries": 255}, None, 97, 3) \
        == ("bernoulli", True, 255)
    for bad in ({"negative_side_sampling": "bern"}, {"negative_side_sampling": None}, {"filter_negatives": 1},
                {"filter_negatives": "yes"}, {"filter_negatives_retries": 0}, {"filter_negatives_retries": 256},
                {"filter_negatives_retries": 2.0}, {"filter_negatives_retries": True}):
        with pytest.raises(ValueError):
            NS.check_fit(bad, None, 97, 3)
    # with sharding asked for, the mere presence of a key is refused (defaults included), on any number of ranks
    for keys in ({"negative_side_sampling": "uniform"}, {"filter_negatives": False}, {"filter_negatives_retries": 4},
                 {"negative_side_sampling": "bernoulli"}):
        for sharding in ("k", "batch"):
            with pytest.raises(NotImplementedError):
                NS.check_fit(keys, sharding, 97, 3)
    assert NS.check_fit({}, "batch", 97, 3) == ("uniform", False, 4)
    with pytest.raises(NotImplementedError):
        NS.check_fit({"filter_negatives": True}, None, 2 ** 31 - 1, 3)        # the key would not fit
    assert NS.check_fit({"negative_side_sampling": "bernoulli"}, None, 2 ** 31 - 1, 3)[0] == "bernoulli"   # (no key needed)


def test_abi_additions():
    from emgraph_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "emgraph_hip.h")).read()
    assert re.search(r"#define\s+EMG_ABI_VERSION\s+9\b", hdr) and L.ABI_VERSION == 9
    lib = ctypes.CDLL(L.LIB_PATH)
    for sym in ("emg_sampler_bind", "emg_sampler_bound", "emg_corrupt_codes_sampled"):
        assert hasattr(lib, sym) and sym in L.SIGNATURES and re.search(r"\bint\s+%s\(" % sym, hdr), sym
    assert "protocol.py:598-641" in hdr[hdr.index("negative sampling: Bernoulli"):hdr.index("} emg_sampler;")]
    # the binding is host state: bound / unbound and its refusals without a device
    lib = L.load()
    a = L.Sampler()
    a.size, a.n_ent, a.n_rel, a.retries = ctypes.sizeof(L.Sampler), 97, 3, 4
    assert lib.emg_sampler_bound() == 0
    assert lib.emg_sampler_bind(ctypes.byref(a)) == 0 and lib.emg_sampler_bound() == 1
    assert lib.emg_sampler_bind(None) == 0 and lib.emg_sampler_bound() == 0
    a.size = 8
    assert lib.emg_sampler_bind(ctypes.byref(a)) != 0 and lib.emg_sampler_bound() == 0
    a.size, a.n_known, a.known_keys = ctypes.sizeof(L.Sampler), 5, 4096      # (never dereferenced on the host)
    a.retries = 0
    assert lib.emg_sampler_bind(ctypes.byref(a)) != 0
    a.retries, a.n_ent = 4, 2 ** 31 - 1
    assert lib.emg_sampler_bind(ctypes.byref(a)) != 0 and b"2^63" in lib.emg_last_error()
    assert lib.emg_sampler_bound() == 0


def test_sampler_structure_has_the_headers_layout(tmp_path):
    import shutil
    import subprocess
    from emgraph_amd import _lib as L
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "emgraph_hip.h"', "int main(void) {",
             'printf("sizeof %zu\\n", sizeof(emg_sampler));']
    lines += ['printf("%s %%zu\\n", offsetof(emg_sampler, %s));' % (f, f) for f, _ in L.Sampler._fields_]
    (tmp_path / "layout.c").write_text("\n".join(lines + ["return 0; }"]))
    subprocess.run([gcc, "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {l.split()[0]: int(l.split()[1]) for l in out if l.strip()}
    assert got["sizeof"] == ctypes.sizeof(L.Sampler) and L.Sampler._fields_[0][0] == "size"
    for f, _ in L.Sampler._fields_:
        assert got[f] == getattr(L.Sampler, f).offset, f


def test_graph_a_makes_the_reference_redraw_leave_known_rows_and_change_sides():
    """what the GPU tests rely on, shown by the reference alone: B = 300, eta = 3, three batches (the last one short), per epoch
    at least 200 redrawn rows and 5 rows left known under every setting with a filter, and a Bernoulli side choice that differs
    from the fair coin in at least 10 % of the rows; the planted (s, p)'s object corruptions never leave the known set"""
    X = ref.graph_a()
    known, thr = ref.known_set(X), ref.keep_thresholds(X, ref.N_REL)
    assert X.shape == (898, 3) and len(known) == 898 and set(np.unique(X[:, [0, 2]])) == set(range(ref.N_ENT))
    assert all((ref.SAT_S, ref.SAT_P, o) in known for o in range(ref.N_ENT))
    assert thr[0] < (1 << 32) // 10 and thr[1] > 9 * ((1 << 32) // 10)      # 1-to-N: subject replaced; N-to-1: subject kept
    assert -(-len(X) // 3) == 300 and len(X) - 2 * 300 == 298
    for sides in (["s,o"], ["s", "o"]):
        for kt in (None, thr):
            for T in (1, 4):
                steps, tot = ref.fit_reference(X, 3, sides, 0, 3, 2, ref.N_ENT, None, kt, known, T)
                assert len(steps) == 6 and tot["rows"] == 2 * 898 * 3 * len(sides)
                for epoch in (1, 2):
                    ep = [s[4]["stats"] for s in steps if s[0] == epoch]
                    assert sum(e["redrawn"] for e in ep) >= 200, (sides, T, epoch)
                    assert sum(e["known_left"] for e in ep) >= 5, (sides, T, epoch)
                for _, _, start, B, sb in steps:
                    xb = X[start:start + B]
                    for part in sb["parts"]:
                        sat = np.tile((xb[:, 0] == ref.SAT_S) & (xb[:, 1] == ref.SAT_P), 3) & (part["keep"] == 1)
                        assert np.all(part["left"][sat]) and np.all(part["attempt"][sat] == T)
                        inside = np.array([tuple(r) in known for r in part["neg"].tolist()])
                        np.testing.assert_array_equal(inside, part["left"])      # no negative is known but the rows counted as left
    uni, _ = ref.fit_reference(X, 3, ["s,o"], 0, 3, 1, ref.N_ENT)
    ber, _ = ref.fit_reference(X, 3, ["s,o"], 0, 3, 1, ref.N_ENT, None, thr)
    ku = np.concatenate([s[4]["parts"][0]["keep"] for s in uni])
    kb = np.concatenate([s[4]["parts"][0]["keep"] for s in ber])
    assert np.mean(ku != kb) >= 0.10
    # a row whose first candidate is unknown gets exactly the unfiltered negative
    flt, _ = ref.fit_reference(X, 3, ["s,o"], 0, 3, 1, ref.N_ENT, None, None, known, 4)
    for a, b in zip(uni, flt):
        same = b[4]["parts"][0]["attempt"] == 0
        np.testing.assert_array_equal(a[4]["codes"][same], b[4]["codes"][same])
        assert same.sum() > 0 and (~same).sum() > 0


def test_the_filter_redraws_on_the_tall_table_too():
    """the reference's counts for the GPU file's bucket-form cases are not all zero: with a 65-entity list as pool the batch on
    the tall table redraws as the one on the small table does"""
    X = ref.graph_a()
    elist = np.array([e for e in range(ref.N_ENT) if e % 3 != 1], np.int32)[::-1].copy()
    want = ref.sample_batch(X[:300], 3, ["s,o"], 11, 6, len(elist), elist, None, ref.known_set(X), 4)
    assert want["stats"]["redrawn"] >= 20 and want["stats"]["known_left"] >= 1
    # a sample of the rows is the same rows of the whole call
    some = np.array([0, 5, 299, 300, 899])
    part = ref.sample_side(X[:300], 3, "s,o", 11, 6, len(elist), elist, ref.keep_thresholds(X, 3), ref.known_set(X), 4, rows=some)
    full = ref.sample_side(X[:300], 3, "s,o", 11, 6, len(elist), elist, ref.keep_thresholds(X, 3), ref.known_set(X), 4)
    np.testing.assert_array_equal(part["codes"], full["codes"][some])
    np.testing.assert_array_equal(part["neg"], full["neg"][some])
