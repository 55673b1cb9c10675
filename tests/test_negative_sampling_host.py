"""Negative sampling (Bernoulli side choice, filtered negatives), the part that needs no GPU: the host reference sampler against
the oracle's draws, the thresholds on hand-made relations, parameter validation and the refusals, the C-ABI additions — and the
conditions that keep tests/test_negative_sampling.py honest: on its graph the REFERENCE alone redraws hundreds of rows per epoch,
leaves known triples behind where it must, and chooses other sides than the fair coin; on Graph B (1024 .. 60001 known triples)
the bind's shift is >= 1 past 1024 keys and the reference examines known and unknown candidates on both sides of 2^32."""
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


# ---- Graph B: what keeps the GPU tests of the filter's second level from passing vacuously (the reference alone) ------------------
B_SETTINGS = [(sides, bern, T) for sides in (["s,o"], ["s", "o"]) for bern in (False, True) for T in (1, 4)]


def test_graph_b_is_what_its_docstring_says():
    assert [ref.coarse_index(n)[0] for n, _ in ref.SIZES_B] == list(ref.SHIFTS_B)
    assert ref.coarse_index(1024) == (0, 1024) and ref.coarse_index(1025) == (1, 513) and ref.coarse_index(60001) == (6, 938)
    assert ref.coarse_index(1) == (0, 1) and ref.coarse_index(272115)[0] == 9
    assert 1025 % 2 == 1 and 5403 % 8 and 60001 % 64          # the final run is short (at 1025: a single key, behind the coarse entry)
    for n_known, n_ids in ref.SIZES_B:
        g = ref.case_b(n_known, n_ids)
        X, ids = g["X"], g["ids"]
        assert X.shape == (n_known, 3) and len(g["known"]) == n_known and len(ids) == n_ids == len(set(ids.tolist()))
        assert set(np.unique(X[:, [0, 2]]).tolist()) <= set(ids.tolist()) and set(np.unique(X[:, 1]).tolist()) == {0, 1, 2}
        assert ids[n_ids // 2 - 1] == n_ids // 2 - 1 and ids[n_ids // 2] == ref.N_ENT_B - n_ids // 2 and ids[-1] == ref.N_ENT_B - 1
        np.testing.assert_array_equal(g["pool"], ids[::-1])
        np.testing.assert_array_equal(g["xb"], X[:300])
        keys = ref.triple_keys(X, ref.N_ENT_B, ref.N_REL)
        assert max(keys) > 10 ** 11 and sum(k < 1 << 32 for k in keys) > n_known // 3 < sum(k >= 1 << 32 for k in keys)
        from emgraph_amd import negative_sampling as NS
        np.testing.assert_array_equal(NS.known_triple_keys(X, ref.N_ENT_B, ref.N_REL), np.sort(np.array(keys, dtype=np.int64)))
        np.testing.assert_array_equal(NS.bernoulli_thresholds(X, ref.N_REL), g["thr"])


@pytest.mark.parametrize("n_known,n_ids", ref.SIZES_B)
def test_graph_b_makes_the_reference_search_both_levels_on_both_sides_of_2_32(n_known, n_ids):
    """every setting the GPU tests run on Graph B: ref.check_not_vacuous (shift, keys and examined candidates on both sides of
    2^32, >= 5 % of the rows redrawn, rows with a final attempt of 0; from 5403 keys on rows left known and every final attempt)"""
    g = ref.case_b(n_known, n_ids)
    for sides, bern, T in B_SETTINGS:
        want = ref.sample_batch(g["xb"], 3, sides, 11, 6, n_ids, g["pool"], g["thr"] if bern else None, g["known"], T)
        assert want["stats"]["rows"] == 900 * len(sides)
        ref.check_not_vacuous(g, want, T)
        for part in want["parts"]:       # the examined candidates are the final one of each row plus the known ones before it
            assert len(part["examined"]) == len(part["keep"]) + int(part["attempt"].sum())
            assert int(part["examined"][:, 3].sum()) == int(part["attempt"].sum()) + int(part["left"].sum())
            inside = np.array([tuple(r) in g["known"] for r in part["neg"].tolist()])
            np.testing.assert_array_equal(inside, part["left"])


def test_graph_b_wide_chunk_sample_and_fit_graph_redraw_too():
    """the sample of rows the wide-chunk bucket test compares, and the dense 60-entity graph fit() trains on (shift 3)"""
    g = ref.case_b(60001, 200)
    rs = np.random.RandomState(77)
    xb = g["X"][rs.randint(0, len(g["X"]), 27000)]
    rows = np.sort(rs.choice(27000 * 10, 3000, replace=False))
    parts = [ref.sample_side(xb, 10, s, 11, 6 + sd, 200, g["pool"], g["thr"], g["known"], 2, rows=rows) for sd, s in enumerate(["s", "s,o"])]
    assert all((p["attempt"] > 0).sum() >= 150 and p["left"].sum() > 0 for p in parts)
    assert all(v > 0 for v in ref.examined_counts(parts, ref.N_ENT_B, ref.N_REL).values())
    X = ref.graph_fit_b()
    assert X.shape == (5403, 3) and len(ref.known_set(X)) == 5403 and ref.coarse_index(5403) == (3, 676)
    assert set(np.unique(X[:, [0, 2]]).tolist()) == set(range(60)) and set(np.unique(X[:, 1]).tolist()) == {0, 1, 2}
    steps, tot = ref.fit_reference(X, 3, ["s,o"], 3, 3, 2, 60, None, ref.keep_thresholds(X, 3), ref.known_set(X), 4)
    assert len(steps) == 6 and tot["rows"] == 2 * 5403 * 3 and 20 * tot["redrawn"] >= tot["rows"] and tot["known_left"] > 0
    attempt = np.concatenate([p["attempt"] for s in steps for p in s[4]["parts"]])
    assert set(attempt.tolist()) == set(range(5))


def test_corner_bindings_put_candidates_outside_the_known_keys_and_on_the_extremes():
    """one known key (the smallest / the largest a candidate of the pool can have) and the pool's extreme combinations absent /
    present: the reference examines candidates below the smallest known key and above the largest one ('one_low': above only, no
    key is smaller; 'one_high': below only; 'present': neither, its extremes ARE the pool's), hits the single key, and examines the
    two extreme combinations themselves"""
    cases = ref.corner_cases_b()
    lo, hi = cases["absent"]["lo"], cases["absent"]["hi"]
    assert ref.triple_keys([lo], ref.N_ENT_B, 3) == [0] and ref.triple_keys([hi], ref.N_ENT_B, 3)[0] == 3 * ref.N_ENT_B ** 2 - 1
    assert set(cases["present"]["known"]) - set(cases["absent"]["known"]) == {lo, hi} <= set(cases["present"]["known"])
    assert len(cases["absent"]["known"]) == 2049 and len(cases["present"]["known"]) == 2051
    assert ref.coarse_index(2049)[0] == ref.coarse_index(2051)[0] == 2
    for name, g in cases.items():
        kmin, kmax = (f(ref.triple_keys(g["X"], ref.N_ENT_B, 3)) for f in (min, max))
        for sides, bern, T in B_SETTINGS:
            want = ref.sample_batch(g["xb"], 3, sides, 11, 6, len(g["pool"]), g["pool"], g["thr"] if bern else None, g["known"], T)
            ex = np.concatenate([p["examined"] for p in want["parts"]])
            keys = np.array(ref.triple_keys(ex, ref.N_ENT_B, 3))
            what = (name, sides, bern, T)
            assert (name in ("one_low", "present") or (keys < kmin).any()) and (name in ("one_high", "present") or (keys > kmax).any()), what
            if name == "one_low":
                assert kmin == 0 and (keys == 0).any() and want["stats"]["redrawn"] > 0, what
            elif name == "one_high":
                assert (keys == kmax).any() and want["stats"]["redrawn"] > 0, what
            else:       # both extreme combinations are looked up: unknown in 'absent', known in 'present'
                for t in (lo, hi):
                    hit = np.all(ex[:, :3] == np.array(t), 1)
                    assert hit.any() and np.all(ex[hit, 3] == (name == "present")), what
                assert 20 * want["stats"]["redrawn"] >= want["stats"]["rows"], what
