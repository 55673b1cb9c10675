"""The batch-local Lp / N3 regulariser, the part that needs no GPU: the float32 restatement of tests/_batchreg_ref.py
against finite differences of the float64 R, parameter parsing, the refusals (raised before fit() asks for a device), save / restore
and the ABI addition."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import _batchreg_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

X_TOY = np.array([["a", "r", "b"], ["b", "r", "c"], ["c", "q", "a"], ["a", "q", "c"]])


def _tables(seed, n_ent=9, n_rel=3, k_int=6):
    """rows away from zero: every |x| in [0.2, 1.2)"""
    rs = np.random.RandomState(seed)
    mk = lambda n: ((0.2 + rs.rand(n, k_int)) * rs.choice([-1.0, 1.0], size=(n, k_int))).astype(np.float32)  # noqa: E731
    pos = np.stack([rs.randint(0, n_ent, 12), rs.randint(0, n_rel, 12), rs.randint(0, n_ent, 12)], 1)
    pos[0] = (2, 1, 2)            # s = o
    pos[1:5, 0] = 4               # one entity in several positives
    return mk(n_ent), mk(n_rel), pos


@pytest.mark.parametrize("modulus", [False, True])
@pytest.mark.parametrize("p", [1, 2, 3])
def test_f32_rows_agree_with_finite_differences_of_the_f64_value(p, modulus):
    """the float32 rows, summed by destination, are dR/dtable: central differences of the float64 R (step h = 1e-5 on values of
    magnitude >= 0.2: truncation h^2 R''' / 6 <= 1e-10, rounding 1e-16 R / h ~ 1e-10) and the analytic float64 gradient; the f32
    rows carry at most 6 roundings of 2^-24 = 6e-8 each (the coefficient, two squares, their sum, the root, two products): rtol 1e-6"""
    E, R, pos = _tables(3 + p)
    lam_e, lam_r = 0.3, 0.7
    ge, de, gr, dr, val = ref.batch_reg(E, R, pos, p, lam_e, lam_r, modulus, modulus)
    assert ge.dtype == np.float32 and gr.dtype == np.float32 and ge.shape == (24, 6) and gr.shape == (12, 6)
    assert de.tolist() == pos[:, 0].tolist() + pos[:, 2].tolist() and dr.tolist() == pos[:, 1].tolist()
    sum_e, sum_r = ref.scatter_rows(len(E), ge, de), ref.scatter_rows(len(R), gr, dr)
    dE, dR = ref.grad64(E, R, pos, p, lam_e, lam_r, modulus, modulus)
    np.testing.assert_allclose(sum_e, dE, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(sum_r, dR, rtol=1e-6, atol=1e-9)
    f = lambda e, r: ref.value64(e, r, pos, p, lam_e, lam_r, modulus, modulus)  # noqa: E731
    np.testing.assert_allclose(val, f(E, R), rtol=1e-6)       # (f32 terms, double sum)
    h = 1e-5
    E64, R64 = E.astype(np.float64), R.astype(np.float64)
    for tab, grad, which in ((E64, sum_e, 0), (R64, sum_r, 1)):
        fd = np.zeros_like(tab)
        for idx in np.ndindex(*tab.shape):
            up, dn = tab.copy(), tab.copy()
            up[idx] += h
            dn[idx] -= h
            fd[idx] = ((f(up, R64) - f(dn, R64)) if which == 0 else (f(E64, up) - f(E64, dn))) / (2 * h)
        np.testing.assert_allclose(grad, fd, rtol=1e-5, atol=1e-7)
    assert np.abs(sum_e).max() > 0.1 and np.abs(sum_r).max() > 0.1
    assert (sum_e[np.setdiff1d(np.arange(len(E)), de)] == 0).all()          # rows no positive names: no gradient


def test_restatement_edge_values():
    """sign(0) = 0, a (0, 0) pair has gradient 0 under every p, an all-zero row adds nothing, the modulus p = 2 gradient is the plain one"""
    X = np.array([[0.0, -0.0, 2.0, -3.0], [0.0, 0.0, 0.0, 0.0], [3.0, 1e-40, 4.0, 0.0]], dtype=np.float32)
    for p in (1, 2, 3):
        for mod in (False, True):
            g, t = ref.rows_f32(X, p, mod, 0.5)
            assert g.dtype == np.float32 and t.dtype == np.float32
            assert (g[1] == 0).all() and (t[1] == 0).all()
            assert np.isfinite(g).all()
        assert ref.rows_f32(X, p, True, 0.5)[0][0, 0] == 0               # pair (0, 2): a = 0
    assert ref.rows_f32(X, 1, False, 0.5)[0][0].tolist() == [0.0, 0.0, 0.5, -0.5]
    assert ref.rows_f32(X, 1, True, 0.5)[0][2].tolist() == [np.float32(0.5) * (np.float32(3) / np.float32(5)), 0.0,
                                                            np.float32(0.5) * (np.float32(4) / np.float32(5)), 0.0]
    assert ref.rows_f32(X, 3, True, 0.5)[0][2].tolist() == [22.5, 0.0, 30.0, 0.0] and ref.rows_f32(X, 3, True, 0.5)[1][2].tolist() == [125.0, 0.0]
    assert np.array_equal(ref.rows_f32(X, 2, True, 0.5)[0], ref.rows_f32(X, 2, False, 0.5)[0])
    assert ref.coefs(1e-5, 3) == (np.float32(3e-5), np.float32(1e-5))


def test_parameter_parsing():
    from emgraph_amd.negative_sampling import batch_regularizer_params as parse
    assert parse("batch_LP", {}) == {"p": 3, "lambda_ent": 1e-5, "lambda_rel": 1e-5, "modulus_ent": False, "modulus_rel": False}
    assert parse("batch_LP", None, pair_rows=True) == {"p": 3, "lambda_ent": 1e-5, "lambda_rel": 1e-5, "modulus_ent": True, "modulus_rel": True}
    assert parse("batch_LP", {"p": 2, "lambda": [0.1, 0.2], "modulus": False}, pair_rows=True) == \
        {"p": 2, "lambda_ent": 0.1, "lambda_rel": 0.2, "modulus_ent": False, "modulus_rel": False}
    assert parse("batch_LP", {"p": np.int64(1), "lambda": 0.5, "modulus": True}) ["modulus_ent"] is False      # ignored: rows are no pairs
    # 'N3' = 'batch_LP' with p = 3 and the modulus form; only 'lambda' is read
    for lam in (0.25, [0.25, 0.5]):
        assert parse("N3", {"lambda": lam}, pair_rows=True) == parse("batch_LP", {"lambda": lam, "p": 3, "modulus": True}, pair_rows=True)
    assert parse("N3", {"lambda": 0.25, "p": 3, "modulus": False}, pair_rows=True)["modulus_ent"] is True
    assert parse("N3", {}, pair_rows=False)["modulus_ent"] is False
    for bad in ({"p": 0}, {"p": 4}, {"p": 2.0}, {"p": True}, {"p": "3"}, {"lambda": [1, 2, 3]}, {"lambda": "x"}, {"lambda": -1.0},
                {"lambda": [0.1, float("nan")]}, {"lambda": np.ones(2)}, {"modulus": 1}, {"modulus": "yes"}):
        with pytest.raises(ValueError):
            parse("batch_LP", bad, pair_rows=True)
    for p in (1, 2, np.int32(2)):
        with pytest.raises(ValueError, match="N3"):
            parse("N3", {"p": p})
    with pytest.raises(ValueError):
        parse("L2", {})


def test_rotate_relation_rows_are_not_regularised():
    from emgraph_amd.models import RotatE
    from emgraph_amd.negative_sampling import batch_regularizer_params as parse
    got = parse("N3", {"lambda": 0.1}, pair_rows=True, phase_relations=True)
    assert got == {"p": 3, "lambda_ent": 0.1, "lambda_rel": 0.0, "modulus_ent": True, "modulus_rel": False}
    assert parse("batch_LP", {"lambda": [0.1, 0.0], "p": 2}, True, True)["lambda_rel"] == 0.0
    with pytest.raises(ValueError, match="phases"):
        parse("batch_LP", {"lambda": [0.1, 0.2]}, True, True)
    m = RotatE(k=4, eta=2, epochs=1, batches_count=1, regularizer="N3", regularizer_params={"lambda": 0.1})
    assert m._batch_regularizer == got
    with pytest.raises(ValueError, match="phases"):
        RotatE(k=4, eta=2, epochs=1, batches_count=1, regularizer="batch_LP", regularizer_params={"lambda": [0.1, 0.2]})


def test_models_accept_the_two_names():
    from emgraph_amd import models as M
    for cls, mod in ((M.ComplEx, True), (M.HolE, True), (M.RotatE, True), (M.TransE, False), (M.DistMult, False), (M.SimplE, False)):
        for name in ("N3", "batch_LP"):
            m = cls(k=4, eta=2, epochs=1, batches_count=1, regularizer=name, regularizer_params={"lambda": 0.1})
            assert m.regularizer == name and m._batch_regularizer["p"] == 3 and m._batch_regularizer["modulus_ent"] is mod, (cls, name)
        assert cls(k=4, eta=2, epochs=1, batches_count=1, regularizer="LP")._batch_regularizer is None
        assert cls(k=4, eta=2, epochs=1, batches_count=1)._batch_regularizer is None
    with pytest.raises(ValueError):
        M.ComplEx(k=4, regularizer="N3", regularizer_params={"p": 2})
    with pytest.raises(ValueError):
        M.ComplEx(k=4, regularizer="batch_LP", regularizer_params={"p": 4})
    with pytest.raises(ValueError, match="Unsupported regularizer"):
        M.ComplEx(k=4, regularizer="N2")


@pytest.mark.parametrize("key,value", [("sharding", "k"), ("sharding", "batch"), ("shared_negatives", 4),
                                       ("negative_side_sampling", "bernoulli"), ("filter_negatives", True),
                                       ("negative_type_constraints", True), ("corrupt_sides", ["s,o", "p"]), ("corrupt_sides", "p")])
def test_fit_refuses_by_name_before_it_asks_for_a_device(key, value):
    from emgraph_amd.models import ComplEx
    for name in ("N3", "batch_LP"):
        with pytest.raises(NotImplementedError, match="batch regulariser") as e:
            ComplEx(k=4, eta=2, epochs=1, batches_count=1, regularizer=name, embedding_model_params={key: value}).fit(X_TOY)
        assert ("'p'" if key == "corrupt_sides" else key) in str(e.value)


def test_trainer_refusals():
    """Trainer(regularizer=...) takes the same names and refuses the same combinations, before it asks for a device"""
    from emgraph_amd import _lib as L
    from emgraph_amd.training import Trainer
    E, R = np.zeros((5, 4), np.float32), np.zeros((3, 4), np.float32)
    mk = lambda **kw: Trainer(L.COMPLEX, 4, 1.0, E, R, 2, regularizer=kw.pop("reg", "N3"), **kw)  # noqa: E731
    for sharded in ("k", "batch", True):
        with pytest.raises(NotImplementedError, match="sharded"):
            mk(sharded=sharded)
    with pytest.raises(NotImplementedError, match="shared_negatives"):
        mk(shared_negatives=4)
    with pytest.raises(NotImplementedError, match="negative sampler"):
        mk(negative_sampler={"keep_thr": None, "known_keys": None, "retries": 4})
    with pytest.raises(NotImplementedError, match="'p'"):
        mk(corrupt_sides=["s", "p"])
    with pytest.raises(ValueError, match="N3"):
        mk(regularizer_params={"p": 2})
    with pytest.raises(ValueError):
        mk(reg="batch_LP", regularizer_params={"p": 5})
    with pytest.raises(ValueError, match="phases"):
        Trainer(L.ROTATE, 4, 1.0, E, R, 2, regularizer="batch_LP", regularizer_params={"lambda": [0.1, 0.1]})


def test_save_and_restore_carry_the_regulariser(tmp_path):
    from emgraph_amd.models import ComplEx
    from emgraph_amd.utils import restore_model, save_model
    for name, params in (("N3", {"lambda": [0.05, 0.1]}), ("batch_LP", {"p": 2, "lambda": 0.02, "modulus": False})):
        m = ComplEx(k=4, eta=2, epochs=1, batches_count=1, regularizer=name, regularizer_params=params)
        path = str(tmp_path / (name + ".pkl"))
        save_model(m, path)
        r = restore_model(path)
        assert type(r) is ComplEx and r.regularizer == name and r.regularizer_params == params
        assert r.get_hyperparameter_dict()["regularizer"] == name and r._batch_regularizer == m._batch_regularizer


def test_abi_addition():
    from emgraph_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "emgraph_hip.h")).read()
    assert re.search(r"#define\s+EMG_ABI_VERSION\s+9\b", hdr) and L.ABI_VERSION == 9
    assert os.path.exists(L.LIB_PATH), "libemgraph_hip.so is not built (run __graft_entry__.build())"
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "emg_batchreg") and "emg_batchreg" in L.SIGNATURES
    assert re.search(r"\bint\s+emg_batchreg\(const emg_batchreg_args\* args, void\* stream\)", hdr)
    assert re.search(r"EMG_BATCHREG_PLAIN = 0, EMG_BATCHREG_MODULUS = 1", hdr) and (L.BATCHREG_PLAIN, L.BATCHREG_MODULUS) == (0, 1)
    assert " emg_batchreg " in open(os.path.join(ROOT, "emgraph_amd", "csrc", "build.sh")).read()
    # argument checks run on the host, before anything is launched
    lib = L.load()
    a = L.BatchregArgs()
    a.k_int, a.p, a.form_ent, a.form_rel, a.n_ent, a.n_rel, a.ld_ent, a.ld_rel, a.ldc, a.B = 8, 3, 1, 1, 50, 4, 8, 8, 8, 0
    a.coef_g_ent = a.coef_v_ent = a.coef_g_rel = a.coef_v_rel = 0.5
    assert lib.emg_batchreg(ctypes.byref(a), None) == 0                      # B == 0
    for field, bad in (("p", 0), ("p", 4), ("form_ent", 2), ("form_rel", -1), ("k_int", 7), ("k_int", 0), ("ld_ent", 4), ("ld_rel", 6),
                       ("n_ent", 0), ("n_rel", 1 << 31), ("B", -1)):
        keep = getattr(a, field)
        setattr(a, field, bad)
        assert lib.emg_batchreg(ctypes.byref(a), None) == -1, field
        assert b"emg_batchreg" in lib.emg_last_error()
        setattr(a, field, keep)
    a.form_ent = a.form_rel = 0
    a.k_int = 7                                                             # odd k_int: the plain form takes it
    assert lib.emg_batchreg(ctypes.byref(a), None) == 0
    a.B = 5                                                                 # a batch without its arrays
    assert lib.emg_batchreg(ctypes.byref(a), None) == -1 and b"null" in lib.emg_last_error()
    assert lib.emg_batchreg(None, None) == -1


def test_args_structure_has_the_headers_layout(tmp_path):
    import shutil
    import subprocess
    from emgraph_amd import _lib as L
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "emgraph_hip.h"', "int main(void) {",
             'printf("sizeof %zu\\n", sizeof(emg_batchreg_args));']
    lines += ['printf("%s %%zu\\n", offsetof(emg_batchreg_args, %s));' % (f, f) for f, _ in L.BatchregArgs._fields_]
    (tmp_path / "layout.c").write_text("\n".join(lines + ["return 0; }"]))
    subprocess.run([gcc, "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {l.split()[0]: int(l.split()[1]) for l in out if l.strip()}
    assert got["sizeof"] == ctypes.sizeof(L.BatchregArgs)
    for f, _ in L.BatchregArgs._fields_:
        assert got[f] == getattr(L.BatchregArgs, f).offset, f
