"""Shared negatives, the part that needs no GPU: the key's validation and refusals (raised before fit() asks for a device), the
code expansion the feature is defined by (tests/_shared_ref.py) on hand-written cases, and the ABI additions."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import _shared_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

X_TOY = np.array([["a", "r", "b"], ["b", "r", "c"], ["c", "q", "a"], ["a", "q", "c"]])


def test_key_validation():
    from emgraph_amd import negative_sampling as NS
    assert NS.shared_negatives_param({}) is None
    assert NS.shared_negatives_param({"shared_negatives": 1}) == 1
    assert NS.shared_negatives_param({"shared_negatives": np.int64(256)}) == 256
    assert NS.shared_negatives_param({"shared_negatives": 64, "negative_corruption_entities": "batch", "corrupt_side": "s"}) == 64
    for bad in (0, -3, 257, 1 << 20, 16.0, "16", True, None, [16]):
        with pytest.raises(ValueError):
            NS.shared_negatives_param({"shared_negatives": bad})


@pytest.mark.parametrize("other,value", [("sharding", "k"), ("sharding", "batch"), ("negative_side_sampling", "bernoulli"),
                                         ("negative_side_sampling", "uniform"), ("filter_negatives", True),
                                         ("negative_type_constraints", True)])
def test_refused_combinations_name_both_keys(other, value):
    from emgraph_amd import negative_sampling as NS
    with pytest.raises(NotImplementedError) as e:
        NS.shared_negatives_param({"shared_negatives": 16, other: value})
    assert "shared_negatives" in str(e.value) and other in str(e.value)
    with pytest.raises(ValueError):                       # a bad value is reported first, whatever else is set
        NS.shared_negatives_param({"shared_negatives": 0, other: value})


def test_fit_decides_before_it_asks_for_a_device():
    """fit() raises the key's own errors ahead of require_gpu(): the same answer on a box without a GPU"""
    from emgraph_amd.models import ComplEx, TransE
    for bad in (0, 257, 2.5, "8", True):
        with pytest.raises(ValueError, match="shared_negatives"):
            ComplEx(k=4, eta=2, epochs=1, batches_count=1, embedding_model_params={"shared_negatives": bad}).fit(X_TOY)
    for other, value in (("sharding", "batch"), ("negative_side_sampling", "bernoulli"), ("filter_negatives", True),
                         ("negative_type_constraints", True)):
        with pytest.raises(NotImplementedError, match="shared_negatives") as e:
            ComplEx(k=4, eta=2, epochs=1, batches_count=1, embedding_model_params={"shared_negatives": 16, other: value}).fit(X_TOY)
        assert other in str(e.value)
    with pytest.raises(NotImplementedError, match="shared_negatives"):
        TransE(k=4, eta=2, epochs=1, batches_count=1, embedding_model_params={"shared_negatives": 4, "norm": np.inf}).fit(X_TOY)


def test_expansion_on_hand_written_cases():
    # B = 4, C = 2, one slot: chunk 0 = rows 0, 1; chunk 1 = rows 2, 3
    assert ref.n_chunks(4, 2) == 2
    assert ref.expand_codes([7, 9], 4, 2, 1).tolist() == [7, 7, 9, 9]
    # B = 5, C = 2 (B % C != 0: the last chunk holds one row), two slots, slot-major layout m * G + g
    assert ref.n_chunks(5, 2) == 3
    cc = [10, 11, 12, 20, 21, 22]
    assert ref.expand_codes(cc, 5, 2, 2).tolist() == [10, 10, 11, 11, 12, 20, 20, 21, 21, 22]
    # C = 1 is the ordinary step's own layout; C >= B is one chunk
    assert ref.expand_codes([3, 4, 5, 6, 7, 8], 3, 1, 2).tolist() == [3, 4, 5, 6, 7, 8]
    assert ref.expand_codes([3, 4], 3, 256, 2).tolist() == [3, 3, 3, 4, 4, 4]
    # the keep-subject bit travels with the code: it holds for the whole chunk
    keep = np.array([5 | (1 << 31), 6], dtype=np.uint32).view(np.int32)
    codes = ref.expand_codes(keep, 3, 2, 1)
    repl, kept = ref.split_codes(codes)
    assert repl.tolist() == [5, 5, 6] and kept.tolist() == [1, 1, 0]
    pos = np.array([[0, 0, 1], [2, 1, 3], [4, 0, 5]])
    assert ref.negatives(pos, codes, 1).tolist() == [[0, 0, 5], [2, 1, 5], [6, 0, 5]]


def test_reference_gradients_against_finite_differences():
    """the float64 restatement the GPU tests compare with is itself the derivative of the scores (central differences)"""
    rs = np.random.RandomState(3)

    def score(model, a, p, b, scale):
        if model in (ref.TRANSE_L1, ref.TRANSE_L2, ref.TRANSE_P):
            d = np.abs(a + p - b)
            o = {ref.TRANSE_L1: 1.0, ref.TRANSE_L2: 2.0}.get(model, scale)
            return -(d ** o).sum(1) ** (1.0 / o)
        if model == ref.DISTMULT:
            return (a * p * b).sum(1)
        n = a.shape[1] // 2
        ac, bc = a[:, :n] + 1j * a[:, n:], b[:, :n] + 1j * b[:, n:]
        if model == ref.ROTATE:
            return -np.abs(ac * np.exp(1j * p[:, :n]) - bc).sum(1)
        return (scale if model == ref.HOLE else 1.0) * ((p[:, :n] + 1j * p[:, n:]) * ac * np.conj(bc)).real.sum(1)

    for model, scale in ((ref.TRANSE_L1, 1.0), (ref.TRANSE_L2, 1.0), (ref.DISTMULT, 1.0), (ref.COMPLEX, 1.0), (ref.HOLE, 0.25),
                         (ref.TRANSE_P, 3.0), (ref.ROTATE, 1.0)):
        a, p, b = rs.randn(3, 6), rs.randn(3, 6), rs.randn(3, 6)
        g = rs.randn(3)
        grads = ref.triple_grads(model, a, p, b, g, scale)
        for which, arr in enumerate((a, p, b)):
            for c in range(6):
                hi, lo = [x.copy() for x in (a, p, b)], [x.copy() for x in (a, p, b)]
                hi[which][:, c] += 1e-6
                lo[which][:, c] -= 1e-6
                fd = g * (score(model, *hi, scale) - score(model, *lo, scale)) / 2e-6
                np.testing.assert_allclose(grads[which][:, c], fd, rtol=1e-5, atol=1e-7, err_msg=str((model, which, c)))


def test_abi_additions():
    from emgraph_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "emgraph_hip.h")).read()
    assert re.search(r"#define\s+EMG_ABI_VERSION\s+9\b", hdr) and L.ABI_VERSION == 9
    assert os.path.exists(L.LIB_PATH), "libemgraph_hip.so is not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(L.LIB_PATH)
    for sym in ("emg_shared_forward", "emg_shared_backward"):
        assert hasattr(lib, sym) and sym in L.SIGNATURES and re.search(r"\bint\s+%s\(const emg_shared_args\* args, void\* stream\)" % sym, hdr), sym
    assert "codes[m * B + i] = chunk_codes[m * G + i / C]" in hdr       # the identity is part of the contract
    assert "emg_shared.hip" in open(os.path.join(ROOT, "emgraph_amd", "csrc", "emg_shared.hip")).read()
    assert " emg_shared " in open(os.path.join(ROOT, "emgraph_amd", "csrc", "build.sh")).read()
    # argument checks run on the host, before anything is launched
    lib = L.load()
    a = L.SharedArgs()
    a.model, a.k_int, a.scale, a.eta_total, a.n_ent, a.n_rel, a.ld_ent, a.ld_rel, a.B, a.C = L.COMPLEX, 8, 1.0, 3, 50, 4, 8, 8, 0, 16
    assert lib.emg_shared_forward(ctypes.byref(a), None) == 0 and lib.emg_shared_backward(ctypes.byref(a), None) == 0   # B == 0
    for field, bad in (("C", 0), ("C", 257), ("model", 7), ("k_int", 7), ("eta_total", 0), ("ld_ent", 4)):
        keep = getattr(a, field)
        setattr(a, field, bad)
        assert lib.emg_shared_forward(ctypes.byref(a), None) != 0 and lib.emg_shared_backward(ctypes.byref(a), None) != 0, field
        assert b"emg_shared_" in lib.emg_last_error()
        setattr(a, field, keep)
    a.B = 5                                                              # a batch without its arrays
    assert lib.emg_shared_forward(ctypes.byref(a), None) != 0 and b"null" in lib.emg_last_error()


def test_args_structure_has_the_headers_layout(tmp_path):
    import shutil
    import subprocess
    from emgraph_amd import _lib as L
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "emgraph_hip.h"', "int main(void) {",
             'printf("sizeof %zu\\n", sizeof(emg_shared_args));']
    lines += ['printf("%s %%zu\\n", offsetof(emg_shared_args, %s));' % (f, f) for f, _ in L.SharedArgs._fields_]
    (tmp_path / "layout.c").write_text("\n".join(lines + ["return 0; }"]))
    subprocess.run([gcc, "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {l.split()[0]: int(l.split()[1]) for l in out if l.strip()}
    assert got["sizeof"] == ctypes.sizeof(L.SharedArgs)
    for f, _ in L.SharedArgs._fields_:
        assert got[f] == getattr(L.SharedArgs, f).offset, f
