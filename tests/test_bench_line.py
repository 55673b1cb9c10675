"""bench.py's stdout contract: the LAST (and only) stdout line is a short strict-JSON summary the driver can parse from an
8 KB tail; the full result goes to bench_detail.json.  Round 4's line was one 20 KB object and the driver recorded
`parsed: null` — these tests pin the size, the strictness and the key set on a canned full result (the builder's round-4
run, tests/golden/bench_full_result.json), and on a hostile one."""
import json
import math
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANNED = os.path.join(ROOT, "tests", "golden", "bench_full_result.json")

CONTRACT_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                 "vs_baseline", "dtype", "data", "config"}
ROOFLINE_KEYS = {"bound", "achieved", "peak", "unit", "frac", "traffic"}
CPU_KEYS = {"value", "unit", "cores", "kind", "sample"}


def strict_loads(s):
    def refuse(tok):
        raise ValueError("non-strict JSON token " + tok)
    return json.loads(s, parse_constant=refuse)


def test_summary_line_is_short_strict_and_complete():
    import bench
    full = json.load(open(CANNED))
    out = bench.summary_line(full)
    assert "\n" not in out
    assert len(out.encode()) < bench.SUMMARY_MAX_BYTES <= 4096
    s = strict_loads(out)
    assert CONTRACT_KEYS <= set(s)
    assert s["metric"] == "positive+negative triples scored/sec at k=200, eta=20; filtered ranks/sec"
    assert s["value"] == full["value"] and s["ms_per_step"] == full["ms_per_step"]
    assert s["steps"] == full["steps"] and s["warmup"] == full["warmup"] and s["n_gpus"] == 1
    assert s["config"]["workload"].startswith("C3") and "model" not in s["config"]
    assert ROOFLINE_KEYS <= set(s["roofline"]) and s["roofline"]["bound"] in ("hbm", "mfma")
    assert abs(s["roofline"]["frac"] - s["roofline"]["achieved"] / s["roofline"]["peak"]) < 1e-3
    assert CPU_KEYS <= set(s["cpu_baseline"]) and s["cpu_baseline"]["kind"] in ("port", "reference")
    assert s["cpu_baseline"]["scope"] == "forward only"
    assert s["default_optimizer"]["ms_per_step"] == full["default_optimizer"]["ms_per_step"]
    assert set(s["others_ms_per_step"]) == set(full["others"])
    assert s["eval"]["exact_fast_random"]["equal_to_exact_f32_ranks"] is True
    assert s["eval"]["bf16"]["frac"] == full["eval"]["bf16"]["roofline"]["frac"]
    assert s["detail_file"] == "bench_detail.json"
    # consistency the driver checks: value = B * (1 + eta) * steps / (ms_per_step * steps)
    c = s["config"]
    assert math.isclose(s["value"], c["global_batch"] * (1 + c["eta"]) / (s["ms_per_step"] * 1e-3), rel_tol=2e-3)


def test_summary_line_survives_non_finite_numbers_and_oversized_blocks():
    import bench
    full = json.load(open(CANNED))
    full["roofline"]["traffic"] = float("nan")
    full["eval"]["bf16"]["roofline"]["frac"] = float("inf")
    full["others"] = {"W%03d" % i: {"ms_per_step": float(i)} for i in range(600)}   # would not fit: must be dropped, not truncated
    out = bench.summary_line(full)
    assert len(out.encode()) < 4096
    s = strict_loads(out)
    assert s["roofline"]["traffic"] is None
    assert CONTRACT_KEYS <= set(s) and "roofline" in s and "cpu_baseline" in s
    assert "others_ms_per_step" not in s


def test_emit_prints_exactly_one_stdout_line_and_writes_the_detail_file(tmp_path):
    code = ("import json, sys; sys.path.insert(0, %r); import bench; bench.ROOT = %r; "
            "bench.emit(json.load(open(%r)))" % (ROOT, str(tmp_path), CANNED))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.splitlines()
    assert len(lines) == 1 and len(lines[0]) < 4096
    assert strict_loads(lines[0])["value"] == json.load(open(CANNED))["value"]
    detail = strict_loads(open(os.path.join(str(tmp_path), "bench_detail.json")).read())
    assert "others" in detail and "stages" in detail and detail["value"] == strict_loads(lines[0])["value"]


class _FakeTrainer:
    """the part of emgraph_amd.training.Trainer dump_outputs reads, on host tensors"""

    def __init__(self, ent, rel):
        self.ent, self.rel = ent, rel

    def materialize(self):
        pass


class _FakeRunner:
    def __init__(self, n_ent, n_rel, k_int, B, nb, steps_run):
        import numpy as np
        import torch
        self.torch = torch
        g = torch.Generator().manual_seed(3)
        self.tr = _FakeTrainer(torch.randn(n_ent, k_int, generator=g), torch.randn(n_rel, k_int, generator=g))
        self.w = {"n_ent": n_ent, "n_rel": n_rel}
        self.B, self.nb, self.i = B, nb, steps_run
        rs = np.random.RandomState(5)
        self.X = np.stack([rs.randint(0, n_ent, nb * B), rs.randint(0, n_rel, nb * B), rs.randint(0, n_ent, nb * B)], 1).astype(np.int32)

    def spec(self, i):
        return ((i % self.nb) * self.B, self.B, i // self.nb + 1, i % self.nb + 1)


def test_dump_outputs_writes_the_last_steps_rows_as_float_arrays(tmp_path):
    """--dump-outputs: float32 / float64 .npy files only; the entity rows of the last step's positives are the table's rows;
    the same runner gives the same files; C3's dump stays far below 64 MB"""
    import numpy as np
    pytest.importorskip("torch")
    import bench
    r = _FakeRunner(n_ent=20000, n_rel=50, k_int=16, B=4096, nb=3, steps_run=5)
    bench.dump_outputs(r, 1234.5, str(tmp_path / "a"), write=True)
    bench.dump_outputs(r, 1234.5, str(tmp_path / "b"), write=True)
    bench.dump_outputs(r, 1234.5, str(tmp_path / "c"), write=False)
    assert not (tmp_path / "c").exists()
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["ent_rows_last_batch.npy", "ent_rows_sample.npy", "loss_sum.npy", "rel_table.npy"]
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
    start = (r.i - 1) % r.nb * r.B                # the last step run: i - 1
    pos = r.X[start:start + bench.DUMP_ENT_BATCH]
    ent = r.tr.ent.numpy()
    got = np.load(tmp_path / "a" / "ent_rows_last_batch.npy")
    np.testing.assert_array_equal(got, ent[np.stack([pos[:, 0], pos[:, 2]], 1).reshape(-1)])
    assert np.load(tmp_path / "a" / "ent_rows_sample.npy").shape == (bench.DUMP_ENT_SAMPLE, 16)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "rel_table.npy"), r.tr.rel.numpy())
    assert np.load(tmp_path / "a" / "loss_sum.npy").tolist() == [1234.5]
    c3 = bench.WORKLOADS["C3"]
    k_int = 2 * c3["k"]
    assert ((2 * bench.DUMP_ENT_BATCH + bench.DUMP_ENT_SAMPLE) * k_int * 4 + c3["n_rel"] * k_int * 4 + 8) < 64 << 20


@pytest.mark.gpu
def test_plain_run_times_k_steps_and_dumps_identical_outputs(tmp_path):
    """a plain `bench.py --steps K --warmup W` times exactly K steps, prints the headline only (no evaluation, CPU baseline,
    stages or secondary workloads: those are --full's) and, with --dump-outputs, writes the same arrays on every run"""
    import numpy as np
    runs = []
    for d in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
               "--dump-outputs", str(tmp_path / d)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, p.stdout[-2000:]
        runs.append(strict_loads(lines[0]))
    for s in runs:
        assert CONTRACT_KEYS <= set(s)
        assert s["steps"] == 7 and s["warmup"] == 2 and s["ms_per_step"] > 0 and s["higher_is_better"] is True
        assert s["unit"] == "triples scored/s" and s["dtype"] == "f32"
        c = s["config"]
        assert math.isclose(s["value"], c["global_batch"] * (1 + c["eta"]) / (s["ms_per_step"] * 1e-3), rel_tol=2e-3)
        assert not {"eval", "cpu_baseline", "others_ms_per_step", "roofline", "sustained"} & set(s) and not s["stages_ms"]
    total = 0
    for n in ("ent_rows_last_batch", "ent_rows_sample", "rel_table"):
        a, b = np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy"))
        assert a.dtype == np.float32 and np.all(np.isfinite(a))
        np.testing.assert_array_equal(a, b)
        total += a.nbytes
    assert total < 64 << 20
    la, lb = np.load(tmp_path / "a" / "loss_sum.npy"), np.load(tmp_path / "b" / "loss_sum.npy")
    assert la.dtype == np.float64 and np.isfinite(la[0])
    np.testing.assert_allclose(la, lb, rtol=1e-6)   # (the batch loss is summed with atomics: its last bits follow their order)
