"""bench.py's contract that can be checked without a GPU: it refuses to run (loudly) when no gfx950 device is present --
there is no CPU path to fall back to -- and its JSON keys are the ones the driver reads."""
import ast
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


@pytest.mark.skipif(not _no_gpu(), reason="only meaningful on a machine without a GPU")
def test_bench_fails_loudly_without_gpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0"], capture_output=True, timeout=300)
    assert r.returncode != 0
    assert b"needs a gfx950 GPU" in r.stderr + r.stdout and not r.stdout.strip().startswith(b"{")


def test_bench_json_keys_and_oracle_use():
    src = open(os.path.join(ROOT, "bench.py")).read()
    tree = ast.parse(src)
    keys = {k.value for node in ast.walk(tree) if isinstance(node, ast.Dict) for k in node.keys if isinstance(k, ast.Constant) and isinstance(k.value, str)}
    keys |= {n.slice.value for n in ast.walk(tree) if isinstance(n, ast.Subscript) and isinstance(n.slice, ast.Constant) and isinstance(n.slice.value, str)}
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "workload", "roofline", "bound", "achieved", "peak", "frac", "traffic", "cpu_baseline", "cores", "kind", "sample"):
        assert k in keys, k
    # the oracle is imported only inside the cpu_baseline leg and the optional --check, never at module level
    top_imports = {a.name for node in tree.body if isinstance(node, (ast.Import, ast.ImportFrom)) for a in node.names}
    assert "ora" not in top_imports


def test_dump_outputs_is_order_free_and_bounded(tmp_path):
    """--dump-outputs: float .npy files only, under 64 MB, and the same files whatever order the engine leaves its rows and keys in"""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench

    class Arr:                           # what skx_engine.Array.export returns: keys, rows x samples codes, per-row counts
        def __init__(self, keys, var, counts):
            self.out = keys, var, counts

        def export(self):
            return tuple(x.copy() for x in self.out)

    rng = np.random.default_rng(3)
    U, S, K = 60_000, 900, 200_000
    keys = np.zeros(K, [("lo", "<u8"), ("hi", "<u8")])
    keys["lo"] = rng.integers(0, 1 << 62, K, dtype=np.uint64)
    var = rng.choice(np.frombuffer(b"ACGT-", np.uint8), size=(U, S))
    counts = rng.integers(0, S, U).astype(np.uint64)
    pr, pk = rng.permutation(U), rng.permutation(K)
    bench.dump_outputs(str(tmp_path / "a"), Arr(keys, var, counts), (K, U, K - U))
    bench.dump_outputs(str(tmp_path / "b"), Arr(keys[pk], var[pr], counts[pr]), (K, U, K - U))
    var[17, 5] = ord("N")
    bench.dump_outputs(str(tmp_path / "c"), Arr(keys, var, counts), (K, U, K - U))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "kept_rows_sample.npy" in names and "step_shape.npy" in names
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
    assert np.load(tmp_path / "a" / "step_shape.npy").tolist() == [K, U, K - U, S]
    assert 0 < len(np.load(tmp_path / "a" / "kept_rows_sample.npy")) < U
    assert not np.array_equal(np.load(tmp_path / "a" / "kept_rows_digest.npy"), np.load(tmp_path / "c" / "kept_rows_digest.npy"))
