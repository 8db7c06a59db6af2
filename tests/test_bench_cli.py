"""bench.py's command line: a plain run times the steps and prints the line
without the --full legs, and --dump-outputs writes the last step's revealed
product (checked against the plaintext product of the job's operands)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "kernel_ms_per_step", "local_compute", "binary", "extras", "cpu_baseline")


def _random_mat(rows, cols, seed, bound):
    """Session.cpp randomMat: the job's operands (xorshift64, values in [-bound, bound))."""
    mask = (1 << 64) - 1
    x = (seed * 0x9E3779B97F4A7C15 + 12345) & mask
    out = np.empty(rows * cols, dtype=object)
    for i in range(rows * cols):
        x ^= (x << 13) & mask
        x ^= x >> 7
        x ^= (x << 17) & mask
        out[i] = x % (2 * bound) - bound
    return out.reshape(rows, cols)


class _FakeSession:
    """result(party) as native.Session gives it: two int64 share arrays."""

    def __init__(self, value, seed):
        rng = np.random.default_rng(seed)
        r = rng.integers(0, 1 << 64, size=(2, value.size), dtype=np.uint64)
        self.first = [r[0], r[1], value.astype(np.int64).view(np.uint64) - r[0] - r[1]]  # wraps mod 2^64

    def result(self, party):
        return self.first[party].view(np.int64), self.first[(party + 2) % 3].view(np.int64)


def test_plain_run_is_the_default():
    import bench

    old = sys.argv
    sys.argv = ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"]
    try:
        args = bench.parse()
    finally:
        sys.argv = old
    assert args.full is False and args.dump_outputs is None and args.steps == 7 and args.warmup == 3


def test_dump_outputs_reveals_the_shares(tmp_path, monkeypatch):
    import bench

    rows, cols, d = 5, 7, 16
    value = np.random.default_rng(3).integers(-(1 << 32), 1 << 32, size=rows * cols)
    bench.dump_outputs(_FakeSession(value, 4), str(tmp_path / "a"), rows, cols, d)
    got = np.load(tmp_path / "a" / "product.npy")
    assert got.dtype == np.float64 and got.shape == (rows, cols)
    assert np.array_equal(got.ravel() * (1 << d), value)
    # above the size limit: the same seeded sample of the entries, in order
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 10 * 8)
    bench.dump_outputs(_FakeSession(value, 5), str(tmp_path / "b"), rows, cols, d)
    sample = np.load(tmp_path / "b" / "product.npy")
    assert sample.dtype == np.float64 and sample.shape == (10,)
    idx = np.sort(np.random.default_rng(0).choice(rows * cols, 10, replace=False))
    assert np.array_equal(sample * (1 << d), value[idx])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_product(gpu, tmp_path):
    """A small plain run in a process of its own: 96 x 80 . 80 x 72 (no
    multiple of the GEMM's tiles), 3 timed steps."""
    M, K, N, D = 96, 80, 72, 16
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--m", str(M), "--k", str(K), "--n", str(N), "--decimal", str(D), "--prewarm-s", "0",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"):
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "mults/s" and line["dtype"] == "int64"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(M * K * N / (line["ms_per_step"] / 1e3), rel=1e-6)
    for k in FULL_ONLY:
        assert k not in line, k + " belongs to --full"
    assert sorted(os.listdir(out)) == ["product.npy"]
    got = np.load(out / "product.npy")
    assert got.dtype == np.float64 and got.shape == (M, N)
    # the plaintext product, truncated: the protocol's result is within
    # [-3, +1] units of the last fixed-point place of floor(a.b / 2^D), the
    # bound of the session's own check (Session.cpp MulJob::check)
    a, b = _random_mat(M, K, 1, 8 << D), _random_mat(K, N, 2, 8 << D)
    want = np.array([[int(v) >> D for v in row] for row in a.dot(b)], dtype=np.float64)
    diff = got * (1 << D) - want
    assert diff.min() >= -3 and diff.max() <= 1, (diff.min(), diff.max())
