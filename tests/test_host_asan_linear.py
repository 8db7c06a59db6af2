"""AddressSanitizer over the host code of the linear-regression and model-score
entry points (tests/cpp/nulldev/linear_asan.cpp): a stand-alone program linked
against the null device, as tests/test_host_asan.py builds its drivers (the
sanitized objects are shared with that module when both run in one session)."""
import os
import subprocess

from test_host_asan import _build


def test_linear_entry_points_sanitized(tmp_path):
    exe = _build(str(tmp_path), "address", driver="linear_asan.cpp")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", ND_ASYNC="0")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "linear_asan: ok" in r.stdout
