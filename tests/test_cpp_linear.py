"""Runs the C++ driver of the whole SGD_Linear loop (tests/cpp/test_linear.cpp)."""
import os
import subprocess

import pytest

BUILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "build")


@pytest.mark.gpu
def test_sgd_linear_whole_loop_gpu():
    # SGD_Linear with its DeviceBatchSampler batches and test_linearModel scores,
    # share-exact vs the computation assembled from the oracle's mulTrunc
    exe = os.path.join(BUILD, "test_linear")
    assert os.path.exists(exe), f"{exe} missing: run `make tests`"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout
    assert r.stdout.count("PASS") == 3
