"""CPU checks behind the linear-regression / model-score GPU tests: the numpy
restatement (tests/ml_restate.py) is pinned to the oracle's share product, the
truncation bound it is used with is confirmed on every input set the GPU tests
use, and the linear dataset generator is checked on its own."""
import numpy as np
import pytest

import ml_restate as mr
import oracle as orc
from aby3_amd import native as nt


def _ops(M, K, N, seed, bits=63):
    rng = np.random.default_rng(seed)
    lo, hi = -(2**bits), 2**bits - 1
    return (rng.integers(lo, hi, size=M * K, dtype=np.int64, endpoint=True),
            rng.integers(lo, hi, size=K * N, dtype=np.int64, endpoint=True))


@pytest.mark.parametrize("M,K,N,trunc,d", [(33, 17, 65, False, 0), (100, 70, 50, True, 16), (128, 256, 1, True, 27)])
def test_restatement_reproduces_oracle_sim_mul(M, K, N, trunc, d):
    """makeEncryptors(0) / makeEvaluators(1) seeds, as orc.sim_mul: the same
    shares of every party and the same revealed values."""
    a, b = _ops(M, K, N, 100 + M)
    esh, eplain = orc.sim_mul(mr.GEMM, trunc, d, a, b, M, K, N)
    sh, plain = mr.sim_mul(trunc, d, a, b, M, K, N)
    assert np.array_equal(sh, esh)
    assert np.array_equal(plain, eplain)


def _check_log(log):
    assert log
    for a, b, c, M, K, N, d in log:
        x = mr.exact_product(a, b, M, K, N)
        assert max(abs(int(v)) for v in x) < 2**61, "inputs must keep the exact product inside 2^61"
        lo, hi = mr.trunc_bounds(x, d)
        got = np.asarray([int(v) for v in c], dtype=object)
        assert np.all(lo <= got) and np.all(got <= hi), (M, K, N, d)


@pytest.mark.parametrize("name", list(mr.LINEAR_CASES))
def test_truncation_bound_linear_cases(name):
    """Every mulTrunc of the linear iterations the GPU tests run reveals a value
    in [floor(x / 2^d) - 3, floor(x / 2^d)], x the exact product of its revealed operands."""
    _, _, log = mr.linear_expected(name)
    c = mr.LINEAR_CASES[name]
    assert len(log) == 2 * c["iters"]
    _check_log(log)


@pytest.mark.parametrize("name", list(mr.SCORE_CASES))
def test_truncation_bound_score_cases(name):
    exp, log = mr.score_expected(name)
    assert len(log) == 2
    _check_log(log)
    n = mr.SCORE_CASES[name]["n"]
    assert exp["score"] == float(exp["l2"][0]) / 2.0**mr.D / n


def test_truncation_bound_logistic_inputs():
    """The logistic input set: the restatement's x w (the linear score's
    prediction, which the logistic score feeds to the sigmoid) and its l2 obey
    the bound; and on the plaintext inputs x w, and the l2 of the largest error
    the sigmoid allows (|f - y| <= 1), stay inside 2^61."""
    exp, log = mr.logistic_expected()
    assert len(log) == 2
    _check_log(log)
    X, Y, w = mr.logistic_inputs()
    assert np.array_equal(log[0][2], exp["pred"])
    n, d = X.shape
    x = mr.exact_product(X, w, n, d, 1)
    assert max(abs(int(v)) for v in x) < 2**61
    assert n * (2**mr.D) ** 2 < 2**61
    f = np.asarray([int(v) >> mr.D for v in x], dtype=object)
    half = 2 ** (mr.D - 1)
    assert (f < -half).any() and (f >= half).any() and ((f >= -half) & (f < half)).any(), "all three sigmoid regions"


def test_linear_dataset_deterministic_and_prefix():
    X, Y, m = nt.linear_dataset(64, 16, 16)
    X2, Y2, m2 = nt.linear_dataset(64, 16, 16)
    assert np.array_equal(X, X2) and np.array_equal(Y, Y2) and np.array_equal(m, m2)
    # the first k rows of an n-row draw are the k-row draw (the reference's
    # test set is the training set's head for this reason)
    Xk, Yk, _ = nt.linear_dataset(20, 16, 16)
    assert np.array_equal(X[:20], Xk) and np.array_equal(Y[:20], Yk)
    # the model is the logistic dataset's (main-linear.cpp:37-45)
    assert np.array_equal(m, nt.lr_dataset(1, 16, 16)[2])


def test_linear_dataset_noise_statistics():
    """Y = X model + noise with noise ~ N(1, 1): (Y - X model) / 2^D has mean
    and standard deviation within 0.05 of 1 at n = 4096, dim = 16."""
    n, dim, D = 4096, 16, 16
    X, Y, m = nt.linear_dataset(n, dim, D)
    noise = (Y.astype(np.float64) - X.astype(np.float64) @ m) / 2.0**D
    assert abs(noise.mean() - 1) < 0.05
    assert abs(noise.std() - 1) < 0.05
