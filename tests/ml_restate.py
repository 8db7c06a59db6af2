"""numpy restatement of the aby3-ML linear iteration and model score.

TEST INFRASTRUCTURE ONLY. The oracle has no linear iteration; this module
restates it from tests/oracle.py's primitives alone (prng_bytes, party_keys,
share_draws, local_product, trunc_tuple), line for line after
oracle/src/orc_core.cpp:110-119 (shareInt), :188-241 (mul, mulTrunc) and
oracle/src/orc_ml.cpp:105-118 (the aby3ML seeds). A value shared among the
three parties is an int64 array [party][share][n]; all sums are mod 2^64.
"""
from __future__ import annotations

import functools

import numpy as np

import oracle as orc
from aby3_amd.native import linear_dataset, lr_batches, lr_dataset

GEMM = 1


def _u(a):
    return np.ascontiguousarray(a, dtype=np.int64).view(np.uint64)


def _i(a):
    return np.ascontiguousarray(a).view(np.int64)


class Party:
    """One Sh3ShareGen: the prev / next PRNG streams at their byte offsets and
    the zero-share draw counter (orc_core.cpp:9-21, 82-91)."""

    def __init__(self, prev_seed: bytes, next_seed: bytes, evaluator: bool):
        self.prev_seed, self.next_seed = prev_seed, next_seed
        self.kprev, self.knext, _, _ = orc.party_keys(prev_seed, next_seed)
        self.draw = 0
        # ShareGen::init takes each stream's first block as a zero-share key;
        # Sh3Evaluator::init one more of each for the OT seeds
        self.prev_off = self.next_off = 32 if evaluator else 16

    def get_shares(self, n: int) -> np.ndarray:
        s, _ = orc.share_draws(0, self.kprev, self.knext, self.draw, n)
        self.draw += n
        return s


def unit_parties(c: int, evaluator: bool):
    """makeEncryptors / makeEvaluators (orc_core.cpp:93-102): seeds toBlock(c, i)."""
    return [Party(orc.to_block(c, i), orc.to_block(c, (i + 1) % 3), evaluator) for i in range(3)]


def ml_parties():
    """mlParties (orc_ml.cpp:105-118): PRNG(toBlock(i))'s first block seeds
    party i's encryptor, the second its evaluator; prev = party i - 1's."""
    es = [orc.prng_bytes(orc.to_block(0, i), 0, 16) for i in range(3)]
    vs = [orc.prng_bytes(orc.to_block(0, i), 16, 16) for i in range(3)]
    enc = [Party(es[(i + 2) % 3], es[i], False) for i in range(3)]
    ev = [Party(vs[(i + 2) % 3], vs[i], True) for i in range(3)]
    return enc, ev


def reshare_ring(x: np.ndarray) -> np.ndarray:
    for i in range(3):
        x[i, 1] = x[(i + 2) % 3, 0]
    return x


def share_int(enc, owner: int, m) -> np.ndarray:
    """shareInt (orc_core.cpp:110-119)."""
    m = np.ascontiguousarray(m, dtype=np.int64).reshape(-1)
    x = np.zeros((3, 2, m.size), dtype=np.int64)
    for i in range(3):
        s = _u(enc[i].get_shares(m.size))
        x[i, 0] = _i(s + _u(m)) if i == owner else _i(s)
    return reshare_ring(x)


def reveal(x: np.ndarray) -> np.ndarray:
    return _i(_u(x[0, 0]) + _u(x[1, 0]) + _u(x[2, 0]))


def _local(A, B, i, M, K, N):
    return orc.local_product(GEMM, A[i, 0], A[i, 1], B[i, 0], B[i, 1], M, K, N)


def mul(ev, A, B, M, K, N) -> np.ndarray:
    """mul (orc_core.cpp:188-198): C0 = local product + getShare, reshared."""
    C = np.zeros((3, 2, M * N), dtype=np.int64)
    for i in range(3):
        C[i, 0] = _i(_u(_local(A, B, i, M, K, N)) + _u(ev[i].get_shares(M * N)))
    return reshare_ring(C)


def mul_trunc(ev, A, B, M, K, N, d, log=None) -> np.ndarray:
    """mulTrunc (orc_core.cpp:200-241). log: a list that receives
    (revealed A, revealed B, revealed C, M, K, N, d) of this call."""
    n = M * N
    C = np.zeros((3, 2, n), dtype=np.int64)
    s = np.zeros(n, dtype=np.uint64)
    for i in range(3):
        p = ev[i]
        R, RT0, RT1 = orc.trunc_tuple(p.next_seed, p.next_off, p.prev_seed, p.prev_off, n, d)
        p.next_off += 8 * n
        p.prev_off += 8 * n
        s = s + (_u(_local(A, B, i, M, K, N)) - _u(R))
        C[i, 0], C[i, 1] = RT0, RT1
    t = _u(_i(s) >> d)
    C[0, 0] = _i(_u(C[0, 0]) + t)  # truncFinalize: parties 0 and 1 only
    C[1, 1] = _i(_u(C[1, 1]) + t)
    if log is not None:
        log.append((reveal(A), reveal(B), reveal(C), M, K, N, d))
    return C


def sub(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return _i(_u(a) - _u(b))


def sim_mul(trunc: bool, d: int, a, b, M, K, N):
    """orc.sim_mul's GEMM mode: unit-test seeds, party 0 shares a then b."""
    enc, ev = unit_parties(0, False), unit_parties(1, True)
    A, B = share_int(enc, 0, a), share_int(enc, 0, b)
    C = mul_trunc(ev, A, B, M, K, N, d) if trunc else mul(ev, A, B, M, K, N)
    return C, reveal(C)


def _rows(x: np.ndarray, cols: int, idx) -> np.ndarray:
    """extractBatch (Regression.h:42-58) on both shares of every party."""
    return np.ascontiguousarray(x.reshape(3, 2, -1, cols)[:, :, np.asarray(idx, dtype=np.int64), :])


def sim_linear(X, Y, batches, D: int, aB: int, log=None):
    """SGD_Linear iterations (Regression.h:145-168) with the aby3ML seeds, party
    0 sharing X, Y, w = 0 in that order. Returns (w shares [3][2][d], revealed w)."""
    X = np.ascontiguousarray(X, dtype=np.int64)
    n, d = X.shape
    enc, ev = ml_parties()
    sX, sY, sW = share_int(enc, 0, X), share_int(enc, 0, Y), share_int(enc, 0, np.zeros(d, np.int64))
    for batch in np.asarray(batches):
        B = len(batch)
        XX = _rows(sX, d, batch)                                   # [3][2][B][d]
        YY = _rows(sY, 1, batch).reshape(3, 2, B)
        XXt = np.ascontiguousarray(XX.transpose(0, 1, 3, 2)).reshape(3, 2, d * B)
        err = sub(mul_trunc(ev, XX.reshape(3, 2, B * d), sW, B, d, 1, D, log), YY)
        sW = sub(sW, mul_trunc(ev, XXt, err, d, B, 1, D + aB, log))
    return sW, reveal(sW)


def model_score_linear(X, Y, w, D: int, log=None):
    """test_linearModel (Regression.h:94-107) with the aby3ML seeds, party 0
    sharing X, Y, w in that order: dict(pred_shares, pred, l2_shares, l2, score)."""
    X = np.ascontiguousarray(X, dtype=np.int64)
    n, d = X.shape
    enc, ev = ml_parties()
    sX, sY, sW = share_int(enc, 0, X), share_int(enc, 0, Y), share_int(enc, 0, w)
    pred = mul_trunc(ev, sX, sW, n, d, 1, D, log)
    err = sub(pred, sY)
    l2 = mul_trunc(ev, err, err, 1, n, 1, D, log)  # err^T is err's own memory
    r = reveal(l2)
    return dict(pred_shares=pred, pred=reveal(pred), l2_shares=l2, l2=r, score=float(r[0]) / 2.0**D / n)


def exact_product(a, b, M, K, N):
    """The product of two int64 matrices in Python integers, [M * N]."""
    a = np.asarray(a, dtype=object).reshape(M, K)
    b = np.asarray(b, dtype=object).reshape(K, N)
    return a.dot(b).reshape(-1)


def trunc_bounds(x, d):
    """mulTrunc's revealed value of an exact product x with |x| < 2^61 lies in
    [floor(x / 2^d) - 3, floor(x / 2^d)]: it is the sum of four floored terms
    (three parties' r_i / 2^d and (x - r_0 - r_1 - r_2) / 2^d) that add up to
    x / 2^d, and |r_i| < 2^61 keeps x - r_0 - r_1 - r_2 inside int64."""
    f = np.asarray([int(v) >> d for v in x], dtype=object)
    return f - 3, f


# ---- the input sets the CPU and GPU tests share ----------------------------

D = 16
# aB = log2(B / rate) at the reference's rate 1 / 1024 (main-linear.cpp:59)
LINEAR_CASES = {
    "n600_d5_B64": dict(n=600, d=5, B=64, aB=16, iters=3),
    "n50_d1_B1": dict(n=50, d=1, B=1, aB=10, iters=2),
    "n300_d128_B32": dict(n=300, d=128, B=32, aB=15, iters=1),
}
SCORE_CASES = {"n300_d7": dict(n=300, d=7), "n2049_d128": dict(n=2049, d=128)}


@functools.lru_cache(maxsize=None)
def linear_inputs(name: str):
    """(X, Y, batches) of a LINEAR_CASES entry: the project's linear dataset
    and getSubset batches (host library, CPU only)."""
    c = LINEAR_CASES[name]
    X, Y, _ = linear_dataset(c["n"], c["d"], D)
    return X, Y, lr_batches(c["n"], c["B"], c["iters"])


@functools.lru_cache(maxsize=None)
def score_inputs(name: str):
    """(X, Y, w) of a SCORE_CASES entry: the linear dataset and a model a
    quarter off the true one in every coefficient, so the error is not noise alone."""
    c = SCORE_CASES[name]
    X, Y, m = linear_dataset(c["n"], c["d"], D)
    return X, Y, np.round((m + 0.25) * 2.0**D).astype(np.int64)


@functools.lru_cache(maxsize=None)
def logistic_inputs():
    """(X, Y, w) for the logistic score: the logistic dataset at n=300, d=7 and
    a model scaled so that x w falls in all three regions of the sigmoid."""
    X, Y, m = lr_dataset(300, 7, D)
    return X, Y, np.round(m * 0.05 * 2.0**D).astype(np.int64)


@functools.lru_cache(maxsize=None)
def logistic_expected():
    """(model_score_linear's dict, mulTrunc log) on logistic_inputs(): the
    linear score of the logistic input set, whose prediction is the x w that
    the logistic score feeds to the sigmoid (same seeds, same input order)."""
    X, Y, w = logistic_inputs()
    log = []
    return model_score_linear(X, Y, w, D, log), log


@functools.lru_cache(maxsize=None)
def linear_expected(name: str):
    """(w shares, revealed w, mulTrunc log) of the restatement on linear_inputs(name)."""
    c = LINEAR_CASES[name]
    X, Y, b = linear_inputs(name)
    log = []
    sh, w = sim_linear(X, Y, b, D, c["aB"], log)
    return sh, w, log


@functools.lru_cache(maxsize=None)
def score_expected(name: str):
    """(model_score_linear's dict, mulTrunc log) on score_inputs(name)."""
    X, Y, w = score_inputs(name)
    log = []
    return model_score_linear(X, Y, w, D, log), log
