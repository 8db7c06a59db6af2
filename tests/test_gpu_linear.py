"""aby3-ML linear regression, model scoring and prediction on shares
(native.sim.linear / native.sim.model_score) against the numpy restatement of
tests/ml_restate.py, share for share, on the kernels in use before the skinny
route (aby3g_skinny_route(1)) and on the skinny kernels (route 2)."""
import numpy as np
import pytest

import ml_restate as mr
from aby3_amd import native as nt

pytestmark = pytest.mark.gpu

ROUTES = [1, 2]


@pytest.fixture
def route(gpu, request):
    gpu.skinny_route(request.param)
    try:
        yield request.param
    finally:
        gpu.skinny_route(0)


@pytest.mark.parametrize("route", ROUTES, indirect=True)
@pytest.mark.parametrize("name", list(mr.LINEAR_CASES))
def test_sim_linear_matches_restatement(gpu, route, name):
    c = mr.LINEAR_CASES[name]
    X, Y, batches = mr.linear_inputs(name)
    esh, ew, _ = mr.linear_expected(name)
    sh, w = nt.sim.linear(X, Y, batches, D=mr.D, aB=c["aB"])
    assert np.array_equal(sh, esh)
    assert np.array_equal(w, ew)
    assert ew.any(), "the iterations moved w"


@pytest.mark.parametrize("route", ROUTES, indirect=True)
@pytest.mark.parametrize("name", list(mr.SCORE_CASES))
def test_model_score_linear_matches_restatement(gpu, route, name):
    X, Y, w = mr.score_inputs(name)
    exp, _ = mr.score_expected(name)
    got = nt.sim.model_score(0, X, Y, w, D=mr.D)
    assert np.array_equal(got["pred_shares"], exp["pred_shares"])
    assert np.array_equal(got["pred"], exp["pred"])
    assert np.array_equal(got["l2_shares"], exp["l2_shares"])
    l2 = mr.reveal(got["l2_shares"])
    assert got["score"][0] == float(l2[0]) / 2.0**mr.D / len(Y)
    assert got["score"][0] == exp["score"]
    assert got["score"][1] == 0


@pytest.mark.parametrize("route", ROUTES, indirect=True)
def test_model_score_logistic(gpu, route):
    X, Y, w = mr.logistic_inputs()
    n, D = len(Y), mr.D
    # the same seeds and input order: kind 0's prediction is kind 1's x w
    lin = nt.sim.model_score(0, X, Y, w, D=D)
    exp, _ = mr.logistic_expected()
    assert np.array_equal(lin["pred_shares"], exp["pred_shares"])
    assert np.array_equal(lin["pred"], exp["pred"])
    assert np.array_equal(lin["l2_shares"], exp["l2_shares"])
    xw = exp["pred"]
    got = nt.sim.model_score(1, X, Y, w, D=D)
    # f = 0 | 0.5 + x | 1 with thresholds -0.5 / 0.5, on the revealed x w
    f = np.clip(xw + 2 ** (D - 1), 0, 2**D)
    assert np.array_equal(got["pred"], f)
    assert np.array_equal(mr.reveal(got["pred_shares"]), f)
    assert len({0, 2**D} & set(f.tolist())) == 2 and ((f > 0) & (f < 2**D)).any(), "all three regions"
    # accuracy: reveal(fxw) > 0.5 agrees with reveal(y) > 0.5
    acc = np.count_nonzero((f / 2.0**D > 0.5) == (Y / 2.0**D > 0.5)) / n
    assert got["score"][1] == acc
    # l2 = mulTrunc(err^T, err) of the revealed error, within the truncation bound
    err = (f - Y).astype(object)
    lo, hi = mr.trunc_bounds([int(err.dot(err))], D)
    l2 = int(mr.reveal(got["l2_shares"])[0])
    assert lo[0] <= l2 <= hi[0]
    assert got["score"][0] == float(l2) / 2.0**D / n
