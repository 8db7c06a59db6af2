// SGD_Linear (aby3-ML/Regression.h:111-185) as a whole -- the DeviceBatchSampler
// batches, sgdLinearStep per iteration and test_linearModel's score at
// i % 1000 == 0 -- on the aby3ML seeds (aby3ML.cpp:4-17), share for share
// against the same computation assembled from the CPU oracle's shareInt /
// mulTrunc. The oracle has no linear iteration of its own; the one here
// follows Regression.h:145-168 and :94-107.
#include <cmath>
#include "aby3ML.h"
#include "harness.h"

using namespace aby3;
using namespace harness;

// three party threads on `device`, seeded as aby3ML::init
static void run3ml(const std::function<void(Sh3Runtime&, Sh3Encryptor&, Sh3Evaluator&, int)>& f, int device = 0) {
    auto comms = makeLocalRing();
    std::exception_ptr err[3];
    std::thread th[3];
    for (int i = 0; i < 3; ++i)
        th[i] = std::thread([&, i] {
            try {
                Sh3Runtime rt;
                Sh3Encryptor enc;
                Sh3Evaluator eval;
                rt.init(i, comms[i], device);
                const MlSeeds ms = mlSeeds(i);
                enc.init(i, ms.encPrev, ms.encNext);
                eval.init(i, ms.evalPrev, ms.evalNext);
                f(rt, enc, eval, i);
                rt.gpu().sync();
            } catch (...) {
                err[i] = std::current_exception();
            }
        });
    for (auto& t : th) t.join();
    for (auto& e : err)
        if (e) std::rethrow_exception(e);
}

static void shareIn(Sh3Runtime& rt, Sh3Encryptor& enc, int p, const i64Matrix& m, si64Matrix& dest) {
    if (p == 0)
        enc.localIntMatrix(rt, m, dest).get();
    else
        enc.remoteIntMatrix(rt, dest).get();
}

static orc::Shared sub(const orc::Shared& a, const orc::Shared& b) {
    orc::Shared r = a;
    for (int p = 0; p < 3; ++p)
        for (int s = 0; s < 2; ++s)
            for (u64 i = 0; i < r[p].s[s].v.size(); ++i)
                r[p].s[s].v[i] = (i64)((u64)a[p].s[s].v[i] - (u64)b[p].s[s].v[i]);
    return r;
}

// the same values seen as rows x cols (a column's transpose)
static orc::Shared reshaped(const orc::Shared& a, u64 rows, u64 cols) {
    orc::Shared r = a;
    for (int p = 0; p < 3; ++p)
        for (int s = 0; s < 2; ++s) {
            r[p].s[s].rows = rows;
            r[p].s[s].cols = cols;
        }
    return r;
}

static void sgdLinearWhole(u64 n, u64 d, u64 B, u64 iters, u64 nTest) {
    const u64 D = 16;
    RegressionParam params;
    params.mIterations = iters;
    params.mBatchSize = B;
    params.mLearningRate = 1.0 / (1 << 10);  // main-linear.cpp:59
    const u64 aB = (u64)std::log2(1 / (params.mLearningRate / (double)B));
    i64Matrix X, Y, Xt, Yt, w0(d, 1);
    linearModelGen(logisticModel(d), n, D, X, Y);
    linearModelGen(logisticModel(d), nTest, D, Xt, Yt);  // the reference's test set: the training set's head
    ShareSink got;
    std::vector<double> scores[3];
    run3ml([&](Sh3Runtime& rt, Sh3Encryptor& enc, Sh3Evaluator& eval, int p) {
        si64Matrix sX(n, d), sY(n, 1), sW(d, 1), sXt(nTest, d), sYt(nTest, 1);
        shareIn(rt, enc, p, X, sX);
        shareIn(rt, enc, p, Y, sY);
        shareIn(rt, enc, p, w0, sW);
        shareIn(rt, enc, p, Xt, sXt);
        shareIn(rt, enc, p, Yt, sYt);
        aby3ML ml(rt, enc, eval, D);
        RegressionParam prm = params;
        SGD_Linear(prm, ml, sX, sY, sW, &sXt, &sYt, &scores[p]);
        got.put(p, sW);
    });
    // the same computation on the oracle's primitives
    std::array<orc::Party, 3> enc, ev;
    orc::mlParties(enc, ev);
    orc::Shared oX = orc::shareInt(enc, 0, toOrc(X)), oY = orc::shareInt(enc, 0, toOrc(Y));
    orc::Shared oW = orc::shareInt(enc, 0, orc::Mat(d, 1));
    orc::Shared oXt = orc::shareInt(enc, 0, toOrc(Xt)), oYt = orc::shareInt(enc, 0, toOrc(Yt));
    orc::BatchSampler sampler(n);
    std::vector<u64> batch(B);
    std::vector<double> expScores;
    for (u64 t = 0; t < iters; ++t) {
        sampler.next(batch);
        orc::Shared XX, YY, XXt;
        for (int p = 0; p < 3; ++p) {
            XX[p] = orc::SMat(B, d);
            YY[p] = orc::SMat(B, 1);
            XXt[p] = orc::SMat(d, B);
            for (int s = 0; s < 2; ++s)
                for (u64 i = 0; i < B; ++i) {  // extractBatch (Regression.h:42-58)
                    for (u64 j = 0; j < d; ++j) {
                        XX[p].s[s].v[i * d + j] = oX[p].s[s].v[batch[i] * d + j];
                        XXt[p].s[s].v[j * B + i] = oX[p].s[s].v[batch[i] * d + j];
                    }
                    YY[p].s[s].v[i] = oY[p].s[s].v[batch[i]];
                }
        }
        orc::Shared err = sub(orc::mulTrunc(ev, orc::MUL_GEMM, XX, oW, D), YY);
        oW = sub(oW, orc::mulTrunc(ev, orc::MUL_GEMM, XXt, err, D + aB));
        if (t % 1000 == 0) {  // test_linearModel (Regression.h:94-107)
            orc::Shared e = sub(orc::mulTrunc(ev, orc::MUL_GEMM, oXt, oW, D), oYt);
            orc::Shared l2 = orc::mulTrunc(ev, orc::MUL_GEMM, reshaped(e, 1, nTest), e, D);
            expScores.push_back((double)orc::revealInt(l2).v[0] / (double)(1ull << D) / (double)nTest);
        }
    }
    got.expectEq(oW, "w after SGD_Linear");
    for (int p = 0; p < 3; ++p) check(scores[p] == expScores, "test_linearModel scores of party " + std::to_string(p));
    check(!expScores.empty() && expScores[0] > 0, "a score was taken");
}

int main() {
    test("sgd_linear_600x5_B64_x3_scored", [] { sgdLinearWhole(600, 5, 64, 3, 100); });
    // a batch across a reshuffle (B does not divide n), one feature
    test("sgd_linear_50x1_B7_x9_scored", [] { sgdLinearWhole(50, 1, 7, 9, 50); });
    test("sgd_linear_300x128_B32_x2_scored", [] { sgdLinearWhole(300, 128, 32, 2, 33); });
    return g_failures ? 1 : 0;
}
