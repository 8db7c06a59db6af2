// Host-runtime memory-safety driver for the linear-regression / model-score
// entry points (aby3h_sim_linear, aby3h_sim_model_score, aby3h_linear_dataset),
// linked against the null device (gen_nulldev.py) and built with
// -fsanitize=address by tests/test_host_asan_linear.py. Compute results are
// meaningless here; only the host code's memory behaviour is under test --
// among it the borrowed view of a column as its own transpose
// (SharedMat::viewOf) and the score outputs.
#include <aby3.h>
#include <cstdio>
#include <vector>

static int fail(const char* what) {
    std::printf("FAIL %s: %s\n", what, aby3h_sim_last_error());
    return 1;
}

int main() {
    const uint64_t n = 300, d = 7, B = 32, iters = 3, D = 16;
    std::vector<int64_t> X(n * d), Y(n), w(d, 1 << 14), wsh(6 * d), wpl(d);
    std::vector<double> model(d);
    if (aby3h_linear_dataset(n, d, D, X.data(), Y.data(), model.data())) return fail("linear_dataset");
    if (aby3h_linear_dataset(n, d, D, nullptr, nullptr, model.data())) return fail("linear_dataset (model only)");
    std::vector<uint64_t> batches(iters * B);
    if (aby3h_lr_batches(n, B, iters, batches.data())) return fail("lr_batches");
    if (aby3h_sim_linear(0, n, d, B, D, 15, iters, X.data(), Y.data(), batches.data(), wsh.data(), wpl.data()))
        return fail("sim_linear");
    // B = 1, d = 1
    if (aby3h_sim_linear(0, n, 1, 1, D, 10, 2, X.data(), Y.data(), batches.data(), wsh.data(), wpl.data()))
        return fail("sim_linear (B = 1, d = 1)");
    batches[0] = n;  // out of range: refused
    if (!aby3h_sim_linear(0, n, d, B, D, 15, iters, X.data(), Y.data(), batches.data(), wsh.data(), wpl.data())) {
        std::printf("FAIL a batch index past the dataset was accepted\n");
        return 1;
    }
    std::vector<int64_t> psh(6 * n), ppl(n), lsh(6);
    double score[2];
    for (int kind = 0; kind < 2; ++kind) {
        if (aby3h_sim_model_score(0, kind, n, d, D, X.data(), Y.data(), w.data(), psh.data(), ppl.data(), lsh.data(),
                                  score))
            return fail("sim_model_score");
        // every output optional
        if (aby3h_sim_model_score(0, kind, n, d, D, X.data(), Y.data(), w.data(), nullptr, nullptr, nullptr, nullptr))
            return fail("sim_model_score (no outputs)");
    }
    if (!aby3h_sim_model_score(0, 2, n, d, D, X.data(), Y.data(), w.data(), nullptr, nullptr, nullptr, nullptr)) {
        std::printf("FAIL an unknown model kind was accepted\n");
        return 1;
    }
    std::printf("linear_asan: ok\n");
    return 0;
}
