// Streaming skinny share product on gfx950: the GEMM-mode C0 part
//   out[m][c] = sum_k A0[m][k] (B0[k][c] + B1[k][c]) + A1[m][k] B0[k][c]   (mod 2^64)
// for N <= kSkinnyMaxN columns. A tall share matrix times a few share columns
// is memory-bound arithmetic mod 2^64: it needs one pass over A. k_small_gemm
// gives such a product one wave per output element (a 1 x 10^6 x 1 dot is one
// wave walking 10^6 terms) and the int8-digit MFMA GEMM writes and re-reads a
// digit image of A and spends a 128 x 64 tile on the few useful columns. Here
// every byte of A is read once, on the VALU, and nothing is written but the
// product (tall) or its split-K slabs (long).
//
// Tall (many rows): a 16-lane group owns kTallRows rows at a time, its lanes
// split K in 16-byte pieces (256 contiguous bytes of a row per load
// instruction and group) and a 4-step butterfly sums them; every lane keeps
// kTallRows rows x 2 shares = 8 loads of 16 B in flight, 8 KiB per wave.
// (B0 + B1, B0) is combined once per workgroup into LDS when it fits
// (kTallLdsTerms), else read through L2.
//
// Long (M N small, K huge): K is cut into chunks, one workgroup per chunk and
// kLongRows rows; its 256 threads split the chunk, a butterfly and a 4-wave
// LDS sum reduce it, and the partial M x N slab goes to the caller's
// workspace, where the epilogues' SrcSlabs / SrcSlabsMinus sum the slabs in
// their own pass. No atomics, no tickets, no workgroup waits on another:
// addition mod 2^64 makes any order bit-identical.
//
// Rows are only 8-byte aligned when K is odd or A sits at an odd word: those
// products take the same kernels with 8-byte loads (W = 1).
#include <atomic>
#include "skinny.h"

namespace aby3g {

namespace {

typedef u64 u64x2 __attribute__((ext_vector_type(2)));

constexpr u32 kTallRows = 4;           // rows in flight per 16-lane group
constexpr u32 kTallWaveRows = 4 * kTallRows;
constexpr u64 kTallLdsTerms = 2048;    // K * N up to which (B0 + B1, B0) sits in LDS (32 KiB)
constexpr u32 kLongRows = 4;           // rows per long workgroup
constexpr u64 kLongChunk = 512;        // long: K chunk granule (256 threads x 16 B)
constexpr u32 kLongMaxSplits = 256;

// The long form is the skinny form of products of at least kLongMinK terms
// per output and at most kLongMaxOut outputs. The automatic route takes it
// wherever it is defined (measured ahead of k_small_gemm and of the MFMA path
// at every such shape), and the tall form only beyond
// k_small_gemm's range and with B in LDS. kTallLdsTerms is the LDS image's
// size, not a measured crossover: past it only 4096 x 4096 x 8 (K N = 32768,
// few rows) was measured, and lost to the MFMA path; products with
// K N > kTallLdsTerms and many rows are unmeasured and stay, conservatively,
// on the MFMA path.
constexpr u64 kLongMinK = 1ull << 14;
constexpr u64 kLongMaxOut = 1024;

std::atomic<int>& route_mode() {
    static std::atomic<int> m{0};
    return m;
}

template <u32 W>
__device__ __forceinline__ void load_terms(const i64* __restrict__ p, u64 (&v)[W]) {
    if constexpr (W == 2) {
        const u64x2 x = *reinterpret_cast<const u64x2*>(p);
        v[0] = x.x;
        v[1] = x.y;
    } else {
        v[0] = (u64)p[0];
    }
}

// W terms k .. k + W - 1 of every column: bs = B0 + B1, bb = B0
template <u32 N, u32 W, bool LDSB>
__device__ __forceinline__ void load_b(const u64* sb, u64 KN, const i64* __restrict__ B0, const i64* __restrict__ B1,
                                       u64 k, u64 (&bs)[W][N], u64 (&bb)[W][N]) {
#pragma unroll
    for (u32 j = 0; j < W; ++j)
#pragma unroll
        for (u32 c = 0; c < N; ++c) {
            const u64 i = (k + j) * N + c;
            if constexpr (LDSB) {
                bs[j][c] = sb[i];
                bb[j][c] = sb[KN + i];
            } else {
                const u64 b0 = (u64)B0[i];
                bs[j][c] = b0 + (u64)B1[i];
                bb[j][c] = b0;
            }
        }
}

template <u32 N, u32 W, bool LDSB>
__global__ void __launch_bounds__(256) k_skinny_tall(const i64* __restrict__ A0, const i64* __restrict__ A1,
                                                     const i64* __restrict__ B0, const i64* __restrict__ B1, u64 M,
                                                     u64 K, i64* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) u64 sb[];  // [K][N] B0 + B1, then [K][N] B0
    const u64 KN = K * N;
    if constexpr (LDSB) {
        for (u64 i = threadIdx.x; i < KN; i += 256) {
            const u64 b0 = (u64)B0[i];
            sb[i] = b0 + (u64)B1[i];
            sb[KN + i] = b0;
        }
        __syncthreads();
    }
    const u32 lane = threadIdx.x & 63, sub = lane & 15, grp = lane >> 4;
    const u64 waves = (u64)gridDim.x * 4, wave = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    for (u64 r0 = wave * kTallWaveRows; r0 < M; r0 += waves * kTallWaveRows) {
        const u64 first = r0 + grp * kTallRows;  // this group's rows
        const i64 *p0[kTallRows], *p1[kTallRows];
#pragma unroll
        for (u32 r = 0; r < kTallRows; ++r) {
            // rows past the end re-read the last row (their sums are not stored)
            const u64 row = min(first + r, M - 1);
            p0[r] = A0 + row * K;
            p1[r] = A1 + row * K;
        }
        u64 acc[kTallRows][N];
#pragma unroll
        for (u32 r = 0; r < kTallRows; ++r)
#pragma unroll
            for (u32 c = 0; c < N; ++c) acc[r][c] = 0;
        for (u64 k = (u64)sub * W; k < K; k += 16 * W) {
            u64 a0[kTallRows][W], a1[kTallRows][W];
#pragma unroll
            for (u32 r = 0; r < kTallRows; ++r) {
                load_terms<W>(p0[r] + k, a0[r]);
                load_terms<W>(p1[r] + k, a1[r]);
            }
            u64 bs[W][N], bb[W][N];
            load_b<N, W, LDSB>(sb, KN, B0, B1, k, bs, bb);
#pragma unroll
            for (u32 r = 0; r < kTallRows; ++r)
#pragma unroll
                for (u32 j = 0; j < W; ++j)
#pragma unroll
                    for (u32 c = 0; c < N; ++c) acc[r][c] += a0[r][j] * bs[j][c] + a1[r][j] * bb[j][c];
        }
#pragma unroll
        for (u32 r = 0; r < kTallRows; ++r)
#pragma unroll
            for (u32 c = 0; c < N; ++c) {
                u64 v = acc[r][c];
#pragma unroll
                for (int o = 8; o; o >>= 1) v += __shfl_xor(v, o, 64);  // within the 16-lane group
                acc[r][c] = v;
            }
        if (sub == 0) {
#pragma unroll
            for (u32 r = 0; r < kTallRows; ++r)
                if (first + r < M) {
#pragma unroll
                    for (u32 c = 0; c < N; ++c) out[(first + r) * N + c] = (i64)acc[r][c];
                }
        }
    }
}

// grid (splits, ceil(M / kLongRows)): terms [x * kPerSplit, ..) of rows
// [y * kLongRows, ..) -> P[x][row][c]. kPerSplit is even, so with W = 2
// (K even) every thread's pair lies inside the chunk.
template <u32 N, u32 W>
__global__ void __launch_bounds__(256) k_skinny_long(const i64* __restrict__ A0, const i64* __restrict__ A1,
                                                     const i64* __restrict__ B0, const i64* __restrict__ B1, u64 M,
                                                     u64 K, u64 kPerSplit, i64* __restrict__ P) {
    __shared__ u64 red[4][kLongRows * N];
    const u64 k0 = (u64)blockIdx.x * kPerSplit, k1 = min(K, k0 + kPerSplit);
    const u64 first = (u64)blockIdx.y * kLongRows;
    const i64 *p0[kLongRows], *p1[kLongRows];
#pragma unroll
    for (u32 r = 0; r < kLongRows; ++r) {
        const u64 row = min(first + r, M - 1);
        p0[r] = A0 + row * K;
        p1[r] = A1 + row * K;
    }
    u64 acc[kLongRows][N];
#pragma unroll
    for (u32 r = 0; r < kLongRows; ++r)
#pragma unroll
        for (u32 c = 0; c < N; ++c) acc[r][c] = 0;
    for (u64 k = k0 + (u64)threadIdx.x * W; k < k1; k += 256 * W) {
        u64 a0[kLongRows][W], a1[kLongRows][W];
#pragma unroll
        for (u32 r = 0; r < kLongRows; ++r) {
            load_terms<W>(p0[r] + k, a0[r]);
            load_terms<W>(p1[r] + k, a1[r]);
        }
        u64 bs[W][N], bb[W][N];
        load_b<N, W, false>(nullptr, 0, B0, B1, k, bs, bb);
#pragma unroll
        for (u32 r = 0; r < kLongRows; ++r)
#pragma unroll
            for (u32 j = 0; j < W; ++j)
#pragma unroll
                for (u32 c = 0; c < N; ++c) acc[r][c] += a0[r][j] * bs[j][c] + a1[r][j] * bb[j][c];
    }
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (u32 r = 0; r < kLongRows; ++r)
#pragma unroll
        for (u32 c = 0; c < N; ++c) {
            u64 v = acc[r][c];
#pragma unroll
            for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0) red[wave][r * N + c] = v;
        }
    __syncthreads();
    if (threadIdx.x < kLongRows * N) {
        const u64 row = first + threadIdx.x / N, c = threadIdx.x % N;
        if (row < M)
            P[(u64)blockIdx.x * M * N + row * N + c] =
                (i64)(red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
    }
}

template <u32 N>
void launch_skinny(const SkinnyPlan& p, bool vec, const i64* A0, const i64* A1, const i64* B0, const i64* B1, u64 M,
                   u64 K, i64* out, hipStream_t s) {
    if (p.form == SKINNY_LONG) {
        const dim3 grid(p.splits, (u32)((M + kLongRows - 1) / kLongRows));
        if (vec)
            launch(PROBE_GEMM, k_skinny_long<N, 2>, grid, dim3(256), 0, s, A0, A1, B0, B1, M, K, p.kPerSplit, out);
        else
            launch(PROBE_GEMM, k_skinny_long<N, 1>, grid, dim3(256), 0, s, A0, A1, B0, B1, M, K, p.kPerSplit, out);
        return;
    }
    const dim3 grid((u32)std::min<u64>((M + 4 * kTallWaveRows - 1) / (4 * kTallWaveRows), 2048));
    const bool ldsb = K * N <= kTallLdsTerms;
    const size_t lds = ldsb ? K * N * 16 : 0;
    if (vec && ldsb)
        launch(PROBE_GEMM, k_skinny_tall<N, 2, true>, grid, dim3(256), lds, s, A0, A1, B0, B1, M, K, out);
    else if (vec)
        launch(PROBE_GEMM, k_skinny_tall<N, 2, false>, grid, dim3(256), lds, s, A0, A1, B0, B1, M, K, out);
    else if (ldsb)
        launch(PROBE_GEMM, k_skinny_tall<N, 1, true>, grid, dim3(256), lds, s, A0, A1, B0, B1, M, K, out);
    else
        launch(PROBE_GEMM, k_skinny_tall<N, 1, false>, grid, dim3(256), lds, s, A0, A1, B0, B1, M, K, out);
}

}  // namespace

SkinnyPlan plan_skinny(u64 M, u64 K, u64 N, bool small) {
    SkinnyPlan p;
    const int mode = route_mode().load(std::memory_order_relaxed);
    if (mode == 1 || !M || !K || !N || N > kSkinnyMaxN) return p;
    const bool lng = K >= kLongMinK && M * N <= kLongMaxOut;
    if (mode == 0 && !lng && (small || K * N > kTallLdsTerms)) return p;
    if (!lng) {
        p.form = SKINNY_TALL;
        return p;
    }
    p.form = SKINNY_LONG;
    // one chunk per workgroup, at most kLongMaxSplits of them, whole granules
    const u64 per = (K + kLongMaxSplits - 1) / kLongMaxSplits;
    p.kPerSplit = std::max<u64>(kLongChunk, (per + kLongChunk - 1) / kLongChunk * kLongChunk);
    p.splits = (u32)((K + p.kPerSplit - 1) / p.kPerSplit);
    p.bytes = (size_t)p.splits * M * N * 8;
    return p;
}

void run_skinny(const SkinnyPlan& p, const i64* A, const i64* B, u64 M, u64 K, u64 N, i64* out, hipStream_t s) {
    const i64 *A0 = A, *A1 = A + M * K, *B0 = B, *B1 = B + K * N;
    // 16-byte loads need 16-byte aligned rows in both shares
    const bool vec = K % 2 == 0 && ((uintptr_t)A & 15) == 0;
    switch (N) {
#define ABY3G_SKINNY_CASE(n) \
    case n:                  \
        return launch_skinny<n>(p, vec, A0, A1, B0, B1, M, K, out, s);
        ABY3G_SKINNY_CASE(1)
        ABY3G_SKINNY_CASE(2)
        ABY3G_SKINNY_CASE(3)
        ABY3G_SKINNY_CASE(4)
        ABY3G_SKINNY_CASE(5)
        ABY3G_SKINNY_CASE(6)
        ABY3G_SKINNY_CASE(7)
        ABY3G_SKINNY_CASE(8)
#undef ABY3G_SKINNY_CASE
        default:
            ABY3G_REQUIRE(false, "skinny product of more than kSkinnyMaxN columns");
    }
}

}  // namespace aby3g

using namespace aby3g;

extern "C" int aby3g_skinny_route(int mode) {
    return guarded([&] {
        ABY3G_REQUIRE(mode >= 0 && mode <= 2, "mode is 0 (auto), 1 (never) or 2 (always)");
        route_mode().store(mode);
    });
}
