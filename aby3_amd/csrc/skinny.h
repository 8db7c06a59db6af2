// The streaming skinny share product (skinny.hip): the GEMM-mode C0 part for
// N <= kSkinnyMaxN output columns, one pass over A on the VALU.
#pragma once
#include "common.h"

namespace aby3g {

constexpr u64 kSkinnyMaxN = 8;

enum SkinnyForm { SKINNY_NONE = 0, SKINNY_TALL = 1, SKINNY_LONG = 2 };

struct SkinnyPlan {
    int form = SKINNY_NONE;
    u32 splits = 1;     // long: K chunks, one partial M x N slab each
    u64 kPerSplit = 0;  // long: terms per chunk (a multiple of 512)
    size_t bytes = 0;   // workspace: the slabs [splits][M][N] (long), 0 (tall)
};

// The route of an M x K x N GEMM-mode product under the process-wide
// aby3g_skinny_route mode; `small` = the shape is inside k_small_gemm.
SkinnyPlan plan_skinny(u64 M, u64 K, u64 N, bool small);

// tall: out[M][N] = the product. long: P[splits][M][N] = the partial slabs.
void run_skinny(const SkinnyPlan& p, const i64* A, const i64* B, u64 M, u64 K, u64 N, i64* out, hipStream_t s);

}  // namespace aby3g
