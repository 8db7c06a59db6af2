"""The streaming skinny share product (aby3_amd/csrc/skinny.hip) behind
aby3g_mul_local / aby3g_mul_trunc_local / aby3g_mul_sub_local: against numpy
uint64 arithmetic, and byte for byte against the kernels it replaces
(aby3g_skinny_route(1)) on the same inputs. The shapes are the smallest at
which the kernels can go wrong: rows around a wave's 16-row batch, K around the
16-lane group's 16 / 32-term step and odd (8-byte loads), every column count's
edge, the long form's split edges, and one shape just beyond each threshold of
the automatic route."""
import ctypes
import functools

import numpy as np
import pytest

import oracle as orc
from aby3_amd import native as nt

pytestmark = pytest.mark.gpu

GEMM = nt.MUL_GEMM
AUTO, NEVER, ALWAYS = 0, 1, 2
SMALL_TERMS = 2**23   # k_small_gemm's range (gemm.hip)
MAX_N = 8             # kSkinnyMaxN
LONG_MIN_K = 2**14    # the long form's smallest K (auto takes it from there)
TALL_LDS_TERMS = 2048  # auto: the tall form only while K N fits the LDS image of B
LONG_MAX_OUT = 1024   # the long form's largest M N
LONG_CHUNK = 512      # the long form's K chunk granule

_KEEP = []


@pytest.fixture(autouse=True)
def _release(gpu):
    try:
        yield
    finally:
        gpu.skinny_route(AUTO)
        _KEEP.clear()


def dev(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda")
    _KEEP.append(t)
    return t


def empty(n):
    import torch

    return torch.zeros(max(n, 1), dtype=torch.int64, device="cuda")


def host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def rnd(seed, n):
    return np.random.default_rng(seed).integers(-(2**63), 2**63 - 1, size=n, dtype=np.int64, endpoint=True)


def corners(seed, n):
    vals = np.array([-(2**63), -1, 2**63 - 1], dtype=np.int64)
    return vals[np.random.default_rng(seed).integers(0, 3, n)]


def product(A, B, M, K, N):
    """C0 = A0 (B0 + B1) + A1 B0 mod 2^64 in numpy uint64."""
    a0, a1 = A[:M * K].view(np.uint64).reshape(M, K), A[M * K:].view(np.uint64).reshape(M, K)
    b0, b1 = B[:K * N].view(np.uint64).reshape(K, N), B[K * N:].view(np.uint64).reshape(K, N)
    return (a0 @ (b0 + b1) + a1 @ b0).reshape(-1)


KP, KN, NS, PS = (bytes(np.random.default_rng(s).integers(0, 256, size=16, dtype=np.uint8)) for s in (6, 7, 13, 14))
ZS_BASE, NOFF, POFF = 77, 32, 40
TRUNC_D = (8, 27)


@functools.lru_cache(maxsize=None)
def randomness(n):
    """The zero-share draws and truncation pairs of n elements (oracle), shared by every case of that size."""
    zs = orc.share_draws(0, KP, KN, ZS_BASE, n)[0].view(np.uint64)
    return zs, {d: orc.trunc_tuple(NS, NOFF, PS, POFF, n, d) for d in TRUNC_D}


def _zs():
    z = nt.ZeroShare()
    z.k_prev[:] = KP
    z.k_next[:] = KN
    z.draw_base = ZS_BASE
    return z


def _ts():
    t = nt.TruncStreams()
    t.next_seed[:] = NS
    t.next_off = NOFF
    t.prev_seed[:] = PS
    t.prev_off = POFF
    return t


def run_ops(gpu, route, A, B, sub, M, K, N, a_word_offset=0):
    """The five local products under `route`; returns their outputs by name."""
    gpu.skinny_route(route)
    n = M * N
    ws_bytes = gpu.dll.aby3g_mul_workspace_bytes(GEMM, M, K, N)
    ws = empty(ws_bytes // 8)
    dA = dev(np.concatenate([np.zeros(a_word_offset, dtype=np.int64), A]))
    assert dA.data_ptr() % 16 == 0
    pA = ctypes.c_void_p(dA.data_ptr() + 8 * a_word_offset)
    dB, dS = dev(B), dev(sub)
    out = {}
    C0 = empty(n)
    gpu.mul_local(GEMM, pA, P(dB), P(C0), M, K, N, None, P(ws), ws_bytes, None)
    out["mul"] = host(C0).view(np.uint64)
    C0 = empty(n)
    gpu.mul_local(GEMM, pA, P(dB), P(C0), M, K, N, ctypes.byref(_zs()), P(ws), ws_bytes, None)
    out["mul_zs"] = host(C0).view(np.uint64)
    for d in TRUNC_D:
        z, C = empty(n), empty(2 * n)
        gpu.mul_trunc_local(GEMM, pA, P(dB), M, K, N, d, ctypes.byref(_ts()), P(z), P(C), P(ws), ws_bytes, None)
        out[f"trunc{d}_z"] = host(z).view(np.uint64)
        out[f"trunc{d}_C"] = host(C)[:2 * n]
    o = empty(n)
    gpu.mul_sub_local(GEMM, pA, P(dB), P(dS), None, P(o), M, K, N, P(ws), ws_bytes, None)
    out["sub"] = host(o).view(np.uint64)
    return out, ws_bytes


def expected(A, B, sub, M, K, N):
    prod = product(A, B, M, K, N)
    zs, tr = randomness(M * N)
    exp = {"mul": prod, "mul_zs": prod + zs, "sub": prod - sub.view(np.uint64)}
    for d in TRUNC_D:
        R, RT0, RT1 = tr[d]
        exp[f"trunc{d}_z"] = prod - R.view(np.uint64)
        exp[f"trunc{d}_C"] = np.concatenate([RT0, RT1])
    return exp


def check_shape(gpu, M, K, N, route=ALWAYS, gen=rnd, a_word_offset=0):
    A, B, sub = gen(1000 + M + K, 2 * M * K), gen(2000 + K + N, 2 * K * N), gen(3000 + M, M * N)
    exp = expected(A, B, sub, M, K, N)
    new, ws_new = run_ops(gpu, route, A, B, sub, M, K, N, a_word_offset)
    old, _ = run_ops(gpu, NEVER, A, B, sub, M, K, N, a_word_offset)
    for name, e in exp.items():
        assert np.array_equal(new[name], e), f"{name}: the skinny route differs from numpy"
        assert new[name].tobytes() == old[name].tobytes(), f"{name}: the routes differ"
    return ws_new


@pytest.mark.parametrize("N", [1, 3, 8])
@pytest.mark.parametrize("K", [1, 2, 3, 127, 128, 129, 257])
@pytest.mark.parametrize("M", [1, 63, 65, 1000])
def test_tall(gpu, M, K, N):
    assert check_shape(gpu, M, K, N) == 0  # the tall form writes nothing but the product


def test_tall_corner_values(gpu):
    """INT64_MIN, -1 and INT64_MAX in both operands."""
    check_shape(gpu, 65, 129, 3, gen=corners)
    check_shape(gpu, 63, 128, 8, gen=corners)


@pytest.mark.parametrize("M,K,N", [(65, 128, 3), (63, 257, 1)])
def test_tall_a_offset_one_word(gpu, M, K, N):
    """A handed over one i64 word into its buffer: rows only 8-byte aligned."""
    check_shape(gpu, M, K, N, a_word_offset=1)


@pytest.mark.parametrize("K", [1025, 1026])
def test_tall_b_beyond_lds(gpu, K):
    """K N past the LDS image of (B0 + B1, B0): B is read through L2, with
    8-byte (odd K) and with 16-byte loads of A (even K)."""
    check_shape(gpu, 17, K, 3)


def _splits(ws_bytes, M, N):
    assert ws_bytes % (8 * M * N) == 0
    return ws_bytes // (8 * M * N)


@pytest.mark.parametrize("M,K,N", [(1, 20000, 1), (3, 16385, 2), (1, 33 * LONG_CHUNK + 1, 1)])
def test_long(gpu, M, K, N):
    """A plain long dot; a K the split does not divide; a last chunk of one term."""
    ws = check_shape(gpu, M, K, N)
    s = _splits(ws, M, N)
    assert s > 1, "the long form splits K into slabs"
    chunk = -(-K // s)
    chunk = -(-chunk // LONG_CHUNK) * LONG_CHUNK
    assert (s - 1) * chunk < K <= s * chunk
    if K % LONG_CHUNK == 1:
        assert K - (s - 1) * chunk == 1, "the last chunk holds a single term"


def test_long_corner_values_and_offset(gpu):
    check_shape(gpu, 2, 16386, 1, gen=corners)
    check_shape(gpu, 1, 16384, 2, a_word_offset=1)


def test_auto_just_beyond_small_gemm_takes_tall(gpu):
    M, K, N = 8193, 128, MAX_N
    assert (M - 1) * K * N == SMALL_TERMS < M * K * N
    gpu.skinny_route(AUTO)
    assert gpu.dll.aby3g_mul_prefers_fused(GEMM, M, K, N) == 1
    assert gpu.dll.aby3g_mul_workspace_bytes(GEMM, M, K, N) == 0
    # one row fewer, or one column more, stays on today's kernels
    assert gpu.dll.aby3g_mul_workspace_bytes(GEMM, M - 1, K, N) == 0
    assert gpu.dll.aby3g_mul_prefers_fused(GEMM, M, K, N + 1) == 0
    gpu.skinny_route(NEVER)
    assert gpu.dll.aby3g_mul_prefers_fused(GEMM, M, K, N) == 0
    assert gpu.dll.aby3g_mul_workspace_bytes(GEMM, M, K, N) > 0
    check_shape(gpu, M, K, N, route=AUTO)


def test_auto_tall_lds_threshold(gpu):
    """Beyond 2^23 terms the automatic route takes the tall form only while
    K N fits the LDS image of B; one K further it keeps the MFMA path."""
    M, K, N = 4097, TALL_LDS_TERMS // MAX_N, MAX_N
    assert M * K * N > SMALL_TERMS
    gpu.skinny_route(AUTO)
    assert gpu.dll.aby3g_mul_prefers_fused(GEMM, M, K, N) == 1
    assert gpu.dll.aby3g_mul_workspace_bytes(GEMM, M, K, N) == 0
    assert gpu.dll.aby3g_mul_prefers_fused(GEMM, M, K + 1, N) == 0
    check_shape(gpu, M, K, N, route=AUTO)


def test_auto_long_threshold(gpu):
    M, K, N = 1, LONG_MIN_K, 1
    gpu.skinny_route(AUTO)
    assert gpu.dll.aby3g_mul_workspace_bytes(GEMM, M, K - 1, N) == 0, "below the threshold: k_small_gemm"
    ws = gpu.dll.aby3g_mul_workspace_bytes(GEMM, M, K, N)
    assert _splits(ws, M, N) == K // LONG_CHUNK
    assert gpu.dll.aby3g_mul_prefers_fused(GEMM, M, K, N) == 1
    assert check_shape(gpu, M, K, N, route=AUTO) == ws


def test_auto_long_output_bound(gpu):
    """M N = 1024 outputs, the long form's upper bound, beyond k_small_gemm's
    range: the automatic route moves this MFMA-sized product onto the long
    kernel (32 row blocks of 4 rows); one output more keeps the MFMA path."""
    M, K, N = 128, LONG_MIN_K, MAX_N
    assert M * N == LONG_MAX_OUT and M * K * N > SMALL_TERMS
    gpu.skinny_route(AUTO)
    ws = gpu.dll.aby3g_mul_workspace_bytes(GEMM, M, K, N)
    assert _splits(ws, M, N) == K // LONG_CHUNK, "long: one slab per chunk"
    assert gpu.dll.aby3g_mul_prefers_fused(GEMM, M, K, N) == 1
    assert gpu.dll.aby3g_mul_prefers_fused(GEMM, LONG_MAX_OUT + 1, K, 1) == 0, "1025 outputs: the MFMA path"
    gpu.skinny_route(NEVER)
    assert gpu.dll.aby3g_mul_prefers_fused(GEMM, M, K, N) == 0
    assert check_shape(gpu, M, K, N, route=AUTO) == ws


@pytest.mark.parametrize("M,K,N", [(7, 16384, 1), (5, 16385, 3), (9, 16386, 8)])
def test_long_several_row_blocks(gpu, M, K, N):
    """More than kLongRows = 4 rows, not a multiple of it: several row blocks,
    the last one clamped and partly stored."""
    ws = check_shape(gpu, M, K, N)
    assert _splits(ws, M, N) > 1


def test_workspace_too_small_is_rejected(gpu):
    M, K, N = 1, 20000, 1
    gpu.skinny_route(ALWAYS)
    ws_bytes = gpu.dll.aby3g_mul_workspace_bytes(GEMM, M, K, N)
    A, B, C0, ws = dev(rnd(1, 2 * M * K)), dev(rnd(2, 2 * K * N)), empty(1), empty(ws_bytes // 8)
    with pytest.raises(nt.NativeError):
        gpu.mul_local(GEMM, P(A), P(B), P(C0), M, K, N, None, P(ws), ws_bytes - 8, None)


def test_route_rejects_unknown_mode(gpu):
    with pytest.raises(nt.NativeError):
        gpu.skinny_route(3)
