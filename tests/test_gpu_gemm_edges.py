"""The share GEMM's MFMA path (aby3_amd/csrc/gemm.hip: k_digits +
k_share_gemm16s) at its digit, split-plan and `sub` edges, bit-exact against
the CPU oracle (all arithmetic is integer mod 2^64).

Every case meant for the MFMA path goes through `mfma_plan`, which asserts
that the shape is not sent to the VALU kernel (k_small_gemm) and recovers the
split-K factor plan_gemm chose from the workspace size, so a moved threshold
or a changed plan fails the case instead of quietly testing another kernel.
"""
import contextlib
import ctypes

import numpy as np
import pytest

import oracle as orc
from aby3_amd import native as nt

pytestmark = pytest.mark.gpu

GEMM = nt.MUL_GEMM

_KEEP = []  # device tensors whose pointers were handed to a kernel stay alive


@pytest.fixture(autouse=True)
def _release():
    yield
    _KEEP.clear()


def dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if not a.flags.writeable:  # the shared references are read-only; torch wants a writable source
        a = a.copy()
    t = torch.from_numpy(a.view(np.int64)).to("cuda")
    _KEEP.append(t)
    return t


def empty(n):
    import torch

    return torch.zeros(n, dtype=torch.int64, device="cuda")


def host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def rnd(seed, n):
    return np.random.default_rng(seed).integers(-(2**63), 2**63 - 1, size=n, dtype=np.int64, endpoint=True)


def k16(seed):
    return bytes(np.random.default_rng(seed).integers(0, 256, size=16, dtype=np.uint8))


def garbage(seed, n):
    """n non-zero words: an element a kernel leaves unwritten shows."""
    return rnd(seed, n) | np.int64(1)


def _zs(kp, kn, base):
    z = nt.ZeroShare()
    z.k_prev[:] = kp
    z.k_next[:] = kn
    z.draw_base = base
    return z


def _ts(ns, noff, ps, poff):
    t = nt.TruncStreams()
    t.next_seed[:] = ns
    t.next_off = noff
    t.prev_seed[:] = ps
    t.prev_off = poff
    return t


def _roundup(x, m):
    return (x + m - 1) // m * m


@contextlib.contextmanager
def sharing(gpu, parties):
    """aby3g_set_gemm_sharing for the block (thread-local), back to 1 after it."""
    gpu.set_gemm_sharing(parties)
    try:
        yield
    finally:
        gpu.set_gemm_sharing(1)


class Plan:
    def __init__(self, splits, TM, TN, stages, ws_bytes):
        self.splits, self.TM, self.TN, self.stages, self.ws_bytes = splits, TM, TN, stages, ws_bytes
        self.per_split = -(-stages // splits)  # K' stages per split
        self.last = stages - (splits - 1) * self.per_split  # stages of the last split

    def __repr__(self):
        return (f"splits {self.splits}, TM {self.TM} x TN {self.TN}, {self.stages} stages, "
                f"{self.per_split} per split, last {self.last}")


def mfma_plan(gpu, M, K, N):
    """The path guard. Asserts that M x K x N is not fused (it takes k_digits +
    k_share_gemm16s, not k_small_gemm) and returns the plan under the calling
    thread's GEMM sharing. The split count is read off the workspace size,
    which plan_gemm lays out as
      roundup(Mp*Kc*8, 256) + roundup(Np*Kc*8, 256) + roundup(splits*M*N*8, 256)
    with Mp, Np, Kp = M, N, K padded to 128, 64, 32 and Kc = 2 Kp: splits is the
    only power of two that fits."""
    assert gpu.dll.aby3g_mul_prefers_fused(GEMM, M, K, N) == 0, f"{M}x{K}x{N} runs k_small_gemm, not the MFMA path"
    Mp, Np, Kc = _roundup(M, 128), _roundup(N, 64), 2 * _roundup(K, 32)
    total = gpu.dll.aby3g_mul_workspace_bytes(GEMM, M, K, N)
    slabs = total - _roundup(Mp * Kc * 8, 256) - _roundup(Np * Kc * 8, 256)
    fits = [s for s in (1 << e for e in range(17)) if _roundup(s * M * N * 8, 256) == slabs]
    assert len(fits) == 1, f"{M}x{K}x{N}: workspace of {total} bytes fits split counts {fits}"
    plan = Plan(fits[0], Mp // 128, Np // 64, Kc // 32, total)
    print(f"plan {M}x{K}x{N}: {plan}")
    return plan


def expect_plan(plan, **want):
    got = {k: getattr(plan, k) for k in want}
    assert got == want, f"planned {plan}"


_REF = {}


def product(M, K, N, seed):
    """(A, B, local product) of a seeded random M x K x N share GEMM, computed
    once per session and read-only."""
    key = (M, K, N, seed)
    if key not in _REF:
        A, B = rnd(seed, 2 * M * K), rnd(seed + 1, 2 * K * N)
        exp = orc.local_product(GEMM, A[:M * K], A[M * K:], B[:K * N], B[K * N:], M, K, N)
        for x in (A, B, exp):
            x.setflags(write=False)
        _REF[key] = (A, B, exp)
    return _REF[key]


def gemm_oracle(A, B, M, K, N):
    return orc.local_product(GEMM, A[:M * K], A[M * K:], B[:K * N], B[K * N:], M, K, N)


def run_mul_local(gpu, plan, A, B, exp, M, K, N, with_zs=False, a_word_offset=0):
    """aby3g_mul_local on the MFMA path against `exp`; A is handed over
    a_word_offset int64 words into its device buffer."""
    n = M * N
    ws = empty(plan.ws_bytes // 8)
    C0 = dev(garbage(99, n + 1))
    dA = dev(np.concatenate([np.zeros(a_word_offset, dtype=np.int64), A]))[a_word_offset:]
    assert dA.data_ptr() % 16 == 8 * (a_word_offset % 2)
    zs = None
    if with_zs:
        kp, kn = k16(6), k16(7)
        zs = ctypes.byref(_zs(kp, kn, 77))
        exp = (exp.view(np.uint64) + orc.share_draws(0, kp, kn, 77, n)[0].view(np.uint64)).view(np.int64)
    gpu.mul_local(GEMM, P(dA), P(dev(B)), P(C0), M, K, N, zs, P(ws), plan.ws_bytes, None)
    got = host(C0)
    assert np.array_equal(got[:n], exp)
    assert got[n] == garbage(99, n + 1)[n], "wrote past the end of C0"


# The split plans of the issue's table, worked out from plan_gemm's rules
# (256 / sharing target workgroups, >= 8 stages per split, K' <= 8192 per split)
# and re-checked on the device by mfma_plan. tiles: TM x TN of 128 x 64.
CASES = {
    # odd K: k_digits' scalar A path with a K tail; M and N one past a tile; last split 3 of 9 stages
    "a": dict(sharing=1, shape=(129, 1031, 65), splits=8, TM=2, TN=2, per_split=9, last=3),
    # the last split has exactly one stage (nst == 1): the prologue re-issues stage 0
    "b": dict(sharing=1, shape=(100, 2150, 60), splits=16, TM=1, TN=1, per_split=9, last=1),
    # T = 24, a multiple of 8: tile_of's XCD bijection, with a partial second row-panel group (gm = 2 after 4)
    "c": dict(sharing=1, shape=(768, 64, 256), splits=1, TM=6, TN=4),
    # T = 40, gm = 1 after 4; K = 48 leaves half a stage of tail
    "d": dict(sharing=1, shape=(640, 48, 512), splits=1, TM=5, TN=8),
    # plan_gemm's second loop: one tile is enough work at sharing 256, the 8192 cap forces the split; odd K
    "e": dict(sharing=256, shape=(128, 4097, 64), splits=2, TM=1, TN=1, per_split=129, last=129),
    # the cap exactly: K' = 8192 in one split
    "f": dict(sharing=256, shape=(128, 4096, 64), splits=1, TM=1, TN=1, per_split=256),
    # the session's plan family (sharing 3) at a quarter of 1024^3's K: splits 1, where sharing 1 plans 2
    "g": dict(sharing=3, shape=(1024, 256, 1024), splits=1, TM=8, TN=16),
    # even K, but A starts 8 bytes past a 16-byte boundary: the aligned-pointer test of k_digits fails
    "h": dict(sharing=1, shape=(256, 130, 256), splits=1, TM=2, TN=4, a_word_offset=1),
}


def case_plan(gpu, name):
    """mfma_plan of a table case under the sharing set by the caller, checked against the table."""
    c = CASES[name]
    plan = mfma_plan(gpu, *c["shape"])
    expect_plan(plan, **{k: v for k, v in c.items() if k in ("splits", "TM", "TN", "per_split", "last")})
    return plan


@pytest.mark.parametrize("name,with_zs", [(c, z) for c in "abcdh" for z in (False, True)] +
                         [(c, False) for c in "efg"])
def test_mul_local_split_and_tile_edges(gpu, name, with_zs):
    c = CASES[name]
    M, K, N = c["shape"]
    A, B, exp = product(M, K, N, 100 + ord(name))
    if name == "g":
        expect_plan(mfma_plan(gpu, M, K, N), splits=2)  # at sharing 1
    with sharing(gpu, c["sharing"]):
        plan = case_plan(gpu, name)
        run_mul_local(gpu, plan, A, B, exp, M, K, N, with_zs, c.get("a_word_offset", 0))


# ---- digit corners on the MFMA path

ALL_M128 = 0x7F7F7F7F7F7F7F80  # every balanced digit is -128
ALL_P127 = 0x7F7F7F7F7F7F7F7F  # every balanced digit is +127
CORNERS = np.array([
    ALL_M128, ALL_P127, 0x8080808080808080, 2**64 - 1, 2**63, 2**63 - 1, 0, 1,
    # one borrow at byte 0, a borrow chain, and a borrow into the upper 32-bit half of digit_words
    0x0000000000000080, 0x00000000000000FF, 0x000000000000FF80, 0x0000008000000000], dtype=np.uint64).view(np.int64)


def _digits(x):
    """The 8 balanced base-256 digits of x (Python int, mod 2^64), as the header of gemm.hip defines them."""
    y = (x + 0x8080808080808080) % 2**64
    return [((y >> (8 * p)) & 0xFF) - 128 for p in range(8)]


def test_corner_values_are_the_digit_extremes():
    assert _digits(ALL_M128) == [-128] * 8 and _digits(ALL_P127) == [127] * 8
    for v in CORNERS.view(np.uint64):
        assert sum(d << (8 * p) for p, d in enumerate(_digits(int(v)))) % 2**64 == int(v)


@pytest.mark.parametrize("draw", ["independent", "b_sum_is_corner"])
def test_digit_corners_mfma(gpu, draw):
    """Operands drawn from the digit-carry corners through k_digits and the
    MFMA accumulators. B's first digit operand is B0 + B1: in the second draw
    B1 is chosen so that the sum is itself a corner value."""
    M, K, N = 192, 256, 192
    plan = mfma_plan(gpu, M, K, N)
    expect_plan(plan, splits=2, TM=2, TN=3)
    rng =np.random.default_rng(31 if draw == "independent" else 32)
    pick = lambda n: CORNERS[rng.integers(0, len(CORNERS), n)]  # noqa: E731
    A = pick(2 * M * K)
    B0 = pick(K * N)
    if draw == "independent":
        B1 = pick(K * N)
    else:
        B1 = (pick(K * N).view(np.uint64) - B0.view(np.uint64)).view(np.int64)
        assert np.isin(B0.view(np.uint64) + B1.view(np.uint64), CORNERS.view(np.uint64)).all()
    B = np.concatenate([B0, B1])
    run_mul_local(gpu, plan, A, B, gemm_oracle(A, B, M, K, N), M, K, N)


@pytest.mark.parametrize("b0", [ALL_M128, ALL_P127], ids=["all_minus128", "sign_mixed"])
def test_digit_worst_case_accumulators(gpu, b0):
    """Every digit of every operand at -128 (or B's at +127) over K' = 8192 in
    one split: plane s reaches (s+1) * 8192 * 2^14 in magnitude, the bound the
    header of gemm.hip states for exact i32 planes (2^30 at plane 7)."""
    M, K, N = CASES["f"]["shape"]
    A = np.full(2 * M * K, ALL_M128, dtype=np.int64)
    B = np.concatenate([np.full(K * N, b0, dtype=np.int64), np.zeros(K * N, dtype=np.int64)])
    exp = gemm_oracle(A, B, M, K, N)
    # a closed form of the same number: 2 K x0 b0 mod 2^64
    assert int(exp.view(np.uint64)[0]) == 2 * K * ALL_M128 * b0 % 2**64 and (exp == exp[0]).all()
    with sharing(gpu, CASES["f"]["sharing"]):
        plan = case_plan(gpu, "f")
        run_mul_local(gpu, plan, A, B, exp, M, K, N)


# ---- aby3g_mul_sub_local: out = local product - sub (sub_ready null)

def run_mul_sub(gpu, mode, A, B, exp, M, K, N, ws_bytes):
    n = M * N
    sub = rnd(55 + n, n)
    ws = empty(max(ws_bytes // 8, 1))
    out = dev(garbage(98, n + 1))
    gpu.mul_sub_local(mode, P(dev(A)), P(dev(B)), P(dev(sub)), None, P(out), M, K, N, P(ws), ws_bytes, None)
    got = host(out)
    assert np.array_equal(got[:n], (exp.view(np.uint64) - sub.view(np.uint64)).view(np.int64))
    assert got[n] == garbage(98, n + 1)[n], "wrote past the end of out"


@pytest.mark.parametrize("M,N", [(7, 3), (128, 128)])
def test_mul_sub_local_hadamard(gpu, M, N):
    n = M * N
    A, B = rnd(40 + M, 2 * n), rnd(41 + M, 2 * n)
    exp = orc.local_product(nt.MUL_HADAMARD, A[:n], A[n:], B[:n], B[n:], M, N, N)
    run_mul_sub(gpu, nt.MUL_HADAMARD, A, B, exp, M, N, N, 0)


def test_mul_sub_local_small_gemm(gpu):
    M, K, N = 33, 17, 65
    assert gpu.dll.aby3g_mul_prefers_fused(GEMM, M, K, N) == 1
    A, B, exp = product(M, K, N, 42)
    run_mul_sub(gpu, GEMM, A, B, exp, M, K, N, 0)


@pytest.mark.parametrize("name,shape,splits", [("257x200x250", (257, 200, 250), 1), ("c", None, 1), ("a", None, 8)])
def test_mul_sub_local_mfma(gpu, name, shape, splits):
    """One split: `sub` is applied in k_share_gemm16s's own epilogue; several:
    in the slab-reducing pass (SrcSlabsMinus)."""
    if shape is None:
        M, K, N = CASES[name]["shape"]
        plan = case_plan(gpu, name)
        A, B, exp = product(M, K, N, 100 + ord(name))
    else:
        M, K, N = shape
        plan = mfma_plan(gpu, M, K, N)
        A, B, exp = product(M, K, N, 43)
    expect_plan(plan, splits=splits)
    run_mul_sub(gpu, GEMM, A, B, exp, M, K, N, plan.ws_bytes)


@pytest.mark.parametrize("mode,M,K,N", [(nt.MUL_HADAMARD, 7, 3, 3), (GEMM, 33, 17, 65), (GEMM, 257, 200, 250)])
def test_mul_sub_local_rejects_null_sub(gpu, mode, M, K, N):
    ws_bytes = gpu.dll.aby3g_mul_workspace_bytes(mode, M, K, N)
    ws, out = empty(max(ws_bytes // 8, 1)), empty(M * N)
    A, B = empty(2 * M * K), empty(2 * max(K * N, M * K))
    with pytest.raises(nt.NativeError, match="null operand"):
        gpu.mul_sub_local(mode, P(A), P(B), None, None, P(out), M, K, N, P(ws), ws_bytes, None)


# ---- aby3g_mul_trunc_local on the direct MFMA branch (split-K 1): the GEMM
# writes the product into z and k_finish_trunc rewrites z in place

TRUNC_SHAPES = {
    # n even
    "257x200x250": dict(sharing=1, shape=(257, 200, 250), TM=3, TN=4),
    # odd n = 16125: C + n is 8 bytes off a 16-byte boundary, trunc_pair_block stores one word at a time.
    # 129 x K x 125 has 4 tiles, so sharing 1 plans one split only up to K = 224, which k_small_gemm takes
    # (<= 2^23 terms up to K = 520): K = 521 is the first K on the MFMA path, and 4 tiles are one split
    # from sharing 64 (256 / 64 target workgroups) on
    "129x521x125": dict(sharing=64, shape=(129, 521, 125), TM=2, TN=2),
    # odd n = 48375 at sharing 1: 12 tiles, 14 stages
    "129x200x375": dict(sharing=1, shape=(129, 200, 375), TM=2, TN=6),
    "g": dict(sharing=3, shape=(1024, 256, 1024), TM=8, TN=16),
}


@pytest.mark.parametrize("noff,poff", [(32, 40), (40, 32), (40, 48)])
@pytest.mark.parametrize("d", [8, 16, 27])
@pytest.mark.parametrize("name", list(TRUNC_SHAPES))
def test_mul_trunc_local_direct_mfma(gpu, name, d, noff, poff):
    """z = product - R and C = (RT0, RT1) against orc.local_product and
    orc.trunc_tuple. A next-stream offset of 40 bytes (an odd word) runs the
    in-place rewrite of z on the one-word path."""
    c = TRUNC_SHAPES[name]
    M, K, N = c["shape"]
    n = M * N
    A, B, prod = product(M, K, N, 100 + ord("g") if name == "g" else 44)
    ns, ps = k16(13), k16(14)
    eR, e0, e1 = orc.trunc_tuple(ns, noff, ps, poff, n, d)
    gz, gC = garbage(96, n + 1), garbage(97, 2 * n + 1)
    z, C = dev(gz), dev(gC)
    with sharing(gpu, c["sharing"]):
        plan = mfma_plan(gpu, M, K, N)
        expect_plan(plan, splits=1, TM=c["TM"], TN=c["TN"])
        ws = empty(plan.ws_bytes // 8)
        gpu.mul_trunc_local(GEMM, P(dev(A)), P(dev(B)), M, K, N, d, ctypes.byref(_ts(ns, noff, ps, poff)), P(z), P(C),
                            P(ws), plan.ws_bytes, None)
    zh, ch = host(z), host(C)
    assert np.array_equal(zh[:n], (prod.view(np.uint64) - eR.view(np.uint64)).view(np.int64))
    assert np.array_equal(ch[:n], e0) and np.array_equal(ch[n:2 * n], e1)
    assert zh[n] == gz[n] and ch[2 * n] == gC[2 * n], "wrote past the end of z or C"
