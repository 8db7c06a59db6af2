"""The binary engine's level kernels (aby3_amd/csrc/binary.hip: k_bin_level,
k_bin_level_in, k_lin_copy) against a numpy gate evaluator, bit-exact.

`level_ref` is the reference: one communication level of one party over
mem[2][wires][words], written from the eight gate formulas of common.h and
checked on the CPU first (three numpy parties evaluate two library circuits
level by level and must reveal a + b and (min, max)), so the GPU tests do not
share a wrong formula with the kernels.

`random_level` draws a level whose gates read the initial wires, the wires
this launch unpacks and the outputs of earlier batches, with z_row and
send_row from two different permutations (the product's z_row is
circuit-global, its send_row level-local). Every GPU case compares the WHOLE
engine memory and the whole send buffer with the reference, so a stray write
or an unwritten row shows.

Every case names the instantiation it means through `form`, the path guard:
a moved threshold fails the guard instead of quietly testing another form.
"""
import ctypes

import numpy as np
import pytest

from aby3_amd import native as nt

gpu_test = pytest.mark.gpu

U64 = np.uint64
NONE = 0xFFFFFFFF
AND_TYPES = (2, 3, 4, 5)
UNARY = (6, 7)
GATE_DT = np.dtype([("in0", "<u4"), ("in1", "<u4"), ("out", "<u4"), ("type", "<u4"), ("z_row", "<u4"),
                    ("send_row", "<u4")])
assert GATE_DT.itemsize == ctypes.sizeof(nt.Gate)

# The instantiations of k_bin_level (binary.hip:909-927, bin_level()): below
# SMAX workgroups (one per 32 words) the 1024-thread forms, from SMAX on the
# 256-thread ones; a launch with a wait or a post takes the hand-off form.
# NS gate slots a workgroup, each taking U gates of a batch per iteration.
SMAX = 128
FORMS = {
    # (small, hand-off): (NS, U)
    (True, False): (32, 4),   # k_bin_level<32, false, 1>
    (True, True): (32, 4),    # k_bin_level<32, true, 1>
    (False, False): (16, 4),  # k_bin_level<8, false, 2>
    (False, True): (16, 2),   # k_bin_level<8, true, 2, 2>
}
# k_bin_level_in<32, *, 1> / <8, *, 2>: the same slots, always four gates a slot
FORMS_IN = {True: (32, 4), False: (16, 4)}
WORDS = {
    "small": 96,                      # 3 workgroups: blockIdx offsets matter
    "small_last": 32 * (SMAX - 1),    # the last small launch
    "large": 32 * SMAX,               # the first large launch
    "large_odd": 32 * (SMAX + 1),     # an odd workgroup count
}
SPARE = 3  # rows of z that no send row matches, and sentinel rows after the send rows


# ------------------------------------------------------------- the reference

def and_share(t, x0, x1, y0, y1):
    """Share 0 of an AND-type gate before its mask (common.h:407-412)."""
    if t == 2:
        return (x0 & y0) ^ (x0 & y1) ^ (x1 & y0)
    if t == 3:
        return (x0 & y0) ^ (x0 & y1) ^ (x1 & y0) ^ x0 ^ y0
    if t == 4:
        return (~x0 & ~y0) ^ (~x0 & ~y1) ^ (~x1 & ~y0)
    assert t == 5
    return (~x0 & y0) ^ (~x0 & y1) ^ (~x1 & y0)


def local_gate(t, x0, x1, y0, y1):
    """Both shares of a local gate (common.h:415-422)."""
    if t == 6:
        return x0, x1
    if t == 7:
        return ~x0, ~x1
    if t == 0:
        return x0 ^ y0, x1 ^ y1
    assert t == 1
    return ~(x0 ^ y0), ~(x1 ^ y1)


def level_ref(mem, gates, batch_ends, recv, unpack_wires, z, send, rr=None):
    """One level of one party: (mem, send) after it, the arguments untouched.
    Share 1 of unpack_wires[j] takes recv[j]; then the gates run in order
    (gates of one batch are independent, so in-order evaluation is the
    reference). rr ([gates][2], NONE = engine memory): share 1 of that input
    is read from this row of recv, as aby3g_bin_level_rr states it."""
    mem, send = mem.copy(), send.copy()
    for j, w in enumerate(unpack_wires):
        mem[1, w] = recv[j]
    n = int(batch_ends[-1]) if len(batch_ends) else 0
    for i in range(n):
        g = gates[i]
        t, a = int(g["type"]), int(g["in0"])
        b = a if t in UNARY else int(g["in1"])  # unary gates ignore in1
        ra = NONE if rr is None else int(rr[i][0])
        rb = NONE if rr is None else int(rr[i][0 if t in UNARY else 1])
        x0, y0 = mem[0, a], mem[0, b]
        x1 = mem[1, a] if ra == NONE else recv[ra]
        y1 = mem[1, b] if rb == NONE else recv[rb]
        if t in AND_TYPES:
            r = and_share(t, x0, x1, y0, y1) ^ z[int(g["z_row"])]
            mem[0, int(g["out"])] = r
            send[int(g["send_row"])] = r
        else:
            o0, o1 = local_gate(t, x0, x1, y0, y1)
            mem[0, int(g["out"])] = o0
            mem[1, int(g["out"])] = o1
    return mem, send


def bit_slice(v, nbits, words):
    """[nbits][words] wire words of the values v (bit r of word w: row 64 w + r), zero past len(v)."""
    col = np.zeros(words * 64, dtype="<u8")
    col[:len(v)] = np.asarray(v).view(U64)
    bits = np.unpackbits(col.view(np.uint8).reshape(words, 64, 8), axis=2, bitorder="little")  # [word][row][bit]
    packed = np.packbits(bits.transpose(2, 0, 1), axis=2, bitorder="little")  # [bit][word][8 bytes of 8 rows]
    return np.ascontiguousarray(packed).view("<u8").reshape(64, words)[:nbits].astype(U64)


def bit_unslice(wire_words, rows):
    """The inverse: rows values from [nbits][words] wire words."""
    sh = np.arange(64, dtype=U64)
    v = np.zeros(wire_words.shape[1] * 64, dtype=U64)
    for b in range(wire_words.shape[0]):
        bits = ((wire_words[b][:, None] >> sh) & U64(1)).reshape(-1)
        v |= bits << U64(b)
    return v[:rows]


def u64s(rng, *shape):
    return rng.integers(0, 2**64, size=shape, dtype=U64)


def three_party_eval(cir, inputs, rows, seed):
    """Three numpy parties run `cir` level by level with level_ref: replicated
    XOR shares of the inputs, per-party masks with z0 ^ z1 ^ z2 == 0, each
    party's send rows the next party's recv rows. Returns the revealed outputs."""
    rng = np.random.default_rng(seed)
    words = -(-rows // 64)
    W = cir["wires"]
    G = cir["gates"]
    plain = np.zeros((W, words), dtype=U64)
    for wires, v in zip(cir["inputs"], inputs):
        plain[wires] = bit_slice(v, len(wires), words)
    s = [u64s(rng, W, words), u64s(rng, W, words)]
    s.append(plain ^ s[0] ^ s[1])
    # party i holds (s_i, s_{i-1}): share 0 goes to the next party as its share 1
    mem = [np.stack([s[i], s[(i + 2) % 3]]) for i in range(3)]
    n_and = int(np.isin(G[:, 3], AND_TYPES).sum())
    z = [u64s(rng, n_and, words), u64s(rng, n_and, words)]
    z.append(z[0] ^ z[1])
    zrow, first, prev_out, prev_send = 0, 0, [], [None] * 3
    for count in [int(c) for c in cir["levels"]] + [0]:  # one more launch unpacks the last AND shares
        lv = np.zeros(count, dtype=GATE_DT)
        outs = []
        for k in range(count):
            a, b, o, t = (int(x) for x in G[first + k])
            lv[k] = (a, b, o, t, 0, 0)
            if t in AND_TYPES:
                lv[k]["z_row"], lv[k]["send_row"] = zrow, len(outs)  # circuit-global / level-local
                zrow += 1
                outs.append(o)
        # the level's own AND outputs have no share 1 yet: no gate of the level may read them
        reads = set(lv["in0"].tolist()) | set(lv["in1"][~np.isin(lv["type"], UNARY)].tolist())
        assert not reads & set(outs)
        sends = []
        for i in range(3):
            recv = prev_send[(i + 2) % 3]
            mem[i], snd = level_ref(mem[i], lv, [count] if count else [], recv, prev_out, z[i],
                                    np.zeros((len(outs), words), dtype=U64))
            sends.append(snd)
        prev_out, prev_send, first = outs, sends, first + count
    assert zrow == n_and
    for i in range(3):  # replicated: my share 1 is the previous party's share 0
        for wires in cir["outputs"]:
            assert np.array_equal(mem[i][1, wires], mem[(i + 2) % 3][0, wires])
    return [bit_unslice(mem[0][0, wires] ^ mem[1][0, wires] ^ mem[2][0, wires], rows) for wires in cir["outputs"]]


def _vals(seed, n):
    v = np.random.default_rng(seed).integers(-(2**63), 2**63 - 1, size=n, dtype=np.int64, endpoint=True)
    v[:6] = [0, -1, 2**63 - 1, -(2**63), 1, 5]
    return v


def test_level_ref_reveals_library_circuits():
    """CPU only: the evaluator alone, no kernel."""
    rows = 100  # two words, the second mostly padding
    a, b = _vals(1, rows), _vals(2, rows)
    b[7] = a[7]
    (s,) = three_party_eval(nt.circuit("int_int_add", 64), [a, b], rows, 3)
    assert np.array_equal(s, a.view(U64) + b.view(U64))
    mn, mx = three_party_eval(nt.circuit("cmp_swap", 64), [a, b], rows, 4)
    assert np.array_equal(mn.view(np.int64), np.minimum(a, b))
    assert np.array_equal(mx.view(np.int64), np.maximum(a, b))


# --------------------------------------------------------- the random level

class Level:
    pass


def random_level(rng, n_free_wires, batch_sizes, n_unpack, must_read=()):
    """A level over wires [free | unpacked | gate outputs | one spare]:
    batch b's gates read wires that existed before batch b -- the free wires,
    the unpacked wires, the outputs of earlier batches -- and each writes a
    fresh wire. The unpacked wires come in three groups: readable from the
    first batch on, readable only by later batches, never read (they must
    still land in mem). Every later batch has a gate reading the batch before
    it; the first and the last batch hold every gate type; must_read wires
    are read by the first batch. Unary gates get a garbage in1 below `wires`."""
    L = Level()
    ngates = int(sum(batch_sizes))
    L.wires = n_free_wires + n_unpack + ngates + 1
    L.batch_ends = np.cumsum(batch_sizes).astype(np.uint32) if len(batch_sizes) else np.zeros(0, np.uint32)
    unp = n_free_wires + rng.permutation(n_unpack)  # recv row j -> a wire, not in wire order
    L.unpack_wires = unp.astype(np.uint32)
    third = -(-n_unpack // 3)
    early, late = list(unp[:third]), list(unp[third:2 * third])
    L.never_read = list(unp[2 * third:])
    outs = n_free_wires + n_unpack + rng.permutation(ngates)
    L.gates = np.zeros(ngates, dtype=GATE_DT)
    types = rng.integers(0, 8, size=ngates)
    first = 0
    for bi, n in enumerate(batch_sizes):
        if n >= 8 and bi in (0, len(batch_sizes) - 1):
            types[first:first + 8] = rng.permutation(8)
        first += n
    pool = list(range(n_free_wires)) + early
    first, late_read = 0, not late
    for bi, n in enumerate(batch_sizes):
        if bi == 1:
            pool += late
        forced = []  # (gate of the batch, operand, wire)
        if bi == 0:
            # reads of the unpacked wires that the recv rows tell apart: a unary gate whose in0 is
            # unpacked, a binary gate with only in1 unpacked, one with only in0, one with both
            una = [k for k in range(n) if types[k] in UNARY]
            bina = [k for k in range(n) if types[k] not in UNARY]
            if early and una:
                forced.append((una[0], 0, early[0]))
            if early and len(bina) >= 3:
                forced += [(bina[0], 1, early[-1]), (bina[0], 0, 0), (bina[1], 0, early[0]), (bina[1], 1, 1),
                           (bina[2], 0, early[0]), (bina[2], 1, early[-1])]
            taken = {k for k, _, _ in forced}
            slots = [(k, op) for k in range(n) if k not in taken for op in ((0,) if types[k] in UNARY else (0, 1))]
            assert len(slots) >= len(must_read), "the first batch is too small for must_read"
            forced += [(k, op, w) for (k, op), w in zip(slots, must_read)]
        else:
            forced.append((0, 0, int(outs[first - 1])))  # the last gate of the batch before
            if not late_read and n >= 2:
                forced.append((n - 1, 0 if types[first + n - 1] in UNARY else 1, late[0]))
                late_read = True
        for k in range(n):
            g = L.gates[first + k]
            g["type"] = types[first + k]
            g["in0"], g["in1"] = rng.choice(pool), rng.choice(pool)
            if g["type"] in UNARY:
                g["in1"] = rng.integers(0, L.wires)  # anything below `wires`: the header allows it
            g["out"] = outs[first + k]
        for k, op, w in forced:
            L.gates[first + k]["in1" if op else "in0"] = w
        pool += [int(o) for o in outs[first:first + n]]
        first += n
    is_and = np.isin(L.gates["type"], AND_TYPES)
    L.n_and = int(is_and.sum())
    L.z_rows = L.n_and + SPARE
    L.gates["z_row"][is_and] = rng.permutation(L.z_rows)[:L.n_and]
    L.gates["send_row"][is_and] = rng.permutation(L.n_and)
    assert L.n_and < 2 or (L.gates["z_row"][is_and] != L.gates["send_row"][is_and]).any()
    # recv_rows as Sh3BinaryEvaluator.cpp:53-76 builds them: the recv row of each input (in1 of a
    # unary gate included, whatever it is) that this launch unpacks
    row_of = {int(w): j for j, w in enumerate(L.unpack_wires)}
    L.rr = np.array([[row_of.get(int(g["in0"]), NONE), row_of.get(int(g["in1"]), NONE)] for g in L.gates],
                    dtype=np.uint32).reshape(ngates, 2)
    return L


def check_level(L, batch_sizes, n_unpack):
    """What the cases rely on, checked on the generated level itself."""
    written = set()
    first = 0
    unp = set(L.unpack_wires.tolist())
    assert len(set(L.gates["out"].tolist())) == len(L.gates) and not unp & set(L.gates["out"].tolist())
    for bi, n in enumerate(batch_sizes):
        b = L.gates[first:first + n]
        reads = set(b["in0"].tolist()) | set(b["in1"][~np.isin(b["type"], UNARY)].tolist())
        assert not reads & set(b["out"].tolist()), "gates of a batch are independent"
        assert bi == 0 or reads & written, "a later batch reads an earlier one"
        if n >= 8 and bi in (0, len(batch_sizes) - 1):
            assert set(b["type"].tolist()) == set(range(8))
        written |= set(b["out"].tolist())
        first += n
    assert int(L.gates["in0"].max(initial=0)) < L.wires and int(L.gates["in1"].max(initial=0)) < L.wires
    reads = set(L.gates["in0"].tolist()) | set(L.gates["in1"][~np.isin(L.gates["type"], UNARY)].tolist())
    assert not reads & set(L.never_read)


def test_random_level_has_the_edges():
    """CPU only: the generator delivers what the GPU cases are meant to run."""
    sizes = batch_sizes(16, 4)
    L = random_level(np.random.default_rng(1), 12, sizes, 4 * 16 + 5)
    check_level(L, sizes, 4 * 16 + 5)
    una = np.isin(L.gates["type"], UNARY)
    n0 = sizes[0]
    r0 = L.rr[:n0]
    assert (una[:n0] & (r0[:, 0] != NONE)).any(), "a unary gate whose in0 is unpacked"
    assert (~una[:n0] & (r0[:, 0] == NONE) & (r0[:, 1] != NONE)).any(), "a gate with only in1 unpacked"
    assert (~una[:n0] & (r0[:, 0] != NONE) & (r0[:, 1] == NONE)).any()
    assert (L.rr[n0:] != NONE).any(), "an unpacked wire read only by a later batch"
    assert L.never_read
    assert int(L.gates["z_row"].max()) >= L.n_and - 1


def batch_sizes(NS, U):
    """Every width around one slot stride and one unrolled iteration, a wide batch after a narrow one."""
    return [NS + 1, 1, 2 * U * NS + 3, NS - 1, U * NS, U * NS + 1, NS, U * NS - 1]


# ------------------------------------------------------------ device helpers

_KEEP = []  # device tensors whose pointers were handed to a kernel stay alive


@pytest.fixture(autouse=True)
def _release():
    yield
    _KEEP.clear()


def dev(a):
    import torch

    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).to("cuda")
    _KEEP.append(t)
    return t


def host(t, dtype=U64):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().view(dtype)


def P(t, byte_offset=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + byte_offset)


def timeouts(gpu):
    n = ctypes.c_uint32(0)
    gpu.handoff_status(ctypes.byref(n))
    return n.value


def form(gpu, words, handoff):
    """The path guard: (NS, U) of the instantiation a launch over `words`
    takes, with the threshold read back from the library."""
    vals = [ctypes.c_int() for _ in range(4)]
    gpu.bin_level_residency(*(ctypes.byref(v) for v in vals))
    smax = vals[3].value
    assert smax == SMAX, f"the small forms now end below {smax} workgroups: FORMS and WORDS describe {SMAX}"
    assert words % 32 == 0
    small = words // 32 < smax
    name = [k for k, w in WORDS.items() if w == words]
    assert name and name[0].startswith("small") == small, f"{words} words are on the other side of the threshold"
    return FORMS[(small, handoff)]


class Flags:
    """The hand-off flags of a launch: `wait` set before the launch (seq in
    some chunks, seq + 3 in others), `post` zeroed with a sentinel word after it."""
    SEQ = 7
    SENTINEL = 0x5EA1ED5EA1ED5EA1

    def __init__(self, chunks, wait, post):
        self.chunks = chunks
        self.wait = self.post = self.wait_t = self.post_t = None
        if wait:
            self.wait_t = dev(np.array([self.SEQ + 3 * (c % 2) for c in range(chunks)], dtype=U64))
            self.wait = nt.Handoff(self.wait_t.data_ptr(), self.SEQ, None)
        if post:
            self.post_t = dev(np.array([0] * chunks + [self.SENTINEL], dtype=U64))
            self.post = nt.Handoff(self.post_t.data_ptr(), self.SEQ, None)

    def ref(self, h):
        return None if h is None else ctypes.byref(h)

    def check(self):
        if self.post:
            f = host(self.post_t)
            assert np.array_equal(f[:self.chunks], np.full(self.chunks, self.SEQ, dtype=U64)), "a chunk not posted"
            assert int(f[self.chunks]) == self.SENTINEL, "posted past the last chunk"
        if self.wait:
            assert np.array_equal(host(self.wait_t),
                                  np.array([self.SEQ + 3 * (c % 2) for c in range(self.chunks)], dtype=U64))


def run_level(gpu, L, words, seed, entry="plain", wait=False, post=False):
    """One launch of the level L over seeded garbage against level_ref: the
    whole mem and the whole send buffer (its sentinel rows included)."""
    rng = np.random.default_rng(seed)
    nun, nb = len(L.unpack_wires), len(L.batch_ends)
    mem = u64s(rng, 2, L.wires, words) | U64(1)
    z, recv = u64s(rng, L.z_rows, words), u64s(rng, max(nun, 1), words)
    send = u64s(rng, L.n_and + SPARE, words) | U64(1)
    rr = L.rr if entry != "plain" and nun else None
    if entry == "rr":
        assert rr is not None
    exp_mem, exp_send = level_ref(mem, L.gates, L.batch_ends, recv, L.unpack_wires, z, send, rr)
    if nun:  # the two readings of the recv rows agree
        m2, s2 = level_ref(mem, L.gates, L.batch_ends, recv, L.unpack_wires, z, send, None)
        assert np.array_equal(m2, exp_mem) and np.array_equal(s2, exp_send)
    dm, ds = dev(mem), dev(send)
    g = dev(L.gates) if len(L.gates) else None
    ends = dev(L.batch_ends) if nb else None
    args = (P(ends), nb, P(dev(recv)) if nun or rr is not None else None, P(dev(L.unpack_wires)) if nun else None, nun,
            P(dm), L.wires, words, P(dev(z)), P(ds))
    fl = Flags(words // 32, wait, post)
    before = timeouts(gpu)
    if entry == "plain":
        gpu.bin_level(P(g), *args, None)
    elif entry == "rr":
        gpu.bin_level_rr(P(g), P(dev(rr)), *args, None)
    else:
        gpu.bin_level_hs(P(g), P(dev(rr)) if rr is not None else None, *args, fl.ref(fl.wait), fl.ref(fl.post), None)
    got_mem, got_send = host(dm).reshape(mem.shape), host(ds).reshape(send.shape)
    assert np.array_equal(got_send, exp_send), "send buffer"
    bad = np.argwhere((got_mem != exp_mem).any(axis=2))
    assert not len(bad), f"engine memory differs at (share, wire) {bad[:8].tolist()}"
    for w in L.never_read:
        j = L.unpack_wires.tolist().index(w)
        assert np.array_equal(got_mem[1, w], recv[j])
    fl.check()
    assert timeouts(gpu) == before


def make_level(seed, NS, U, n_unpack, short=False):
    sizes = [NS + 1, 1, 9] if short else batch_sizes(NS, U)
    L = random_level(np.random.default_rng(seed), 12, sizes, n_unpack)
    check_level(L, sizes, n_unpack)
    return L


def unpack_counts(NS):
    return [0, 1, NS - 1, 4 * NS + 5]


# ----------------------------------- aby3g_bin_level, _rr, _hs: all four forms

@gpu_test
@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("size", ["small", "large"])
def test_bin_level_plain(gpu, size, k):
    """k_bin_level<32, false, 1> and <8, false, 2>: every batch width around
    NS and U * NS, with 0, 1, NS - 1 and 4 NS + 5 unpacked wires."""
    words = WORDS[size]
    NS, U = form(gpu, words, False)
    run_level(gpu, make_level(10 + k, NS, U, unpack_counts(NS)[k]), words, 20 + k)


@gpu_test
@pytest.mark.parametrize("size", ["small_last", "large_odd"])
def test_bin_level_plain_threshold_neighbours(gpu, size):
    """The last small launch (a short gate list) and an odd large workgroup count."""
    words = WORDS[size]
    NS, U = form(gpu, words, False)
    run_level(gpu, make_level(30, NS, U, NS - 1, short=size == "small_last"), words, 31)


@gpu_test
@pytest.mark.parametrize("part", ["unpack_only", "gates_only"])
@pytest.mark.parametrize("handoff", [False, True])
@pytest.mark.parametrize("size", ["small", "large"])
def test_bin_level_one_part_empty(gpu, size, handoff, part):
    """nbatches = 0 with nunpack > 0, and nunpack = 0 with gates only; the
    hand-off forms with the one hand-off that part allows (a wait needs
    received shares)."""
    words = WORDS[size]
    NS, U = form(gpu, words, handoff)
    if part == "unpack_only":
        L = random_level(np.random.default_rng(40), 12, [], 4 * NS + 5)
        run_level(gpu, L, words, 41, "hs" if handoff else "plain", wait=handoff)
    else:
        run_level(gpu, make_level(42, NS, U, 0, short=True), words, 43, "hs" if handoff else "plain", post=handoff)


@gpu_test
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("size", ["small", "large"])
def test_bin_level_rr(gpu, size, k):
    """recv_rows: the gates take share 1 of the unpacked wires from the recv
    rows (the first batch runs without a barrier after the unpack), with
    unary gates whose in0 is unpacked and gates with only in1 unpacked."""
    words = WORDS[size]
    NS, U = form(gpu, words, False)
    run_level(gpu, make_level(50 + k, NS, U, unpack_counts(NS)[k]), words, 60 + k, "rr")


HS_CASES = [
    # size, wait, post, recv_rows, unpacked wires (index of unpack_counts), short gate list
    ("small", True, True, True, 3, False),
    ("small", True, True, False, 2, False),
    ("small", True, False, True, 1, False),
    ("small", False, True, False, 0, False),
    ("small", False, True, True, 3, False),
    ("small_last", True, True, True, 2, True),
    ("large", True, True, True, 3, False),
    ("large", True, True, False, 2, False),
    ("large", True, False, True, 1, False),
    ("large", False, True, False, 0, False),
    ("large", False, True, True, 3, False),
    ("large_odd", True, True, True, 2, False),
]


@gpu_test
@pytest.mark.parametrize("size,wait,post,rr,k,short", HS_CASES)
def test_bin_level_handoff_forms(gpu, size, wait, post, rr, k, short):
    """k_bin_level<32, true, 1> and <8, true, 2, 2> (the only U = 2 form)
    through aby3g_bin_level_hs: wait flags already at seq or beyond, post
    flags zeroed; wait and post, wait only, post only."""
    words = WORDS[size]
    NS, U = form(gpu, words, True)
    L = make_level(70 + k, NS, U, unpack_counts(NS)[k], short)
    if not rr:
        L.rr = None
    run_level(gpu, L, words, 80 + k, "hs", wait, post)


# ------------------------------------------------------- aby3g_bin_level_in

class Src:
    """One source of aby3g_bin_level_in: `nbits` wires from `wire` on of
    `share`, v[r] = sum coef[t] term[t][r] + constant for r < rows."""

    def __init__(self, wire, share, nbits=64, terms=(), constant=0):
        self.wire, self.share, self.nbits, self.terms, self.constant = wire, share, nbits, list(terms), constant

    def value(self, rows):
        v = np.zeros(rows, dtype=U64)
        with np.errstate(over="ignore"):
            for coef, t in self.terms:
                if t is not None:
                    v += U64(coef % 2**64) * t.view(U64)
            return v + U64(self.constant % 2**64)

    @property
    def has_terms(self):
        return any(t is not None for _, t in self.terms)


def input_wires_ref(srcs, rows, in_lo, in_hi, words):
    """[2][in_hi - in_lo][words]: the sources' values bit-sliced, zero on rows
    >= rows (the constant does not reach them) and on wires no source covers."""
    inp = np.zeros((2, in_hi - in_lo, words), dtype=U64)
    for s in srcs:
        if s.has_terms:
            inp[s.share, s.wire - in_lo:s.wire - in_lo + s.nbits] = bit_slice(s.value(rows), s.nbits, words)
    return inp


def level_in_ref(mem, srcs, rows, in_lo, in_hi, write_inputs, L, z, send):
    inp = input_wires_ref(srcs, rows, in_lo, in_hi, mem.shape[2])
    m = mem.copy()
    m[:, in_lo:in_hi] = inp
    m, s = level_ref(m, L.gates, L.batch_ends, None, [], z, send)
    if not write_inputs:
        m[:, in_lo:in_hi] = mem[:, in_lo:in_hi]  # the input wires' garbage is untouched
    return m, s


def wire_srcs(srcs, dmem, wires, words, cols64=1):
    """The aby3g_wire_src array of `srcs` over the device memory dmem; the terms stay alive in _KEEP."""
    arr = (nt.WireSrc * max(len(srcs), 1))()
    for k, s in enumerate(srcs):
        for t, (coef, term) in enumerate(s.terms):
            arr[k].coef[t] = coef
            if term is not None:
                arr[k].term[t] = ctypes.cast(dev(term).data_ptr(), ctypes.POINTER(ctypes.c_int64))
        arr[k].constant, arr[k].cols64, arr[k].nbits = s.constant, cols64, s.nbits
        arr[k].wire_rows = ctypes.cast(dmem.data_ptr() + 8 * (s.share * wires + s.wire) * words,
                                       ctypes.POINTER(ctypes.c_uint64))
    return arr


def i64s(rng, n):
    return rng.integers(-(2**63), 2**63 - 1, size=n, dtype=np.int64, endpoint=True)


IN_SHAPES = {
    # size: (words, rows): rows no multiple of 64 or 2048, the last chunk mostly padding
    "small": (64, 2048 + 65),
    "large": (WORDS["large"], 2048 * (SMAX - 1) + 65),
}


def in_form(gpu, size):
    words, rows = IN_SHAPES[size]
    vals = [ctypes.c_int() for _ in range(4)]
    gpu.bin_level_residency(*(ctypes.byref(v) for v in vals))
    assert vals[3].value == SMAX
    assert (words // 32 < SMAX) == (size == "small") and 64 * (words - 32) < rows < 64 * words
    return words, rows, FORMS_IN[size == "small"]


def run_level_in(gpu, srcs, in_lo, in_hi, L, words, rows, seed, write_inputs, post):
    rng = np.random.default_rng(seed)
    mem = u64s(rng, 2, L.wires, words) | U64(1)
    z = u64s(rng, L.z_rows, words)
    send = u64s(rng, L.n_and + SPARE, words) | U64(1)
    exp_mem, exp_send = level_in_ref(mem, srcs, rows, in_lo, in_hi, write_inputs, L, z, send)
    dm, ds = dev(mem), dev(send)
    arr = wire_srcs(srcs, dm, L.wires, words)
    fl = Flags(words // 32, False, post)
    before = timeouts(gpu)
    gpu.bin_level_in(arr, len(srcs), rows, in_lo, in_hi, write_inputs, P(dev(L.gates)), P(dev(L.batch_ends)),
                     len(L.batch_ends), P(dm), L.wires, words, P(dev(z)), P(ds), fl.ref(fl.post), None)
    got_mem, got_send = host(dm).reshape(mem.shape), host(ds).reshape(send.shape)
    assert np.array_equal(got_send, exp_send), "send buffer"
    bad = np.argwhere((got_mem != exp_mem).any(axis=2))
    assert not len(bad), f"engine memory differs at (share, wire) {bad[:8].tolist()}"
    fl.check()
    assert timeouts(gpu) == before
    return mem, z, send, got_mem, got_send


def in_level(seed, n_initial, NS, U, full=False, must_read=()):
    sizes = batch_sizes(NS, U) if full else [NS + 1, 3, 9]
    L = random_level(np.random.default_rng(seed), n_initial, sizes, 0, must_read)
    check_level(L, sizes, 0)
    return L


def four_pairs(rng, rows, in_lo=0):
    """Two 64-bit inputs x two shares, four terms each with negative and
    wrap-around coefficients and a non-zero constant."""
    coefs = [(3, -1, 2**63 - 1, -(2**63)), (-7, 2**62, 1, -2), (1, 1, -1, 5), (-(2**63), 2**63 - 1, -3, 9)]
    consts = [1234567, -5, 2**63 - 1, -(2**62) - 1]
    return [Src(in_lo + 64 * (k // 2), k % 2, 64, [(c, i64s(rng, rows)) for c in coefs[k]], consts[k])
            for k in range(4)]


@gpu_test
@pytest.mark.parametrize("write_inputs", [0, 1])
@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("size", ["small", "large"])
def test_level_in_all_four_pairs(gpu, size, post, write_inputs):
    """All four (input, share) pairs with terms, nin = 128, every batch width;
    with write_inputs = 0 the input wires' garbage in mem is untouched, with 1
    they hold the transposed values."""
    words, rows, (NS, U) = in_form(gpu, size)
    srcs = four_pairs(np.random.default_rng(90), rows)
    L = in_level(91, 128 + 6, NS, U, full=True, must_read=[128, 133])
    run_level_in(gpu, srcs, 0, 128, L, words, rows, 92, write_inputs, post)


def role_sources(role, rng, rows, in_lo=0):
    """The sources setTwoInputSharing queues (Sh3BinaryEvaluator.cpp:443-499) in
    its three term patterns; a copy-out already made is one term of coefficient 1."""
    in0, in1 = in_lo, in_lo + 64
    zero = lambda w, s: Src(w, s, 64, [], 0)  # noqa: E731
    if role == "one_with_terms":  # P0: in0 = (sign (x0 + x2) + off, 0), in1 = (0, 0)
        return [Src(in0, 0, 64, [(1, i64s(rng, rows))], -(2**40) + 3), zero(in0, 1), zero(in1, 0), zero(in1, 1)]
    if role == "two_with_terms":  # P1: in1 = (x1, 0), in0 = (0, v + off)
        return [Src(in1, 0, 64, [(1, i64s(rng, rows))], 0), zero(in1, 1), zero(in0, 0),
                Src(in0, 1, 64, [(1, i64s(rng, rows))], 2**40 + 1)]
    return [zero(in0, 0), zero(in0, 1), zero(in1, 0), zero(in1, 1)]  # nl = 0: no LDS at all


@gpu_test
@pytest.mark.parametrize("role", ["one_with_terms", "two_with_terms", "none_with_terms"])
@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("size", ["small", "large"])
def test_level_in_party_roles(gpu, size, post, role):
    words, rows, (NS, U) = in_form(gpu, size)
    srcs = role_sources(role, np.random.default_rng(100), rows)
    run_level_in(gpu, srcs, 0, 128, in_level(101, 128 + 4, NS, U), words, rows, 102, 1, post)


@gpu_test
@pytest.mark.parametrize("write_inputs", [0, 1])
@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("size", ["small", "large"])
def test_level_in_short_and_offset_sources(gpu, size, post, write_inputs):
    """in_lo = 3, sources of 1, 16 and 64 bits with gaps inside [in_lo, in_hi):
    the uncovered wires read zero (and are written as zero with write_inputs);
    gates also read wires below in_lo and from in_hi on, which come from mem."""
    words, rows, (NS, U) = in_form(gpu, size)
    rng = np.random.default_rng(110)
    in_lo, in_hi = 3, 3 + 110
    srcs = [Src(5, 1, 1, [(-3, i64s(rng, rows)), (0, None), (2, i64s(rng, rows))], 1),  # a null term in the middle
            Src(10, 0, 16, [(1, i64s(rng, rows))], -1),
            Src(10, 1, 16, [], 0),
            Src(40, 0, 64, [(2**63 - 1, i64s(rng, rows)), (5, i64s(rng, rows))], 77),
            Src(45, 1, 64, [(1, i64s(rng, rows))], 0)]
    L = in_level(111, in_hi + 5, NS, U, must_read=[0, 2, 3, 4, 5, 6, 26, 104, 109, in_hi - 1, in_hi, in_hi + 4])
    run_level_in(gpu, srcs, in_lo, in_hi, L, words, rows, 112, write_inputs, post)


@gpu_test
@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("size", ["small", "large"])
def test_level_in_eight_sources_with_terms(gpu, size, post):
    """ABY3G_WIRE_SRC_MAX sources with terms: 128 KiB of dynamic LDS beside
    the kernel's static 512 bytes, beyond the 64 KiB a launch gets unasked
    (the entry point raises the limit with hipFuncSetAttribute; on the MI355X
    the launch is accepted and computes the reference's values)."""
    words, rows, (NS, U) = in_form(gpu, size)
    rng = np.random.default_rng(120)
    srcs = [Src(16 * k, k % 2, 16, [(k + 1, i64s(rng, rows)), (-1, i64s(rng, rows))], 3 * k - 7) for k in range(8)]
    L = in_level(121, 128 + 4, NS, U, must_read=[0, 15, 16, 127])
    run_level_in(gpu, srcs, 0, 128, L, words, rows, 122, 1, post)


def depth_batches(gates):
    """A level's gates (n x 4) in batches by in-level dependency depth: a
    gate's batch is one more than its deepest in-level producer. Returns the
    reordered gate indices and the batch sizes."""
    depth_of, depth = {}, []
    for a, b, o, t in gates.tolist():
        ins = [a] if t in UNARY else [a, b]
        d = 1 + max([depth_of.get(w, -1) for w in ins])
        depth_of[o] = d
        depth.append(d)
    depth = np.array(depth)
    order = np.argsort(depth, kind="stable")
    return order, np.bincount(depth).tolist()


@gpu_test
@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("size", ["small", "large"])
def test_level_in_real_first_level(gpu, size, post):
    """Level 0 of the comparison circuit with P0's sources."""
    words, rows, _ = in_form(gpu, size)
    cir = nt.circuit("int_comp_helper", 64)
    lv = cir["gates"][:int(cir["levels"][0])]
    order, sizes = depth_batches(lv)
    assert len(sizes) > 1 and sum(sizes) == len(lv)
    L = Level()
    L.wires, L.batch_ends = cir["wires"], np.cumsum(sizes).astype(np.uint32)
    g = np.zeros(len(lv), dtype=GATE_DT)
    row = 0
    for k, (a, b, o, t) in enumerate(lv.tolist()):  # mask and send rows in level-list order
        g[k] = (a, b, o, t, 0, 0)
        if t in AND_TYPES:
            g[k]["z_row"] = g[k]["send_row"] = row
            row += 1
    L.gates, L.n_and, L.z_rows = g[order], row, row + SPARE
    in_lo = min(min(w) for w in cir["inputs"])
    in_hi = max(max(w) for w in cir["inputs"]) + 1
    assert [len(w) for w in cir["inputs"]] == [64, 64] and in_hi - in_lo == 128
    assert cir["inputs"][0][0] == in_lo and cir["inputs"][1][0] == in_lo + 64
    srcs = role_sources("one_with_terms", np.random.default_rng(130), rows, in_lo)
    run_level_in(gpu, srcs, in_lo, in_hi, L, words, rows, 131, 1, post)


@gpu_test
@pytest.mark.parametrize("size", ["small", "large"])
def test_level_in_equals_transpose_then_level(gpu, size):
    """The header's equivalence: aby3g_bin_level_in with write_inputs ==
    aby3g_bits_to_wires_lin then aby3g_bin_level on a second copy of mem."""
    words, rows, (NS, U) = in_form(gpu, size)
    srcs = four_pairs(np.random.default_rng(140), rows, in_lo=2)
    L = in_level(141, 2 + 128 + 3, NS, U, must_read=[0, 1, 130, 132])
    mem, z, send, got_mem, got_send = run_level_in(gpu, srcs, 2, 130, L, words, rows, 142, 1, False)
    dm, ds = dev(mem), dev(send)
    gpu.bits_to_wires_lin(wire_srcs(srcs, dm, L.wires, words), len(srcs), rows, words, None)
    gpu.bin_level(P(dev(L.gates)), P(dev(L.batch_ends)), len(L.batch_ends), None, None, 0, P(dm), L.wires, words,
                  P(dev(z)), P(ds), None)
    assert np.array_equal(host(dm).reshape(mem.shape), got_mem)
    assert np.array_equal(host(ds).reshape(send.shape), got_send)


@gpu_test
@pytest.mark.parametrize("what,match", [
    ("constant_without_terms", "zero constant"),
    ("copy_out", "copy_out"),
    ("two_columns", "one 64-bit column"),
    ("wire_rows_before_mem", "wire_rows outside mem"),
    ("wire_rows_after_mem", "wire_rows outside mem"),
    ("source_below_in_lo", r"outside \[in_lo, in_hi\)"),
    ("source_past_in_hi", r"outside \[in_lo, in_hi\)"),
    ("too_many_input_wires", "input wires out of range"),
])
def test_level_in_rejections(gpu, what, match):
    words, rows, wires = 32, 100, 200
    rng = np.random.default_rng(150)
    mem = u64s(rng, 2, wires, words)
    # mem starts one wire row into its tensor, so that a pointer before it is still an address of the test's
    both = dev(np.concatenate([np.zeros(words, dtype=U64), mem.reshape(-1), np.zeros(words, dtype=U64)]))

    class M:
        @staticmethod
        def data_ptr():
            return both.data_ptr() + 8 * words

    in_lo, in_hi, cols64 = 4, 132, 1
    s = Src(4, 0, 64, [(1, i64s(rng, rows))], 9)
    if what == "constant_without_terms":
        s = Src(4, 0, 64, [], 9)
    elif what == "source_below_in_lo":
        s.wire = in_lo - 1
    elif what == "source_past_in_hi":
        s.wire = in_hi - 63
    elif what == "too_many_input_wires":
        in_hi = in_lo + 129
    elif what == "two_columns":
        cols64 = 2
    arr = wire_srcs([s], M, wires, words, cols64)
    if what == "copy_out":
        arr[0].copy_out = ctypes.cast(dev(np.zeros(rows, dtype=U64)).data_ptr(), ctypes.POINTER(ctypes.c_int64))
    elif what == "wire_rows_before_mem":
        arr[0].wire_rows = ctypes.cast(M.data_ptr() - 8 * words, ctypes.POINTER(ctypes.c_uint64))
    elif what == "wire_rows_after_mem":
        arr[0].wire_rows = ctypes.cast(M.data_ptr() + 8 * 2 * wires * words, ctypes.POINTER(ctypes.c_uint64))
    g = np.zeros(1, dtype=GATE_DT)
    g[0] = (4, 5, 150, 0, 0, 0)
    with pytest.raises(nt.NativeError, match=match):
        gpu.bin_level_in(arr, 1, rows, in_lo, in_hi, 0, P(dev(g)), P(dev(np.array([1], dtype=np.uint32))), 1,
                         ctypes.c_void_p(M.data_ptr()), wires, words, P(dev(u64s(rng, 1, words))), None, None, None)
    assert np.array_equal(host(both)[words:-words].reshape(mem.shape), mem), "a rejected call launched"


# ------------------------------------------------------- aby3g_lin_copy_out

SENT = np.int64(0x0DDC0FFEE0DDF00D)


class Copy:
    """One source of aby3g_lin_copy_out: terms ([rows * cols64] or None, with
    the words to skip into their device buffers), and where copy_out starts."""

    def __init__(self, rng, rows, cols64, coefs, null=(), term_skip=(0, 0, 0, 0), out_skip=0, has_out=True):
        n = rows * cols64
        self.n, self.cols64, self.coefs, self.term_skip, self.out_skip, self.has_out = (n, cols64, coefs, term_skip,
                                                                                        out_skip, has_out)
        self.terms = [None if t in null or t >= len(coefs) else i64s(rng, n) for t in range(4)]
        self.out0 = np.concatenate([i64s(rng, out_skip + n) | np.int64(1), [SENT]])

    def expect(self):
        v = np.zeros(self.n, dtype=U64)
        with np.errstate(over="ignore"):
            for c, t in zip(self.coefs, self.terms):
                if t is not None:
                    v += U64(c % 2**64) * t.view(U64)
        e = self.out0.copy()
        if self.has_out:
            e[self.out_skip:self.out_skip + self.n] = v.view(np.int64)
        return e


COPY_CASES = {
    "even_rows_aligned": lambda r: (1000, [Copy(r, 1000, 1, (3, -1, 2**63 - 1, -(2**63)))]),
    "odd_rows_scalar_tail": lambda r: (1001, [Copy(r, 1001, 1, (3, -1))]),
    "term_one_word_in": lambda r: (1000, [Copy(r, 1000, 1, (3, -1, 5), term_skip=(0, 1, 0, 0))]),
    "copy_out_one_word_in": lambda r: (1000, [Copy(r, 1000, 1, (3, -1), out_skip=1)]),
    "one_row": lambda r: (1, [Copy(r, 1, 1, (-7, 2))]),
    "two_column_counts": lambda r: (700, [Copy(r, 700, 1, (2, 9)), Copy(r, 700, 2, (-1, 4, 6))]),
    "null_copy_out_between": lambda r: (514, [Copy(r, 514, 1, (1, 1)), Copy(r, 514, 1, (5,), has_out=False),
                                              Copy(r, 514, 1, (-3, 8))]),
    "null_term_in_the_middle": lambda r: (1000, [Copy(r, 1000, 1, (3, -1, 11, -13), null=(1, 2))]),
}


@gpu_test
@pytest.mark.parametrize("name", list(COPY_CASES))
def test_lin_copy_out(gpu, name):
    """copy_out = sum coef[t] term[t] (no constant) over rows x cols64, by
    16-byte accesses where every pointer allows them and one word at a time
    otherwise; a sentinel word follows every copy_out buffer."""
    rows, cps = COPY_CASES[name](np.random.default_rng(160))
    arr = (nt.WireSrc * len(cps))()
    outs = []
    for k, c in enumerate(cps):
        for t in range(4):
            arr[k].coef[t] = c.coefs[t] if t < len(c.coefs) else 0
            if c.terms[t] is not None:
                skip = c.term_skip[t]
                d = dev(np.concatenate([np.zeros(skip, dtype=np.int64), c.terms[t]]))
                assert d.data_ptr() % 16 == 0
                arr[k].term[t] = ctypes.cast(d.data_ptr() + 8 * skip, ctypes.POINTER(ctypes.c_int64))
        arr[k].constant, arr[k].cols64, arr[k].nbits = 12345, c.cols64, 64 * c.cols64
        d = dev(c.out0)
        assert d.data_ptr() % 16 == 0
        outs.append(d)
        if c.has_out:
            arr[k].copy_out = ctypes.cast(d.data_ptr() + 8 * c.out_skip, ctypes.POINTER(ctypes.c_int64))
    gpu.lin_copy_out(arr, len(cps), rows, None)
    for c, d in zip(cps, outs):
        assert np.array_equal(host(d, np.int64), c.expect())
