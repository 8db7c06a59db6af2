#!/usr/bin/env python3
"""Benchmark of the ABY3 replicated-secret-sharing hot path on MI355X.

Workload (BASELINE.json configs[1]): Sh3Evaluator::asyncMul on 1024x1024
sf64Matrix shares with truncation (D16), upstream GEMM semantics, three
parties. On each GPU the three parties run co-located (three host threads,
three HIP streams, device-to-device channels); with --gpus N every rank runs
its own independent 3-party job on its own GPU (weak scaling, no data-path
collective: each rank's multiplications are independent units of work).

One step = one complete 3-party asyncMul + truncation: every party's digit
split + int8-MFMA share GEMM, truncation pair (AES-CTR on device), the z
messages to P0/P1 and the finalize. `value` = secret-shared 64-bit mults
(M*N*K product terms per multiplication) completed per second by the whole
job; the metric is quoted "per party" because every party takes part in
every multiplication.

A plain run sets up, warms up, times --steps steps, writes the last step's
product if --dump-outputs is given, and prints the JSON line. Every other
leg runs only with --full: the plaintext check of the product, and the legs
behind these further entries of the JSON line:
  roofline      -- the share-GEMM kernel: int8 MFMA ops per launch
                   (144*M*N*K) / its average launch time,
                   measured with HIP events on the party streams, vs the
                   gfx950 dense int8 peak; `traffic` from the committed PMC
                   profile when one matches (profiles/pmc_*.json);
  binary        -- the binary-AND side of the metric (config C3): cipher_gt
                   (reshare + MSB(a+b) circuit) over 2^20 rows, AND
                   word-gates/s and the gate-kernel HBM roofline;
  cpu_baseline  -- the CPU restatement (oracle/, kind "port") of the same
                   multiplication on this host, 3 party threads.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_INT8_TOPS = 256 * 4 * 2048 * 2.4e9 / 1e12  # 256 CU x 4 SIMD x 2048 int8 op/clk x 2.4 GHz = 5033 TOP/s
PEAK_HBM_GBS = 8000.0  # MI355X HBM3E spec


# timed LR iterations (host-API bound, so a longer sample for a stable figure)
LR_ITERS = 300

# --dump-outputs writes at most this much
DUMP_LIMIT_BYTES = 64 << 20
# and tops the pre-warm's step count up to a multiple of this (0.3 s of C2
# steps is about 1200 steps, so runs on slower and faster builds land on 4096)
DUMP_STEP_QUANTUM = 4096

def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--decimal", type=int, default=16)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run every other leg: the plaintext check of the product, the "
                         "share-GEMM roofline pass and kernel breakdown, the binary (C3) leg, the C1/C4/C5 and "
                         "conversion extras, the party-process layouts and the CPU baselines (minutes, not "
                         "seconds). Without it the run sets up, warms up, times --steps steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last timed step computed to DIR/product.npy: the "
                         "product the three parties' result shares reveal, as float64 (fixed point / 2^decimal), "
                         f"row-major; above {DUMP_LIMIT_BYTES >> 20} MB a fixed seeded sample of its entries. The "
                         "operands are the same in every run. The truncation's last bit depends on how many steps "
                         f"ran before, so the pre-warm is topped up to a multiple of {DUMP_STEP_QUANTUM} steps: runs "
                         "with the same arguments then write the same array (were the counts to differ, entries "
                         "would differ by at most 4 * 2^-decimal)")
    ap.add_argument("--binary-rows", type=int, default=1 << 20)
    ap.add_argument("--binary-steps", type=int, default=30)
    ap.add_argument("--binary-cpu-rows", type=int, default=1 << 18, help="rows of the CPU baseline sample (C3)")
    ap.add_argument("--no-binary", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-reps", type=int, default=10)
    ap.add_argument("--no-extras", action="store_true", help="skip the LR-iteration and merge-layer lines")
    ap.add_argument("--lr-rows", type=int, default=1000000)
    ap.add_argument("--prewarm-s", type=float, default=0.3,
                    help="seconds of untimed steps before the W warmup steps of every timed leg: the GPU's clocks "
                         "take ~50 ms of load to ramp after an idle host phase (scripts/steady_state.py: C2 "
                         "0.32 ms/step after 5 warmup steps vs 0.255 after 50 ms of steps)")
    ap.add_argument("--gemm-turns", action="store_true",
                    help="co-located parties' share GEMMs take turns in every pass (aby3g_mfma_turn), so that a "
                         "profiler's launch spans are the kernel's own (scripts/gpu_profile.sh)")
    ap.add_argument("--deployment", choices=("replicas", "parties", "rowsplit"), default="replicas",
                    help="replicas: every rank runs a whole 3-party job on its GPU; parties: every 3 ranks form "
                         "one job, one party per rank and GPU (the north_star layout; world size a multiple of 3); "
                         "rowsplit: the ranks split one product's rows, rank r running rows [r*M/N, (r+1)*M/N) as "
                         "a 3-party job on its GPU, every party's rows split over the N GPUs (SURVEY.md §8e; "
                         "strong scaling)")
    return ap.parse_args()


def dist_setup():
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    pg = None
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # control plane only (barrier, max over ranks): no data crosses ranks.
        # gloo reports its connections on the process's stdout, where the
        # one JSON line goes: point fd 1 at stderr while it connects.
        sys.stdout.flush()
        saved = os.dup(1)
        os.dup2(2, 1)
        try:
            dist.init_process_group(backend="gloo")
            dist.barrier()
        finally:
            sys.stdout.flush()
            os.dup2(saved, 1)
            os.close(saved)
        pg = dist
    return world, rank, local, pg


def progress(msg):
    """One line per phase on stderr: a long default run keeps writing (the
    GPU harness takes a silent command for a hung one)."""
    print(f"bench: {msg} ({time.strftime('%H:%M:%S')})", file=sys.stderr, flush=True)


def barrier(pg):
    if pg is not None:
        pg.barrier()


def allmax(pg, x: float) -> float:
    if pg is None:
        return x
    import torch

    t = torch.tensor([x], dtype=torch.float64)
    pg.all_reduce(t, op=pg.ReduceOp.MAX)
    return float(t.item())


def load_pmc(kind: str, cfg: dict, field: str = "hbm_bytes_per_launch"):
    """HBM bytes (per launch, or the named field) from a committed rocprofv3
    PMC summary (profiles/pmc_*.json, scripts/pmc_summary.py), if its config matches."""
    import glob

    best = None
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "pmc_*.json"))):
        try:
            d = json.load(open(f))
        except Exception:
            continue
        e = d.get(kind)
        if e and e.get("config") == cfg:
            best = e.get(field)
    return best


def load_mfma(cfg: dict):
    """The newest committed MFMA PMC summary (profiles/mfma_*.json, written by
    scripts/mfma_summary.py for the C2 job at 1024^3), or None."""
    import glob

    if cfg != {"m": 1024, "k": 1024, "n": 1024}:
        return None
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "mfma_r*.json")))
    if not files:
        return None
    d = json.load(open(files[-1]))
    keep = ("avg_ns", "effective_clock_ghz", "mfma_busy_frac_of_occupied_simds", "mfma_busy_over_issued_cycles",
            "mfma_instructions", "note")
    out = {k: d[k] for k in keep if k in d}
    out["source"] = os.path.join("profiles", os.path.basename(files[-1]))
    return out


def compute_fraction(nt, job, params, dev, steps, warmup=3):
    """The local-compute fraction of wall clock, measured on the device: a
    separate pass of the job with every kernel launch bracketed by HIP events
    (all families, all parties): per party and step, the time its stream
    spends inside its own kernels minus the time those kernels spent waiting
    in-kernel for a peer's message (aby3g_handoff wait_ticks), over the pass's
    wall clock per step. Hand-offs by stream operations (waits outside the
    kernels) and dispatch gaps count as not computing. The probes add host
    work per launch, so the pass runs a little slower than the timed one."""
    with nt.Session(job, params, devices=(dev,) * 3, probe=True) as s:
        s.run(warmup)
        prewarm(s, 0.2)
        s.probe_reset()
        t0 = time.perf_counter()
        s.run(steps)
        wall_us = (time.perf_counter() - t0) * 1e6 / steps
        fam_ms = [s.probe(fam)[0] / steps for fam in range(6)]  # all parties, per step
        kernel_us = sum(fam_ms) * 1e3 / 3  # per party
        wait_us = s.info()["device_wait_us"]
    return {
        "family_ms_per_step": fam_ms,
        "local_compute_fraction": max(0.0, min(1.0, (kernel_us - wait_us) / wall_us)),
        "kernel_us_per_step": kernel_us, "in_kernel_wait_us_per_step": wait_us, "probed_step_us": wall_us,
        "method": "per party: HIP-event kernel time - in-kernel peer waits, over the wall clock of a probed pass. "
                  "The in-kernel waits are those of each launch's first workgroup (hs_wait) and of the fused "
                  "LR launch's protocol workgroup: other workgroups of a multi-chunk level may wait longer, so "
                  "the fraction is an upper bound",
    }


def prewarm(sess, secs, chunk=5):
    """Untimed steps for `secs` seconds (clock ramp after host-side phases
    such as a reveal or session setup); returns the steps run."""
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < secs:
        sess.run(chunk)
        n += chunk
    return n


def timed(sess, steps, pg, secs=0.0, warmup=0):
    """Pre-warm for `secs`, run `warmup` steps, then time exactly `steps`."""
    if secs > 0:
        prewarm(sess, secs)
    if warmup:
        sess.run(warmup)
    barrier(pg)
    t0 = time.perf_counter()
    sess.run(steps)
    t1 = time.perf_counter()
    barrier(pg)
    return allmax(pg, t1 - t0)


def dump_outputs(sess, path, rows, cols, decimal):
    """What the last step of `sess` (a C2 session) computed, as a caller of
    asyncMul receives it and reveals it: the three parties' first result
    shares summed modulo 2^64, the fixed-point product, written as float64
    (exact: the product of operands in [-8, 8) has far fewer than 53 bits)
    to path/product.npy. Above DUMP_LIMIT_BYTES a sample of the entries at
    fixed seeded positions, in row-major order."""
    import numpy as np

    total = np.zeros(rows * cols, dtype=np.uint64)
    for party in range(3):
        total += sess.result(party)[0].view(np.uint64)
    prod = total.view(np.int64).astype(np.float64) / float(1 << decimal)
    limit = DUMP_LIMIT_BYTES // 8
    if prod.size > limit:
        prod = prod[np.sort(np.random.default_rng(0).choice(prod.size, limit, replace=False))]
    else:
        prod = prod.reshape(rows, cols)
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "product.npy"), prod)


def cpu_mul_procs_s(mode, reps):
    """Seconds per C1 multiplication of the oracle as BASELINE configs[0]
    states it: three CPU processes, one party each, the reshare crossing
    between them (oracle/src/orc_c1_procs.cpp; cpu_baseline leg only)."""
    import subprocess

    exe = os.path.join(ROOT, "oracle", "build", "orc_c1_procs")
    r = subprocess.run([exe, str(mode), "128", "128", "128", str(reps)], capture_output=True, text=True,
                       timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"bench: oracle C1 process baseline failed ({r.returncode}): {r.stderr[-500:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])["secs"] / reps


def cpu_mul_s(mode, reps):
    """Seconds per C1 multiplication of the oracle (cpu_baseline leg only)."""
    import ctypes

    orc = ctypes.CDLL(os.path.join(ROOT, "oracle", "build", "liborc.so"))
    orc.orc_bench_mul.restype = ctypes.c_double
    secs = orc.orc_bench_mul(mode, 128, 128, 128, reps)
    if secs < 0:
        raise SystemExit("bench: oracle C1 baseline failed")
    return secs / reps


def party_job(job, params, steps, warmup=0, layout=1):
    """A job in the north_star's process layout: three processes, one party
    each (aby3h_party_create), on this node's GPU 0 (the driver's boxes have
    one GPU, so the three share it), messages over the shared-memory links
    and IPC staging slots (the fused LR iteration over IPC-mapped mailboxes).
    Returns the slowest party's ms per step and the parties' lines."""
    import subprocess

    link = f"bench{os.getpid()}.{job}.{len(params)}"
    env = dict(os.environ, ABY3_LINK_TIMEOUT_S="120", ABY3_WARMUP_STEPS=str(warmup))
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "party_worker.py"), str(job), str(p),
                               str(steps), link, "0", ",".join(str(x) for x in params), str(layout)],
                              stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True, env=env)
             for p in range(3)]
    outs = []
    for p in procs:
        o, e = p.communicate(timeout=300)
        if p.returncode != 0:
            raise SystemExit("bench: party process failed: " + e[-2000:])
        outs.append(json.loads(o.strip().splitlines()[-1]))
    if not all(o["ok"] for o in outs):
        raise SystemExit("bench: party-process result differs from the plaintext")
    return max(o["ms_per_step"] for o in outs), outs


def cpu_msb(nt, rows, reps):
    """The oracle's 3-party fetch_msb on this host: evaluations per second
    (cpu_baseline leg only)."""
    import ctypes

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle as orc

    args, keep = orc._cir_args(nt.circuit("int_comp_helper", 64))
    f = orc.dll().orc_bench_fetch_msb
    f.restype = ctypes.c_double
    secs = f(*args, ctypes.c_uint64(rows), reps)
    if secs < 0:
        raise SystemExit("bench: oracle fetch_msb baseline failed: " + orc.dll().orc_last_error().decode())
    return reps / secs


def cpu_lr_ms(nt, iters):
    """The oracle's LR iteration on this host (cpu_baseline leg only)."""
    import ctypes

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle as orc

    args, keep = orc._cir_args(nt.circuit("int_Sh3Piecewise_helper", 64, 2))
    f = orc.dll().orc_bench_lr
    f.restype = ctypes.c_double
    u = ctypes.c_uint64
    secs = f(*args, u(65536), u(128), u(256), u(16), u(11), iters)
    if secs < 0:
        raise SystemExit("bench: oracle LR baseline failed: " + orc.dll().orc_last_error().decode())
    return secs / iters * 1e3


def cpu_conversion_rates(nt):
    """The oracle's toBinaryMatrix / bitInjection on this host (cpu_baseline legs
    only): values/s and bits/s, three parties in sequence on one thread."""
    import ctypes

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle as orc

    u = ctypes.c_uint64
    # the engine's A->B circuit for 64 bits is the one 64-bit adder (int_int_add)
    args, keep = orc._cir_args(nt.circuit("int_int_add", 64))
    f = orc.dll().orc_bench_a2b
    f.restype = ctypes.c_double
    a2b_n, a2b_reps = 1 << 20, 2
    secs = f(*args, u(a2b_n), a2b_reps)
    g = orc.dll().orc_bench_bitinj
    g.restype = ctypes.c_double
    bi_rows, bi_reps = 1 << 16, 2
    secs2 = g(u(bi_rows), u(64), bi_reps)
    if secs < 0 or secs2 < 0:
        raise SystemExit("bench: oracle conversion baseline failed: " + orc.dll().orc_last_error().decode())
    return (a2b_n * a2b_reps / secs, f"{a2b_reps} x toBinaryMatrix of {a2b_n} values"), \
           (bi_rows * 64 * bi_reps / secs2, f"{bi_reps} x bitInjection of {bi_rows}x64 bits")


def cpu_sort_rate(nt):
    """The oracle's batched odd-even merge sort on this host (cpu_baseline leg
    only), AND word-gates/s over a 2^16-key sort, three parties in sequence
    on one thread."""
    import ctypes

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle as orc

    import numpy as np

    n = 1 << 16
    args, keep = orc._cir_args(nt.circuit("cmp_swap", 64))
    f = orc.dll().orc_bench_sort
    f.restype = ctypes.c_double
    secs = f(*args, ctypes.c_uint64(n))
    if secs < 0:
        raise SystemExit("bench: oracle sort baseline failed: " + orc.dll().orc_last_error().decode())
    cir = nt.circuit("cmp_swap", 64)
    ands = sum(1 for g in np.asarray(cir["gates"]).reshape(-1, 4) if g[3] in (2, 3, 4, 5))
    words = 0
    for lv in range(16):  # 2^(15 - lv) merges of two lists of 2^lv keys, 1 + lv rounds
        L = 1 << lv
        words += sum(math.ceil((1 << (15 - lv)) * c / 64) for c in _round_pairs(L))
    return ands * words / secs, (f"1 x odd_even_merge_sort of {n} keys (oracle restatement: bit-sliced u64 "
                                 "cmp_swap rounds, AES-NI z masks, 3 parties on one thread)")


def _round_pairs(L):
    """Pairs per merge in each round of the merge of two lists of L keys
    (Sort.cpp:361-398)."""
    t = math.ceil(math.log2(L) + 1)
    q, d, r, out = 2 ** (t - 1), 1, 0, []
    while d > 0:
        out.append(max(0, (2 * L - d - r + 1) // 2))
        d, q, r = q - 1, q >> 1, 1
    return out


def extras(args, nt, dev, world, pg):
    """C4 (one SGD_Logistic iteration, 10^6 x 128, B=256, D16) and C5 (the
    whole odd-even merge sort of 2^20 keys), each checked."""
    res = {}
    with nt.Session(nt.JOB_LR, [args.lr_rows, 128, 256, 16, 11], devices=(dev,) * 3, probe=False) as s:
        s.run(20)
        dt = timed(s, LR_ITERS, pg, secs=args.prewarm_s)
        linfo = s.info()
        if not s.check():
            raise SystemExit("bench: LR model differs from the plaintext fixed-point restatement")
        res["lr_iteration"] = {
            "workload": f"SGD_Logistic iteration, {args.lr_rows}x128, batch 256, D16, lr 2^-11 (sigmoid piecewise)",
            "ms_per_iteration": dt / LR_ITERS * 1e3,
            "iterations_per_s": world * LR_ITERS / dt,
        }
        res["lr_iteration"]["local_compute"] = compute_fraction(nt, nt.JOB_LR, [args.lr_rows, 128, 256, 16, 11],
                                                                dev, 100)
        if world == 1 and not args.no_cpu_baseline:
            progress("C4 CPU baseline")
            cpu_ms = cpu_lr_ms(nt, iters=200)
            res["lr_iteration"]["cpu_baseline"] = {
                "value": cpu_ms, "unit": "ms/iteration", "cores": 1, "kind": "port",
                "sample": "200 iterations of the oracle's SGD_Logistic restatement (65536x128 dataset, batch 256, "
                          "D16, aB 11), the three parties simulated in sequence on one thread, no network",
            }
            res["lr_iteration"]["speedup_vs_cpu_baseline"] = cpu_ms / (dt / LR_ITERS * 1e3)
    # C4 as the reference times it (main-logistic.cpp:163-167 over SGD_Logistic,
    # Regression.h:249-293): whole epochs with getSubset in every iteration
    epoch_iters = -(-args.lr_rows // 256)
    with nt.Session(nt.JOB_LR, [args.lr_rows, 128, 256, 16, 11, 1], devices=(dev,) * 3, probe=False) as s:
        s.run(20)
        dt = timed(s, epoch_iters, pg, secs=args.prewarm_s)
        if not s.check():
            raise SystemExit("bench: LR (getSubset per iteration) model differs from the plaintext restatement")
        res["lr_epoch"] = {
            "workload": f"one epoch of SGD_Logistic: {epoch_iters} iterations over {args.lr_rows}x128, batch 256, "
                        "each drawing its mini-batch with getSubset (the pool resident in HBM; the next epoch's "
                        "reshuffle on a host thread during the current one, uploaded when the pool runs out)",
            "iterations": epoch_iters,
            "ms_per_epoch": dt * 1e3,
            "ms_per_iteration": dt / epoch_iters * 1e3,
            "iterations_per_s": world * epoch_iters / dt,
        }
        if world == 1 and not args.no_cpu_baseline:
            progress("C4 epoch CPU baseline")
            cpu_ms = cpu_lr_ms(nt, iters=512)
            res["lr_epoch"]["cpu_baseline"] = {
                "value": 1e3 / cpu_ms, "unit": "iterations/s", "cores": 1, "kind": "port",
                "sample": "512 iterations (two epochs, two reshuffles of the pool) of the oracle's SGD_Logistic "
                          "restatement with getSubset per iteration (65536x128 dataset, batch 256, D16, aB 11), the "
                          "three parties simulated in sequence on one thread, no network",
            }
            res["lr_epoch"]["speedup_vs_cpu_baseline"] = res["lr_epoch"]["iterations_per_s"] / (1e3 / cpu_ms)
    with nt.Session(nt.JOB_SORT, [1 << 20], devices=(dev,) * 3, probe=False) as s:
        s.run(1)
        reps = 2
        dt = timed(s, reps, pg)  # one sort is ~70 ms of load: its own warm-up
        if not s.check():
            raise SystemExit("bench: merge sort output differs from std::sort of the keys")
        info = s.info()
        res["merge_sort"] = {
            "workload": "odd_even_merge_sort of 2^20 64-bit keys: 20 multi-merge levels, 210 rounds, every round "
                        "one cmp_swap evaluation over its 2^19 compare-exchanges (gather/scatter fused into the "
                        "transposes), 3 parties",
            "ms_per_sort": dt / reps * 1e3,
            "keys_per_s": world * reps * (1 << 20) / dt,
            "and_words_per_sort": info["and_words"],
            "and_word_gates_per_s": world * reps * info["and_words"] / dt,
        }
        if world == 1 and not args.no_cpu_baseline:
            progress("C5 CPU baseline")
            rate, sample = cpu_sort_rate(nt)
            res["merge_sort"]["cpu_baseline"] = {
                "value": rate, "unit": "AND word-gates/s", "cores": 1, "kind": "port", "sample": sample,
                "est_full_sort_s": info["and_words"] / rate,
            }
            res["merge_sort"]["speedup_vs_cpu_baseline"] = res["merge_sort"]["and_word_gates_per_s"] / rate
    # The reference's own merge order (Sort.cpp:413-437: odd_even_multi_merge
    # calls odd_even_merge for one pair after the other), whose randomness
    # draws -- and so shares -- the batched form does not reproduce: priced at
    # 2^14 keys, beside the batched order at the same size.
    seq_keys = 1 << 14
    seq = {"workload": f"odd_even_merge_sort of {seq_keys} 64-bit keys in the reference's order "
                       "(MergeOrder::Sequential: every pairwise merge its own cmp_swap evaluations, one after "
                       "the other), 3 parties; beside it the batched order at the same size", "keys": seq_keys}
    for order, name in ((1, "sequential"), (0, "batched")):
        with nt.Session(nt.JOB_SORT, [seq_keys, order], devices=(dev,) * 3, probe=False) as s:
            s.run(1)
            reps = 1 if order else 20
            dt = timed(s, reps, pg)
            if not s.check():
                raise SystemExit(f"bench: {name} merge sort output differs from std::sort of the keys")
            info = s.info()
            seq[name] = {"ms_per_sort": dt / reps * 1e3, "and_words_per_sort": info["and_words"],
                         "and_word_gates_per_s": world * reps * info["and_words"] / dt}
    seq["sequential_over_batched"] = seq["sequential"]["ms_per_sort"] / seq["batched"]["ms_per_sort"]
    res["merge_sort"]["sequential"] = seq
    # C1: asyncMul 128x128, both modes, no truncation
    res["c1_mul"] = {}
    for mode, name in ((0, "hadamard"), (1, "gemm")):
        with nt.Session(nt.JOB_MUL, [128, 128, 128, mode], devices=(dev,) * 3, probe=False) as s:
            s.run(20)
            if not s.check():
                raise SystemExit("bench: C1 product differs from the plaintext")
            reps = 500
            dt = timed(s, reps, pg, secs=args.prewarm_s)
            mults = 128 * 128 * (128 if mode else 1)
            e = {"workload": f"asyncMul 128x128 si64 ({name}{', 128x128x128' if mode else ''}), 3 parties",
                 "ms_per_mul": dt / reps * 1e3, "mults_per_s": world * reps * mults / dt}
            if world == 1 and not args.no_cpu_baseline:
                n_cpu = 2000 if mode == 0 else 300
                cpu_s = cpu_mul_procs_s(mode, n_cpu)
                e["cpu_baseline"] = {
                    "value": mults / cpu_s, "unit": "mults/s", "cores": 3, "kind": "port",
                    "sample": f"{n_cpu} x asyncMul 128x128 ({name}) as configs[0] states it: three CPU processes, one "
                              "party each (oracle/build/orc_c1_procs), each computing its local share product + "
                              "zero-share and sending it to the next party through a shared-memory mailbox (a copy "
                              "in and a copy out, as through a localhost socket)"}
                e["cpu_baseline_threads"] = {
                    "value": mults / cpu_mul_s(mode, n_cpu), "unit": "mults/s", "cores": 3,
                    "sample": "the same with the parties as three threads of one process, the reshare a copy"}
                e["speedup_vs_cpu_baseline"] = e["mults_per_s"] / e["cpu_baseline"]["value"]
            res["c1_mul"][name] = e
    # share conversions, each checked on its revealed output
    with nt.Session(nt.JOB_A2B, [1 << 20], devices=(dev,) * 3, probe=False) as s:
        s.run(2)
        dt = timed(s, 10, pg, secs=args.prewarm_s)
        if not s.check():
            raise SystemExit("bench: toBinaryMatrix output differs from the input")
        info = s.info()
        res["a2b"] = {
            "workload": "Sh3Converter::toBinaryMatrix of 2^20 64-bit values (resharing + 64-bit adder circuit)",
            "ms_per_conversion": dt / 10 * 1e3,
            "values_per_s": world * 10 * (1 << 20) / dt,
            "and_word_gates_per_s": world * 10 * info["and_words"] / dt,
        }
    cpu_conv = None
    if world == 1 and not args.no_cpu_baseline:
        progress("conversion CPU baselines")
        cpu_conv = cpu_conversion_rates(nt)
        res["a2b"]["cpu_baseline"] = {
            "value": cpu_conv[0][0], "unit": "values/s", "cores": 1, "kind": "port",
            "sample": cpu_conv[0][1] + " (oracle restatement: AES-NI streams, bit-sliced adder, 3 parties on one thread)",
        }
        res["a2b"]["speedup_vs_cpu_baseline"] = res["a2b"]["values_per_s"] / cpu_conv[0][0]
    with nt.Session(nt.JOB_BITINJ, [1 << 16, 64], devices=(dev,) * 3, probe=False) as s:
        s.run(2)
        dt = timed(s, 10, pg, secs=args.prewarm_s)
        if not s.check():
            raise SystemExit("bench: bitInjection output differs from the input bits")
        res["bit_injection"] = {
            "workload": "Sh3Converter::bitInjection of 2^16 x 64 bits (3-party OT per bit, one round + OT)",
            "ms_per_conversion": dt / 10 * 1e3,
            "bits_per_s": world * 10 * (1 << 16) * 64 / dt,
        }
        if cpu_conv:
            res["bit_injection"]["cpu_baseline"] = {
                "value": cpu_conv[1][0], "unit": "bits/s", "cores": 1, "kind": "port",
                "sample": cpu_conv[1][1] + " (oracle restatement: AES-NI OT pads, 3 parties on one thread)",
            }
            res["bit_injection"]["speedup_vs_cpu_baseline"] = res["bit_injection"]["bits_per_s"] / cpu_conv[1][0]
    return res


def main_parties(args, world, rank, local, pg, nt):
    """--deployment parties: ranks 3g, 3g+1, 3g+2 are parties 0, 1, 2 of job g,
    each on its own GPU (local rank modulo the visible devices), messages
    over shared-memory links and IPC device slots (peer reads over xGMI)."""
    import ctypes

    if world % 3:
        raise SystemExit("bench: --deployment parties needs a world size that is a multiple of 3")
    n = ctypes.c_int(0)
    nt.lib().device_count(ctypes.byref(n))
    dev = local % max(n.value, 1)
    party, group = rank % 3, rank // 3
    colocated = n.value < 3
    M, K, N, D = args.m, args.k, args.n, args.decimal
    # a per-launch nonce in the link name (rank 0's, broadcast): a rerun never
    # attaches to a segment a killed run left behind under the same port
    nonce = [os.urandom(4).hex()]
    if pg is not None:
        pg.broadcast_object_list(nonce, src=0)
    link = f"bench{os.environ.get('MASTER_PORT', '0')}.{nonce[0]}.{group}"
    s = nt.Session.party(nt.JOB_MUL_TRUNC, [M, K, N, D, 1], party, link, device=dev, colocated=colocated)
    s.run(2)
    ok = s.check()
    if allmax(pg, 0.0 if ok else 1.0) > 0:
        raise SystemExit("bench: revealed product does not match the plaintext")
    dt = timed(s, args.steps, pg, secs=args.prewarm_s, warmup=args.warmup)
    info = s.info()
    s.close()
    groups = world // 3
    out = {
        "metric": "secret-shared 64-bit mults/sec (matmul + binary-AND) per party, 3 parties on 3 MI355X",
        "value": groups * args.steps * info["mults_per_step"] / dt,
        "unit": "mults/s",
        "n_gpus": world if not colocated else n.value,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "int64",
        "data": "synthetic: fixed-point operands round(U[-8,8) * 2^16), shared by party 0",
        "config": {
            "workload": f"sf64Matrix asyncMul + truncation {M}x{K} . {K}x{N} (D{D}), upstream GEMM semantics, "
                        "one party per process" + (" (processes sharing a GPU)" if colocated else " and GPU"),
            "parties_per_gpu": 3 if colocated else 1,
            "global_batch": groups,
            "parallelism": f"parties3x{groups}",
        },
        "host_recv_wait_us_per_step": info["host_recv_wait_us"],
    }
    if rank == 0:
        print(json.dumps(out))
    if pg is not None:
        pg.destroy_process_group()


def main_rowsplit(args, world, rank, local, pg, nt):
    """--deployment rowsplit: rank r runs rows [r*M/N, (r+1)*M/N) of ONE C2
    product as a three-party job on its GPU (ABY3H_JOB_MUL_TRUNC's shard
    parameters: every slice's shares are those rows of the unsplit product's,
    tests/test_gpu_rowsplit.py); no exchange between the ranks' jobs. A step
    is the whole product: value = M*N*K / the slowest rank's time."""
    import ctypes

    n = ctypes.c_int(0)
    nt.lib().device_count(ctypes.byref(n))
    dev = local % max(n.value, 1)
    M, K, N, D = args.m, args.k, args.n, args.decimal
    s = nt.Session(nt.JOB_MUL_TRUNC, [M, K, N, D, 1, 1, rank, world], devices=(dev, dev, dev), probe=False)
    s.run(2)
    ok = s.check()
    if allmax(pg, 0.0 if ok else 1.0) > 0:
        raise SystemExit("bench: revealed product slice does not match the plaintext")
    dt = timed(s, args.steps, pg, secs=args.prewarm_s, warmup=args.warmup)
    s.close()
    out = {
        "metric": "secret-shared 64-bit mults/sec (matmul + binary-AND) per party, 3 parties on 3 MI355X",
        "value": args.steps * M * N * K / dt,
        "unit": "mults/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "int64",
        "data": "synthetic: fixed-point operands round(U[-8,8) * 2^16), shared by party 0",
        "config": {
            "workload": f"sf64Matrix asyncMul + truncation {M}x{K} . {K}x{N} (D{D}), upstream GEMM semantics, "
                        f"the product's rows split over {world} GPU(s), each slice 3 parties co-located",
            "parties_per_gpu": 3,
            "global_batch": 1,
            "parallelism": f"rowsplit{world}",
        },
    }
    if rank == 0:
        print(json.dumps(out))
    if pg is not None:
        pg.destroy_process_group()


def main():
    args = parse()
    world, rank, local, pg = dist_setup()
    from aby3_amd import native as nt

    if args.dump_outputs and args.deployment != "replicas":
        raise SystemExit("bench: --dump-outputs writes the replicas deployment's product only")
    if args.deployment == "parties":
        return main_parties(args, world, rank, local, pg, nt)
    if args.deployment == "rowsplit":
        return main_rowsplit(args, world, rank, local, pg, nt)

    import ctypes

    ndev = ctypes.c_int(0)
    nt.lib().device_count(ctypes.byref(ndev))
    dev = local % max(ndev.value, 1)  # one GPU per rank, also when each rank sees only its own
    M, K, N, D = args.m, args.k, args.n, args.decimal
    if args.gemm_turns:
        nt.lib().mfma_turn(1)
    # only the share-GEMM launches carry timing events (the roofline kernel);
    # digit and epilogue times come from a second, separately probed pass.
    # A plain run keeps those events although only --full reports them: the
    # timed steps are the same steps with and without --full
    progress("C2 asyncMul + truncation session")
    sess = nt.Session(nt.JOB_MUL_TRUNC, [M, K, N, D, 1], devices=(dev, dev, dev), probe=1 << nt.PROBE_GEMM)
    # correctness first (--full), then the warmup steps right before the timed
    # region (a host-side reveal between warmup and timing lets the clocks drop)
    sess.run(2)
    if args.full and not sess.check():
        raise SystemExit("bench: revealed product does not match the plaintext")
    # time-based pre-warm, then the W warmup steps right before the timed region
    # (after the host-side reveal the clocks have dropped; ~50 ms of steps
    # bring them back: scripts/steady_state.py)
    t_pw = time.perf_counter()
    prewarm_steps = prewarm(sess, args.prewarm_s)
    if args.dump_outputs and prewarm_steps:
        # every step advances the parties' randomness, which decides the
        # last bit of the truncation: top the time-based count up to a fixed
        # one, so that the last step's product is the same from run to run
        # (a smaller quantum where the steps are long: at most 4 s of them)
        quantum, step_s = DUMP_STEP_QUANTUM, (time.perf_counter() - t_pw) / prewarm_steps
        while quantum > 1 and quantum * step_s > 4.0:
            quantum //= 4
        pad = -prewarm_steps % quantum
        if pad:
            sess.run(pad)
        prewarm_steps += pad
    prewarm_s = time.perf_counter() - t_pw
    sess.run(args.warmup)
    sess.probe_reset()
    barrier(pg)
    t0 = time.perf_counter()
    sess.run(args.steps)  # returns after every party stream drained
    t1 = time.perf_counter()
    barrier(pg)
    dt = allmax(pg, t1 - t0)
    info = sess.info()
    ovl_ms, ovl_n = sess.probe(nt.PROBE_GEMM)
    if args.dump_outputs and rank == 0:
        dump_outputs(sess, args.dump_outputs, M, N, D)
    sess.close()

    mults = info["mults_per_step"]
    value = world * args.steps * mults / dt
    out = {
        "metric": "secret-shared 64-bit mults/sec (matmul + binary-AND) per party, 3 parties on 3 MI355X",
        "value": value,
        "unit": "mults/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "warmup_s": prewarm_s,
        "prewarm_steps": prewarm_steps,
        "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "int64",
        "data": "synthetic: fixed-point operands round(U[-8,8) * 2^16), shared by party 0",
        "config": {
            "workload": f"sf64Matrix asyncMul + truncation {M}x{K} . {K}x{N} (D{D}), upstream GEMM semantics, "
                        "3 parties co-located per GPU",
            "parties_per_gpu": 3,
            "global_batch": world,
            "parallelism": f"replicas{world}",
        },
        "host_recv_wait_us_per_step": info["host_recv_wait_us"],
    }
    if not args.full:
        if rank == 0:
            print(json.dumps(out))
        if pg is not None:
            pg.destroy_process_group()
        return

    # Roofline pass: in the timed region the three co-located parties' GEMMs
    # overlap on the one GPU (faster together), so a launch's span there also
    # covers the CUs spent on the other two; here they take turns and each
    # launch's HIP-event span is the kernel's own duration.
    progress("C2 roofline pass (GEMMs take turns)")
    nt.lib().mfma_turn(1)
    with nt.Session(nt.JOB_MUL_TRUNC, [M, K, N, D, 1], devices=(dev, dev, dev), probe=1 << nt.PROBE_GEMM) as rp:
        rp.run(5)
        prewarm(rp, 0.2)
        rp.probe_reset()
        rp.run(30)
        gemm_ms, gemm_n = rp.probe(nt.PROBE_GEMM)
    nt.lib().mfma_turn(1 if args.gemm_turns else 0)
    # kernel-time breakdown and the device-side local-compute fraction from a
    # separate pass with every family probed (event pairs around every launch
    # perturb the timing, so not the timed run)
    c2_local = compute_fraction(nt, nt.JOB_MUL_TRUNC, [M, K, N, D, 1], dev, 10)
    breakdown = {name: c2_local["family_ms_per_step"][fam] for name, fam in
                 (("share_gemm", nt.PROBE_GEMM), ("digit_planes", nt.PROBE_DIGITS),
                  ("trunc_epilogue", nt.PROBE_EPILOGUE))}
    gemm_avg_s = gemm_ms / max(gemm_n, 1) / 1e3
    achieved_tops = info["gemm_int8_ops"] / gemm_avg_s / 1e12 if gemm_avg_s > 0 else 0.0
    cfg = {"m": M, "k": K, "n": N}
    traffic = load_pmc("share_gemm", cfg)
    out.update({
        "roofline": {
            "bound": "mfma",
            "kernel": "k_share_gemm16s (int8 MFMA 16x16x64, 36 digit pairs as 20 two-pair MFMAs per block and stage)",
            "achieved": achieved_tops,
            "peak": PEAK_INT8_TOPS,
            "unit": "TOP/s",
            "frac": achieved_tops / PEAK_INT8_TOPS,
            "traffic": traffic,
            "traffic_unit": "HBM bytes per launch (rocprofv3 FETCH_SIZE x2 + WRITE_SIZE, profiles/pmc_*.json)",
            "launch_ms": gemm_avg_s * 1e3,
            "launch_ms_measured": "HIP events around every share-GEMM launch of a 30-step pass whose co-located "
                                  "parties' GEMMs take turns (aby3g_mfma_turn); in the timed region they overlap. "
                                  "Co-located parties plan each GEMM for a third of the chip "
                                  "(aby3g_set_gemm_sharing(3): 128 workgroups of 128x64 tiles, one K split at "
                                  "1024^3), so a launch alone leaves half the CUs to the other parties' kernels",
            # the launch's own CUs: one 128 x 64 tile per workgroup and CU
            # (one K split at this size), so the peak it can reach alone is
            # that share of the chip's
            "cus_used": min(256, -(-M // 128) * -(-N // 64)),
            "frac_of_cus_used": achieved_tops / (PEAK_INT8_TOPS * min(256, -(-M // 128) * -(-N // 64)) / 256),
            "job_mfma_rate": info["gemm_int8_ops"] * 3 / (dt / args.steps) / 1e12,
            "job_mfma_rate_unit": "TOP/s: the three parties' share-GEMM int8 ops per step / the whole step",
            "launch_span_ms_overlapped": ovl_ms / max(ovl_n, 1),
            "ops_per_launch": info["gemm_int8_ops"],
            # MFMA utilisation from the committed PMC pass of the same job
            # (scripts/gemm_mfma_pmc.sh: SQ_VALU_MFMA_BUSY_CYCLES and the
            # effective clock, GRBM_GUI_ACTIVE / 8 / wall), if there is one
            "mfma_utilisation": load_mfma(cfg),
        },
        "kernel_ms_per_step": breakdown,
        # share of the wall clock a party's GPU stream spends computing (its
        # kernels, minus their in-kernel waits for peers), from a probed pass
        "local_compute_fraction": c2_local["local_compute_fraction"],
        "local_compute": c2_local,
    })

    if not args.no_binary:
        progress("C3 binary session")
        # the timed run carries no probes (event pairs around every level
        # launch would add host work per level); the gate kernels' time comes
        # from the separate probed pass of compute_fraction
        bs = nt.Session(nt.JOB_MSB, [args.binary_rows], devices=(dev, dev, dev), probe=False)
        bs.run(1)
        if not bs.check():
            raise SystemExit("bench: binary MSB result does not match the plaintext")
        prewarm(bs, args.prewarm_s)
        bs.run(4)
        barrier(pg)
        b0 = time.perf_counter()
        bs.run(args.binary_steps)
        b1 = time.perf_counter()
        barrier(pg)
        bdt = allmax(pg, b1 - b0)
        binfo = bs.info()
        bs.close()
        c3_local = compute_fraction(nt, nt.JOB_MSB, [args.binary_rows], dev, args.binary_steps)
        gate_s = c3_local["family_ms_per_step"][nt.PROBE_BINARY] / 3 / 1e3  # per party per step
        gbs = binfo["gate_bytes"] / gate_s / 1e9 if gate_s > 0 else 0.0
        out["binary"] = {
            "workload": f"cipher_gt / fetch_msb over {args.binary_rows} rows (MSB(a+b) circuit), 3 parties",
            "value": world * args.binary_steps * binfo["and_words"] / bdt,
            "unit": "AND word-gates/s (1 AND-type gate on one 64-row word)",
            "ms_per_step": bdt / args.binary_steps * 1e3,
            "and_words_per_step": binfo["and_words"],
            "local_compute": c3_local,
            "roofline": {
                "bound": "hbm",
                "kernel": "k_bin_level (one launch per level: unpack of the received AND shares + the level's gate batches)",
                "achieved": gbs,
                "peak": PEAK_HBM_GBS,
                "unit": "GB/s",
                "frac": gbs / PEAK_HBM_GBS,
                "traffic": load_pmc("bin_gates", {"rows": args.binary_rows}, "hbm_bytes_per_step_per_party"),
                "traffic_unit": "HBM bytes per step per party (rocprofv3 FETCH_SIZE/WRITE_SIZE)",
                "bytes_per_step_per_party": binfo["gate_bytes"],
            },
        }
        if rank == 0 and world == 1 and not args.no_cpu_baseline:
            progress("C3 CPU baseline")
            cpu = cpu_msb(nt, args.binary_cpu_rows, reps=1)
            out["binary"]["cpu_baseline"] = {
                "value": cpu * binfo["and_words"] * args.binary_cpu_rows / args.binary_rows,
                "unit": "AND word-gates/s",
                "cores": 1,
                "kind": "port",
                "sample": f"1 x cipher_gt over {args.binary_cpu_rows} rows: the oracle's 3-party fetch_msb "
                          "(bit-sliced u64 gate loops, AES-NI z masks, reference Release flags), the three "
                          "parties simulated in sequence on one thread, no network",
            }
            out["binary"]["speedup_vs_cpu_baseline"] = out["binary"]["value"] / out["binary"]["cpu_baseline"]["value"]

    if not args.no_extras:
        progress("C4 / C5 extras")
        out["extras"] = extras(args, nt, dev, world, pg)
        if world == 1:
            progress("C2 / C3 / C4 as three party processes")
            pp = {}
            ms, outs = party_job(nt.JOB_MUL_TRUNC, [M, K, N, D, 1], 30, warmup=100)
            pp["c2"] = {
                "workload": "the C2 multiplication, each party in its own process (aby3h_party_create), all three "
                            "on GPU 0, messages over shared-memory links + IPC device staging slots",
                "ms_per_step": ms,
                "mults_per_s": M * N * K / (ms * 1e-3),
                "recv_wait_us_per_step": [o["recv_wait_us"] for o in sorted(outs, key=lambda o: o["party"])],
            }
            ms, outs = party_job(nt.JOB_MSB, [args.binary_rows], 30, warmup=50)
            pp["c3"] = {"workload": f"cipher_gt over {args.binary_rows} rows, one party per process",
                        "ms_per_step": ms}
            ms, outs = party_job(nt.JOB_LR, [args.lr_rows, 128, 256, 16, 11], LR_ITERS, warmup=1000)
            pp["c4"] = {"workload": f"SGD_Logistic iteration, {args.lr_rows}x128, batch 256, one party per process "
                                    "(the fused launch over IPC-mapped mailboxes)",
                        "ms_per_iteration": ms,
                        "fused": all(o["lr_fused"] == 1 for o in outs)}
            # the three-GPU layout's branches on this GPU (aby3h_party_create
            # colocated = 2): uncached mailboxes + system-scope messages for the
            # fused iteration, staged IPC copies for every C2 device message
            ms, outs = party_job(nt.JOB_LR, [args.lr_rows, 128, 256, 16, 11], LR_ITERS, warmup=1000, layout=2)
            pp["c4_remote_branches"] = {
                "workload": f"SGD_Logistic iteration, {args.lr_rows}x128, batch 256, one party per process, the "
                            "cross-GPU branches forced on GPU 0 (uncached mailboxes, system-scope messages)",
                "ms_per_iteration": ms,
                "fused": all(o["lr_fused"] == 1 for o in outs),
                "sys_scope": all(o["lr_sys_scope"] == 1 for o in outs)}
            ms, outs = party_job(nt.JOB_MUL_TRUNC, [M, K, N, D, 1], 30, warmup=100, layout=2)
            pp["c2_remote_branches"] = {
                "workload": "the C2 multiplication, one party per process, the cross-GPU branches forced on GPU 0 "
                            "(every z message a staged copy out of the sender's IPC slot, no arenas)",
                "ms_per_step": ms}
            out["extras"]["party_processes"] = pp
            # the verdict's flat keys
            pp["ms_per_step"] = pp["c2"]["ms_per_step"]
            pp["lr_ms_per_iteration"] = pp["c4"]["ms_per_iteration"]
            pp["c3_ms_per_step"] = pp["c3"]["ms_per_step"]

    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        import ctypes

        orc = ctypes.CDLL(os.path.join(ROOT, "oracle", "build", "liborc.so"))
        orc.orc_bench_mul_trunc.restype = ctypes.c_double
        reps = args.cpu_reps
        progress("C2 CPU baseline")
        secs = orc.orc_bench_mul_trunc(1, M, K, N, D, reps)
        out["cpu_baseline"] = {
            "value": reps * M * N * K / secs,
            "unit": "mults/s",
            "cores": 3,
            "kind": "port",
            "sample": f"{reps} x asyncMul+trunc {M}x{K}x{N}: three scalar i64 GEMMs (Eigen-style, "
                      "reference Release flags) + AES-NI truncation pair per party, 3 party threads",
            "cpu": open("/proc/cpuinfo").read().split("model name")[1].split("\n")[0].strip(": \t")
            if os.path.exists("/proc/cpuinfo") else "unknown",
        }
        out["speedup_vs_cpu_baseline"] = value / out["cpu_baseline"]["value"]

    if rank == 0:
        print(json.dumps(out))
    if pg is not None:
        pg.destroy_process_group()


if __name__ == "__main__":
    main()
