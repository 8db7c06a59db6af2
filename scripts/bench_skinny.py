"""Skinny share products (N <= 8 columns) through the C-ABI: the streaming
skinny route (aby3g_skinny_route 2) against the kernels it replaces (route 1)
and the automatic choice (route 0), one stream, no co-located parties.

    python scripts/bench_skinny.py [--out profiles/skinny_route.json] [MxKxN ...]

The driver runs each group of shapes in a child process of its own under
`timeout`, and stops at the first child that fails. A child (--worker) times
aby3g_mul_local (no zero-share) and aby3g_mul_trunc_local (d = 16) with device
events: 3 warm-up calls per route, then --reps timed calls per route,
the routes alternating call by call, the median reported. It first checks that
the routes' outputs are bit-identical. `a_gbs` is the A bytes (2 shares x M x
K x 8) over the median time: the tall form's share of the HBM rate.

--parent-root DIR names a built checkout of the parent commit: its library is
timed in one more child process at PARENT_SHAPES (a tree without
aby3g_skinny_route has one route, "parent") and the rows go to `parent_rows`
of the output, to confirm that route 1 is the parent's code path. (--root DIR
is what that child uses: it imports aby3_amd from DIR.)
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

GROUPS = {
    # the flagship tall shapes: 2^20 rows of dim 128 times 1..8 columns
    "tall": ["1048576x128x1", "1048576x128x2", "1048576x128x4", "1048576x128x8"],
    # long dots
    "long": ["1x1048576x1", "128x65536x1"],
    # around k_small_gemm's 2^23-term limit (tall) and K N around the LDS image of B (2048 terms)
    "tall_edges": ["65536x128x1", "65537x128x1", "8192x128x8", "8193x128x8", "4097x256x8", "4097x257x8",
                   "4096x4096x8", "1024x8192x1"],
    # around the long form's K (2^14) and M N (1024) limits
    "long_edges": ["1x16383x1", "1x16384x1", "1x32768x1", "1x131072x1", "64x32768x1", "512x16384x1",
                   "1024x16384x1", "1025x16384x1", "1024x32768x1"],
}
PARENT_SHAPES = ["1048576x128x1", "1x1048576x1"]
TIMEOUT_S = 240
NOTE = ("routes: old = aby3g_skinny_route(1) (k_small_gemm / the MFMA digit GEMM), skinny = route 2, auto = route 0; "
        "the three alternate call by call in one process. parent_rows: the parent commit's library "
        "(--parent-root), a process of its own.")


def worker(args):
    sys.path.insert(0, os.path.abspath(args.root))
    import torch

    from aby3_amd import native as nt

    L = nt.lib()
    L.set_device(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    routed = hasattr(L.dll, "aby3g_skinny_route")
    routes = [("old", 1), ("skinny", 2), ("auto", 0)] if routed else [("parent", None)]

    def set_route(r):
        if r is not None and L.dll.aby3g_skinny_route(r) != 0:
            raise RuntimeError("aby3g_skinny_route failed")

    ts = nt.TruncStreams()
    ts.next_seed[:] = bytes(range(16))
    ts.prev_seed[:] = bytes(range(16, 32))
    ts.next_off, ts.prev_off = 32, 40
    ev = []
    for _ in range(2):
        e = ctypes.c_void_p()
        L.event_create_timed(ctypes.byref(e))
        ev.append(e)
    results = []
    for shape in args.shapes.split(","):
        M, K, N = map(int, shape.split("x"))
        n = M * N
        g = torch.Generator(device="cuda").manual_seed(M + K + N)
        A = torch.randint(-2**63, 2**63 - 1, (2 * M * K,), dtype=torch.int64, device="cuda", generator=g)
        B = torch.randint(-2**63, 2**63 - 1, (2 * K * N,), dtype=torch.int64, device="cuda", generator=g)
        C0, z, C = (torch.empty(k * n, dtype=torch.int64, device="cuda") for k in (1, 1, 2))
        ws, wsb, form = {}, {}, {}
        for name, r in routes:
            set_route(r)
            wsb[name] = L.dll.aby3g_mul_workspace_bytes(1, M, K, N)
            ws[name] = torch.empty(wsb[name] // 8 + 1, dtype=torch.int64, device="cuda")
            form[name] = dict(workspace_bytes=wsb[name], prefers_fused=L.dll.aby3g_mul_prefers_fused(1, M, K, N))

        def call(op, name):
            if op == "mul_local":
                L.mul_local(1, P(A), P(B), P(C0), M, K, N, None, P(ws[name]), wsb[name], None)
            else:
                L.mul_trunc_local(1, P(A), P(B), M, K, N, 16, ctypes.byref(ts), P(z), P(C), P(ws[name]), wsb[name],
                                  None)

        # results must not change: every route's product and z, bit for bit
        ref = None
        for name, r in routes:
            set_route(r)
            call("mul_local", name)
            call("mul_trunc_local", name)
            torch.cuda.synchronize()
            got = (C0.clone(), z.clone(), C.clone())
            if ref is None:
                ref = got
            elif not all(torch.equal(a, b) for a, b in zip(ref, got)):
                raise RuntimeError(f"{shape}: route {name} computes other values")
        row = dict(shape=shape, M=M, K=K, N=N, a_bytes=16 * M * K, routes=form, reps=args.reps, us={}, a_gbs={})
        for op in ("mul_local", "mul_trunc_local"):
            times = {name: [] for name, _ in routes}
            for name, r in routes:
                set_route(r)
                for _ in range(3):
                    call(op, name)
            torch.cuda.synchronize()
            for _ in range(args.reps):
                for name, r in routes:
                    set_route(r)
                    L.event_record(ev[0], None)
                    call(op, name)
                    L.event_record(ev[1], None)
                    L.event_sync(ev[1])
                    ms = ctypes.c_float()
                    L.event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms))
                    times[name].append(ms.value * 1e3)
            row["us"][op] = {k: round(statistics.median(v), 2) for k, v in times.items()}
            row["a_gbs"][op] = {k: round(16 * M * K / (statistics.median(v) * 1e-6) / 1e9, 1) for k, v in times.items()}
        print(json.dumps(row), flush=True)
        results.append(row)
        del A, B, ws
        torch.cuda.empty_cache()
    set_route(0 if routed else None)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=results), f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes_list", nargs="*")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--shapes", default="")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    groups = {"cli": args.shapes_list} if args.shapes_list else GROUPS

    def child(gname, shapes, root):
        """One group of shapes in a process of its own under `timeout`: (status, device name, rows)."""
        part = (args.out or "skinny_route.json") + f".{gname}.part"
        cmd = ["timeout", "-k", "10", str(TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--worker", "--shapes",
               ",".join(shapes), "--root", root, "--reps", str(args.reps), "--out", part]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            # a fault, an abort or a time limit: nothing more is started on the GPU
            print(f"group {gname} ended with status {rc}; stopping", flush=True)
            return rc, None, []
        with open(part) as f:
            got = json.load(f)
        os.remove(part)
        return 0, got["device"], got["rows"]

    table, device = [], None
    for gname, shapes in groups.items():
        rc, device, rows = child(gname, shapes, args.root)
        if rc != 0:
            return rc
        table += [dict(group=gname, **row) for row in rows]
    out = dict(device=device, unit="us (median of device-event spans)", note=NOTE, rows=table)
    if args.parent_root:
        rc, _, out["parent_rows"] = child("parent", PARENT_SHAPES, args.parent_root)
        if rc != 0:
            return rc
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
