#!/usr/bin/env python3
"""ECDH key-derivation throughput (§8f row 4): fpnn_ecdh_calc_keys on the GPU -- one
server private key against N peer public keys, i.e. ECCKeyExchange::calcKey for N
accepted connections (config C5's 65 536-connection key table) -- against the reference's
own calcKey (core/KeyExchange.cpp + core/micro-ecc, oracle/_ref/ecdh_ref) on the host
cores, one process per core.

  python tools/bench_ecdh.py [--n 65536] [--reps 5] [--cpu-seconds 3]
Prints one JSON object (derivations/s per curve).

  python tools/bench_ecdh.py --accept [--n 65536] [--reps 7]
The "accept" row instead (accept_row below): the time from queueing the ECDH of n peers to
the end of the first package encrypt under their keys, through the host (calc_keys, copy
back, host key expansion, fpnn_aes_keyset_set) and on the device (fpnn_ecdh_accept).
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
ECDH_REF = os.path.join(ROOT, "oracle", "_ref", "ecdh_ref")


def gpu_rate(engine, curve: str, n: int, reps: int):
    import numpy as np
    import torch
    import fpnn_amd
    lib = fpnn_amd.lib
    cv = engine.ecdh_curve(curve)
    pl = lib.fpnn_ecdh_private_len(cv)
    rng = np.random.default_rng(n)
    privs = torch.from_numpy(rng.integers(0, 256, (n, pl), dtype=np.uint8)).to("cuda:0")
    privs[:, 0] &= 0x7F
    peers, ok = engine.ecdh_public_keys(curve, privs)  # setup, not timed
    server = bytes(rng.integers(1, 255, pl, dtype=np.uint8))
    torch.cuda.synchronize()
    engine.ecdh_calc_keys(curve, server, peers, 32)  # warm-up
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        keys, ivs, ok = engine.ecdh_calc_keys(curve, server, peers, 32)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    assert bool(ok.all())
    return n / best, best * 1e3


def gpu_percall(engine, curve: str, calls: int):
    """The drop-in per-call form (ECCKeyExchange::calcKey through fpnn_ecdh_calc_key_host:
    one peer, host buffers, synchronous): median microseconds per call."""
    import statistics
    import numpy as np
    import torch
    import fpnn_amd
    cv = engine.ecdh_curve(curve)
    pl = fpnn_amd.lib.fpnn_ecdh_private_len(cv)
    rng = np.random.default_rng(77)
    privs = torch.from_numpy(rng.integers(0, 256, (calls, pl), dtype=np.uint8)).to("cuda:0")
    privs[:, 0] &= 0x7F
    peers, _ = engine.ecdh_public_keys(curve, privs)
    peers = peers.cpu().numpy()
    server = bytes(rng.integers(1, 255, pl, dtype=np.uint8))
    engine.ecdh_calc_key_host(curve, server, peers[0].tobytes(), 32)  # warm-up (scratch)
    times = []
    for i in range(calls):
        p = peers[i].tobytes()
        t0 = time.perf_counter()
        engine.ecdh_calc_key_host(curve, server, p, 32)
        times.append(time.perf_counter() - t0)
    return statistics.median(times) * 1e6


def accept_row(engine, n: int, reps: int):
    """The "accept" row: n secp256k1 peers into a reserved AES-256 table, from the queue of
    the ECDH to the completion of a following 145-byte package encrypt that names every new
    slot, by two routes measured alternately in this one session (host clock around work that
    ends in a device synchronise):
      host    fpnn_ecdh_calc_keys -> device-to-host copy of (key, iv) -> one host
              fpnn_aes_setup_encrypt per connection -> fpnn_aes_keyset_set -> encrypt
      device  fpnn_ecdh_accept -> encrypt
    The host expansion is a Python loop over a ctypes call; the same loop over a C call that
    does nothing (fpnn_aes_keyset_nrounds(NULL)) is timed beside it and subtracted, so
    host_ms is the route less the interpreter's share (host_wall_ms keeps it)."""
    import ctypes as C
    import statistics
    import numpy as np
    import torch
    import fpnn_amd
    from fpnn_amd._lib import Schedule
    lib = fpnn_amd.lib
    curve, keylen, L = "secp256k1", 32, 145
    rng = np.random.default_rng(n + 1)
    privs = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).to("cuda:0")
    privs[:, 0] &= 0x7F
    peers, _ = engine.ecdh_public_keys(curve, privs)  # setup, not timed
    server = bytes(rng.integers(1, 255, 32, dtype=np.uint8))
    cv = engine.ecdh_curve(curve)
    engine.reserve(n, n * ((L + 15) // 16))
    tables = {r: fpnn_amd.KeySet.reserve(engine, n, keylen) for r in ("host", "device")}
    src = torch.from_numpy(rng.integers(0, 256, n * L, dtype=np.uint8)).to("cuda:0")
    dst = {r: torch.zeros(n * L, dtype=torch.uint8, device="cuda:0") for r in tables}
    slot = torch.arange(n, dtype=torch.int32, device="cuda:0")
    keys = torch.empty((n, keylen), dtype=torch.uint8, device="cuda:0")
    ivs = torch.empty((n, 16), dtype=torch.uint8, device="cuda:0")
    ok = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    ctx = (Schedule * n)()
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    u8p = C.POINTER(C.c_uint8)

    def encrypt(route):
        engine.package_encrypt(src, dst[route], n, tables[route], stride=L, uniform_len=L, key_slot=slot, max_len=L)

    def host_route():
        t0 = time.perf_counter()
        fpnn_amd.check(lib.fpnn_ecdh_calc_keys(engine.handle, cv, server, ptr(peers), n, keylen, ptr(keys), ptr(ivs),
                                               ptr(ok)), "calc_keys")
        hk, hi = keys.cpu().numpy(), ivs.cpu().numpy()  # (waits for the derivation)
        t1 = time.perf_counter()
        kp = hk.ctypes.data
        for i in range(n):
            lib.fpnn_aes_setup_encrypt(C.byref(ctx[i]), C.cast(kp + keylen * i, u8p), keylen)
        t2 = time.perf_counter()
        for i in range(n):  # the loop's own cost: the same argument work around a call that does nothing
            C.byref(ctx[i])
            C.cast(kp + keylen * i, u8p)
            lib.fpnn_aes_keyset_nrounds(None)
        t3 = time.perf_counter()
        fpnn_amd.check(lib.fpnn_aes_keyset_set(tables["host"].handle, 0, n, ctx, hi.ctypes.data_as(C.c_void_p)),
                       "keyset_set")
        tables["host"].count = n
        encrypt("host")
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        wall = t4 - t0 - (t3 - t2)  # the route as it ran (the do-nothing loop is no part of it)
        return wall - (t3 - t2), wall, (t1 - t0, (t2 - t1) - (t3 - t2), t4 - t3)  # less the interpreter's share

    def device_route():
        t0 = time.perf_counter()
        engine.ecdh_accept(curve, server, peers, tables["device"], ok=ok, count=n)
        encrypt("device")
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for _ in range(2):  # warm-up: code objects, scratch and tables at their final size
        host_route()
        device_route()
    assert torch.equal(dst["host"], dst["device"]) and bool(ok.all())
    host, wall, dev, parts = [], [], [], []
    for _ in range(reps):  # alternating
        h, w, p = host_route()
        host.append(h)
        wall.append(w)
        parts.append(p)
        dev.append(device_route())
    ms = lambda v: round(statistics.median(v) * 1e3, 3)  # noqa: E731
    for t in tables.values():
        t.close()
    return {"n": n, "reps": reps, "frame_bytes": L,
            "host_ms": ms(host), "host_ms_min": round(min(host) * 1e3, 3), "host_wall_ms": ms(wall),
            "host_parts_ms": {"derive_and_copy_back": ms([p[0] for p in parts]),
                              "host_expansion": ms([p[1] for p in parts]),
                              "upload_and_encrypt": ms([p[2] for p in parts])},
            "device_ms": ms(dev), "device_ms_min": round(min(dev) * 1e3, 3),
            "host_over_device": round(statistics.median(host) / statistics.median(dev), 2)}


def cpu_rate(curve: str, procs: int, seconds: float):
    """calcKey/s of the reference, `procs` processes in parallel (one per core)."""
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "ecdh_cases.json")))
    cv = next(c for c in g["curves"] if c["curve"] == curve)
    req = f"T {curve} {cv['server_private']} {cv['clients'][0]['public']} 50\n"
    t0 = time.perf_counter()
    r = subprocess.run([ECDH_REF], input=req, capture_output=True, text=True, check=True)
    one = float([ln for ln in r.stdout.splitlines() if ln.startswith("R ")][0].split()[1]) / 50
    reps = max(20, int(seconds / one))
    req = f"T {curve} {cv['server_private']} {cv['clients'][0]['public']} {reps}\n"
    t0 = time.perf_counter()
    ps = [subprocess.Popen([ECDH_REF], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True) for _ in range(procs)]
    for p in ps:
        p.stdin.write(req)
        p.stdin.close()
    for p in ps:
        p.wait()
    wall = time.perf_counter() - t0
    return procs * reps / wall, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-seconds", type=float, default=3.0)
    ap.add_argument("--curves", default="secp256k1,secp256r1,secp224r1,secp192r1")
    ap.add_argument("--no-cpu", action="store_true", help="skip the reference CPU legs (profiling runs)")
    ap.add_argument("--percall", type=int, default=0, help="also time this many single-peer calcKey calls")
    ap.add_argument("--accept", action="store_true",
                    help="only the accept row: ECDH -> live key table -> first encrypt, host route against device route")
    args = ap.parse_args()
    import fpnn_amd
    eng = fpnn_amd.Engine(0)
    if args.accept:
        print(json.dumps({"metric": "accept: ECDH queued -> 145-B package encrypt of every new slot done (ms)",
                          "accept": accept_row(eng, args.n, max(args.reps, 7))}))
        return
    cores = len(os.sched_getaffinity(0))
    try:
        quota = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota[0] != "max":
            cores = min(cores, max(1, int(int(quota[0]) / int(quota[1]))))
    except OSError:
        pass
    out = {"metric": "ECDH calcKey derivations/s", "n": args.n, "host_cores_used": cores, "curves": {}}
    for curve in args.curves.split(","):
        g, ms = gpu_rate(eng, curve, args.n, args.reps)
        row = {"gpu_per_s": round(g), "gpu_ms_per_batch": round(ms, 3)}
        if args.percall:
            row["gpu_percall_us_median"] = round(gpu_percall(eng, curve, args.percall), 1)
        if os.path.exists(ECDH_REF) and not args.no_cpu:
            c1, _ = cpu_rate(curve, 1, args.cpu_seconds)
            cn, _ = cpu_rate(curve, cores, args.cpu_seconds)
            row.update({"reference_1core_per_s": round(c1), f"reference_{cores}cores_per_s": round(cn),
                        "gpu_over_reference_all_cores": round(g / cn, 1)})
            if args.percall:
                row["reference_percall_us"] = round(1e6 / c1, 1)
        out["curves"][curve] = row
        print(json.dumps({curve: row}), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
