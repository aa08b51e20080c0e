#!/usr/bin/env python3
"""One side of the same-box A/B for the slot-addressed stream calls: C3 framed as ONE call
(4096 streams x 4 MiB, AES-128, random 1 B..64 KiB frames; bench_configs' framed_onecall
point) through fpnn_aes_stream_encrypt_frames / _decrypt_frames and, where the library has
them, through the *_frames_at pair with identity slots and with permuted slots.  Run it
alternately from two checkouts (the parent commit's and this one's), each in a process of
its own; every run prints one JSON line of kernel-time and wall GiB/s (steady state,
tools/bench_configs.timed).

  python tools/ab_stream_slots.py [--reps 5] [--label new]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import workloads as W  # noqa: E402
from bench_configs import gib, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import fpnn_amd
    E, D = fpnn_amd.K_ENCRYPT, fpnn_amd.K_DECRYPT
    eng = fpnn_amd.Engine(0)
    c = W.C3
    S, L = c["streams"], c["length"]
    keys, ivs = W.many_keys(c)
    a = torch.empty(S * L, dtype=torch.uint8, device="cuda")
    eng.fill_synthetic(a, c["payload_seed"])
    b, r = torch.empty_like(a), torch.empty_like(a)
    splits = [W.stream_splits(c, s) for s in range(S)]
    lens = np.concatenate([np.asarray(x, dtype=np.int32) for x in splits])
    first = np.concatenate([[0], np.cumsum([len(x) for x in splits])]).astype(np.int32)
    offs = np.concatenate([s * L + np.concatenate([[0], np.cumsum(x[:-1])]).astype(np.int64)
                           for s, x in enumerate(splits)])
    nseg = int(first[-1])
    d_lens, d_offs, d_first = (torch.from_numpy(x).cuda() for x in (lens, offs, first))
    ident = torch.arange(S, dtype=torch.int32, device="cuda")
    d_slots = torch.repeat_interleave(ident, torch.from_numpy(np.diff(first)).cuda())
    eng.reserve(nseg, S * L // 16 + nseg)
    st_iv, st_pos = torch.zeros(16 * S, dtype=torch.uint8, device="cuda"), torch.zeros(S, dtype=torch.int32,
                                                                                       device="cuda")
    perm = np.random.default_rng(c["payload_seed"]).permutation(S)
    inv = np.argsort(perm)
    res = {"label": args.label, "streams": S, "segments": nseg, "version_has_at": hasattr(eng, "stream_encrypt_frames_at")}

    def point(tag, table_order, call):
        ks = fpnn_amd.KeySet(eng, keys.reshape(S, -1)[table_order].tobytes(), c["keylen"],
                             ivs.reshape(S, 16)[table_order].tobytes())
        iv0 = torch.from_numpy(np.ascontiguousarray(ivs.reshape(S, 16)[table_order]).reshape(-1)).cuda()

        def run(encrypt, src, dst):
            st_iv.copy_(iv0)
            st_pos.zero_()
            call(encrypt, src, dst, ks)

        we, ke, _ = timed(eng, E, lambda: run(True, a, b if tag == "frames" else r), args.reps)
        if tag != "frames":
            assert torch.equal(r, b), tag  # (b: the *_frames call's ciphertext)
        wd, kd, _ = timed(eng, D, lambda: run(False, b, r), args.reps)
        assert torch.equal(r, a), tag
        res[tag] = {"encrypt_kernel_GiBs": gib(S * L, ke), "encrypt_wall_GiBs": gib(S * L, we),
                    "decrypt_kernel_GiBs": gib(S * L, kd), "decrypt_wall_GiBs": gib(S * L, wd)}
        print(json.dumps({tag: res[tag]}), file=sys.stderr, flush=True)

    kw = dict(in_off=d_offs, lens=d_lens)
    point("frames", np.arange(S), lambda enc, src, dst, ks: (
        eng.stream_encrypt_frames if enc else eng.stream_decrypt_frames)(
            src, dst, nseg, ks, st_iv, st_pos, d_first, S, key_slot=d_slots, **kw))
    if res["version_has_at"]:
        for tag, order, sl in (("at_identity", np.arange(S), ident),
                               ("at_permuted", inv, torch.from_numpy(perm.astype(np.int32)).cuda())):
            point(tag, order, lambda enc, src, dst, ks, sl=sl: (
                eng.stream_encrypt_frames_at if enc else eng.stream_decrypt_frames_at)(
                    src, dst, nseg, ks, st_iv, st_pos, d_first, S, sl, S, **kw))
    eng.sync()
    print(json.dumps({"ab_stream_slots": res}))


if __name__ == "__main__":
    main()
