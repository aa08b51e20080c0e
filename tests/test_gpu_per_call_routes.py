"""The three routes of a single CFB call from host memory (include/fpnn_aes.h: fpnn_aes_cfb_host;
fpnn_amd/csrc/engine.hip, "single call from host memory"): the resident server K0s (the default
for calls of up to 16 KiB), a K0 launch per call (FPNN_AES_SMALL_SERVER=0) and the batch
kernels for every length (FPNN_AES_SMALL=0) -- and the ECB / CBC / OFB calls, whose staging
CFB's batch route shares.  The suite reached only the default route before; anyone who moves
this code needs all three pinned.

Both toggles are read once per process, so every route runs in a fresh child process (this file
run as a program, one engine each), one child after another.  A child only computes: it writes
what it got to a JSON file, and the parent compares
  1. all 240 cases of tests/golden/cfb_cases.json (lengths 0-1000, every entry position, the
     three key lengths, both directions): output, iv_out and pos_out against the fixture;
  2. per direction one chain of calls carrying (ivec, pos) over the 16 KiB bound between the
     routes with a partial block open (AES-256, entry position 3, lengths 5, 16379, 16384,
     16385, 1): every call's output and state against the oracle;
  3. the kernel name after a 1 KiB encrypt (the route's own) and after a 16385-byte encrypt
     (the same batch kernel on every route);
  4. one golden CBC and one golden OFB case.
Server lifecycle, expiry, stop and concurrent engines are tests/test_gpu_threads.py's.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

TOGGLES = ("FPNN_AES_SMALL", "FPNN_AES_SMALL_SERVER")
ROUTES = {"default": {}, "server_off": {"FPNN_AES_SMALL_SERVER": "0"}, "small_off": {"FPNN_AES_SMALL": "0"}}
CHAIN_LENS = [5, 16379, 16384, 16385, 1]
CHAIN_POS = 3
CBC_CASE, OFB_CASE = 7, 7  # modes_cases.json: CBC encrypt of 33 bytes (AES-192), OFB of 33 bytes from position 9
CHILD_LIMIT_S = 60


def _golden(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


def _chain_inputs():
    """AES-256 key, entry ivec and the chain's data (the same bytes in both directions)."""
    rng = np.random.default_rng(16384)
    return rng.bytes(32), rng.bytes(16), [rng.bytes(n) for n in CHAIN_LENS]


def _child(out_path):
    import fpnn_amd
    res = {}
    eng = fpnn_amd.Engine(0)
    try:
        res["golden"] = []
        for c in _golden("cfb_cases.json"):
            ctx = fpnn_amd.setup_encrypt(bytes.fromhex(c["key"]))
            out, iv, pos = eng.cfb(ctx, c["encrypt"], bytes.fromhex(c["in"]), bytes.fromhex(c["iv"]), c["pos"])
            res["golden"].append([out.hex(), iv.hex(), pos])
        key, iv0, data = _chain_inputs()
        ctx = fpnn_amd.setup_encrypt(key)
        res["chain"] = {}
        for enc in (True, False):
            iv, pos, calls = iv0, CHAIN_POS, []
            for d in data:
                out, iv, pos = eng.cfb(ctx, enc, d, iv, pos)
                calls.append([out.hex(), iv.hex(), pos])
            res["chain"]["encrypt" if enc else "decrypt"] = calls
        eng.cfb(ctx, True, bytes(1024), iv0, 0)
        res["kernel_1k"] = eng.last_kernel(fpnn_amd.K_ENCRYPT)
        eng.cfb(ctx, True, bytes(16385), iv0, 0)
        res["kernel_16385"] = eng.last_kernel(fpnn_amd.K_ENCRYPT)
        g = _golden("modes_cases.json")
        c = g["cbc"][CBC_CASE]
        k = bytes.fromhex(c["key"])
        out, iv = eng.cbc(fpnn_amd.setup_encrypt(k) if c["encrypt"] else fpnn_amd.setup_decrypt(k), c["encrypt"],
                          bytes.fromhex(c["in"]), bytes.fromhex(c["iv"]), c["len"])
        res["cbc"] = [out.hex(), iv.hex()]
        c = g["ofb"][OFB_CASE]
        out, iv, pos = eng.ofb(fpnn_amd.setup_encrypt(bytes.fromhex(c["key"])), bytes.fromhex(c["in"]),
                               bytes.fromhex(c["iv"]), c["pos"])
        res["ofb"] = [out.hex(), iv.hex(), pos]
    finally:
        eng.sync()
        eng.close()
    with open(out_path, "w") as f:
        json.dump(res, f)
    print("routes child ok")


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """route -> what its child computed.  The children run one after another; after one that
    failed (a fault, an abort, its time limit) none is started."""
    got = {}
    for route, extra in ROUTES.items():
        env = {k: v for k, v in os.environ.items() if k not in TOGGLES}
        env.update(extra)
        out_path = str(tmp_path_factory.mktemp(route) / "result.json")
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable]
        if sys.flags.no_user_site:
            cmd.append("-s")
        r = subprocess.run(cmd + [os.path.abspath(__file__), "routes-child", out_path], env=env, capture_output=True,
                           text=True)
        print(r.stdout)
        print(r.stderr, file=sys.stderr)
        if r.returncode != 0 or "routes child ok" not in r.stdout:
            got[route] = (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
            break
        with open(out_path) as f:
            got[route] = json.load(f)
    return got


def _result(children, route):
    assert route in children, f"not run: an earlier child failed ({list(children)})"
    assert isinstance(children[route], dict), children[route]
    return children[route]


@pytest.fixture(scope="module")
def chain_expected(oracle):
    """direction -> [(out, ivec, pos)] of the boundary chain, from the oracle."""
    key, iv0, data = _chain_inputs()
    exp = {}
    for enc in (True, False):
        iv, pos, calls = iv0, CHAIN_POS, []
        for d in data:
            out, iv, pos = oracle.cfb(key, enc, d, iv, pos)
            calls.append([out.hex(), iv.hex(), pos])
        exp["encrypt" if enc else "decrypt"] = calls
    return exp


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES))
def test_golden_cfb_cases(children, golden, route):
    got = _result(children, route)["golden"]
    cases = golden("cfb_cases.json")
    assert len(got) == len(cases) == 240
    for i, (c, g) in enumerate(zip(cases, got)):
        assert g == [c["out"], c["iv_out"], c["pos_out"]], (route, i, len(c["in"]) // 2, c["pos"], c["encrypt"])


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES))
def test_chain_over_the_route_boundary(children, chain_expected, route):
    got = _result(children, route)["chain"]
    for direction in ("encrypt", "decrypt"):
        assert len(got[direction]) == len(CHAIN_LENS)
        for n, g, e in zip(CHAIN_LENS, got[direction], chain_expected[direction]):
            assert g[0] == e[0], (route, direction, n, "bytes")
            assert g[1:] == e[1:], (route, direction, n, "state", g[1:], e[1:])


@pytest.mark.gpu
def test_route_names(children):
    small = {r: _result(children, r)["kernel_1k"] for r in ROUTES}
    assert small["default"] == "cfb_server"
    assert small["server_off"] == "cfb_single_encrypt"
    assert small["small_off"] and small["small_off"] not in ("cfb_server", "cfb_single_encrypt"), small
    large = {r: children[r]["kernel_16385"] for r in ROUTES}
    assert large["default"] and large["default"] not in ("cfb_server", "cfb_single_encrypt"), large
    assert large["server_off"] == large["default"] and large["small_off"] == large["default"], large


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES))
def test_modes_share_the_stage(children, golden, route):
    got = _result(children, route)
    g = golden("modes_cases.json")
    c = g["cbc"][CBC_CASE]
    assert got["cbc"] == [c["out"], c["iv_out"]], (route, "cbc")
    c = g["ofb"][OFB_CASE]
    assert got["ofb"] == [c["out"], c["iv_out"], c["pos_out"]], (route, "ofb")


if __name__ == "__main__" and sys.argv[1:2] == ["routes-child"]:
    _child(sys.argv[2])
