"""fpnn_aes_udp_recv / _recv_take (include/fpnn_aes.h) without a GPU: the front library exports
and forwards them, the Python layer binds them with the header's signature, the three table
structs in fpnn_amd/_lib.py (and their numpy views) have the header's sizes and offsets -- read
from a compiled offsetof probe -- and NULL arguments are FPNN_AES_ERR_ARG.  (Every argument check
is a pure host function: tests/test_udp_recv_plan.py.)"""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fpnn_aes_udp_recv", "fpnn_aes_udp_recv_take")
STRUCTS = {"fpnn_aes_udp_scan": "UdpScan", "fpnn_aes_udp_pkg": "UdpPkg", "fpnn_aes_udp_section": "UdpSection"}


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fpnn_aes.h")).read(), flags=re.S)


def test_symbols_exported_and_forwarded():
    import fpnn_amd
    front = C.CDLL(fpnn_amd.LIB_PATH)
    fwd = open(os.path.join(ROOT, "fpnn_amd", "csrc", "front_fwd.inc")).read()
    for name in NAMES:
        assert hasattr(front, name), name
        assert re.search(r"^FPNN_FWD\(int, %s, " % name, fwd, flags=re.M), f"{name}: run gen_front.py"
        assert re.search(r"\b%s\s*\(" % name, header()), name


def test_bound_with_the_header_signature():
    import fpnn_amd
    from fpnn_amd._lib import SIGNATURES
    for name, nargs in zip(NAMES, (9, 11)):
        params = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, header(), flags=re.S).group(1)
        assert len(params.split(",")) == len(SIGNATURES[name][1]) == nargs, name
        assert getattr(fpnn_amd.lib, name).restype is C.c_int
    for name in ("udp_recv", "udp_recv_take"):
        assert callable(getattr(fpnn_amd.Engine, name)), name


def test_struct_layouts_equal_the_headers(tmp_path):
    """sizeof and offsetof of every field, from a C program compiled against the header."""
    from fpnn_amd import _lib, engine
    hdr = header()
    fields = {}
    for cname in STRUCTS:
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % cname, hdr).group(1)
        fields[cname] = [n.strip() for decl in body.split(";") if decl.strip()
                         for n in re.sub(r"^\s*\w+\s+", "", decl.strip()).split(",")]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "fpnn_aes.h"', "int main(void) {"]
    for cname, names in fields.items():
        lines.append('printf("%s %%zu", sizeof(%s));' % (cname, cname))
        lines += ['printf(" %s=%%zu", offsetof(%s, %s));' % (n, cname, n) for n in names]
        lines.append('printf("\\n");')
    lines += ['printf("flags %u %u\\n", FPNN_AES_UDP_F_WALK_ONLY, FPNN_AES_UDP_F_PLAIN);',
              'printf("status %d %d %d %d %d %d %d %d\\n", FPNN_AES_UDP_OK, FPNN_AES_UDP_SHORT, FPNN_AES_UDP_VERSION, '
              'FPNN_AES_UDP_TYPE, FPNN_AES_UDP_ACKS, FPNN_AES_UDP_CLOSE, FPNN_AES_UDP_FULL, FPNN_AES_UDP_LONG);',
              "return 0; }"]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    np_views = {"fpnn_aes_udp_scan": engine.udp_scan_dtype, "fpnn_aes_udp_pkg": engine.udp_pkg_dtype,
                "fpnn_aes_udp_section": engine.udp_section_dtype}
    for line, (cname, pyname) in zip(out, STRUCTS.items()):
        words = line.split()
        st = getattr(_lib, pyname)
        assert words[0] == cname and int(words[1]) == C.sizeof(st) == np_views[cname].itemsize, line
        want = [tuple(w.split("=")) for w in words[2:]]
        assert [(f[0], str(getattr(st, f[0]).offset)) for f in st._fields_] == want, line
        assert [(n, str(np_views[cname].fields[n][1])) for n in np_views[cname].names] == want, line
        assert [getattr(st, f[0]).size for f in st._fields_] == [np_views[cname].fields[n][0].itemsize
                                                                 for n in np_views[cname].names], line
    assert out[3].split() == ["flags", str(_lib.UDP_F_WALK_ONLY), str(_lib.UDP_F_PLAIN)]
    assert [int(x) for x in out[4].split()[1:]] == [_lib.UDP_OK, _lib.UDP_SHORT, _lib.UDP_VERSION, _lib.UDP_TYPE,
                                                    _lib.UDP_ACKS, _lib.UDP_CLOSE, _lib.UDP_FULL, _lib.UDP_LONG]
    assert [C.sizeof(getattr(_lib, p)) for p in STRUCTS.values()] == [8, 16, 16]


def test_null_arguments_are_err_arg():
    """No engine, no batch or no fpnn_aes_udp_data: FPNN_AES_ERR_ARG."""
    import fpnn_amd
    from fpnn_amd._lib import BatchDesc, UdpData
    recv, take = (getattr(fpnn_amd.lib, n) for n in NAMES)
    for b, u in ((None, None), (C.byref(BatchDesc()), C.byref(UdpData())), (C.byref(BatchDesc()), None)):
        assert recv(None, b, u, 0, 1, 1, None, None, None) == fpnn_amd.ERR_ARG
        assert take(None, b, u, 1, 1, None, None, None, None, None, 0) == fpnn_amd.ERR_ARG
