"""tests/udp_wire.py by itself: the datagram builder and the Python restatement of ARQParser's
structural walk (core/UDP.v2/UDPParser.v2.cpp) give, on every case family of the receive tests,
the tables worked out by hand from the wire layout in udp_wire.cases() -- so the expected values
of tests/test_gpu_udp_recv.py are tested before any device sees them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import udp_wire as W  # noqa: E402

CASES = W.cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_walk_matches_the_hand_worked_tables(case):
    name, dgram, max_pkgs, max_sections, status, version, pkgs, sections = case
    w = W.Walk(dgram, max_pkgs, max_sections)
    assert (w.status, w.version) == (status, version)
    assert [(p["type"], p["status"], p["off"], p["len"], p["first_section"], p["nsections"]) for p in w.pkgs] == pkgs
    assert [(s["type"], s["flag"], s["pkg"], s["off"], s["len"], s["package_id"], s["seg_index"])
            for s in w.sections] == sections
    # every row lies inside the datagram, sections inside their package, in ascending order
    end = 0
    for s in w.sections:
        p = w.pkgs[s["pkg"]]
        assert p["off"] <= s["off"] and s["off"] + s["len"] <= p["off"] + p["len"] <= len(dgram)
        assert s["off"] >= end
        end = s["off"] + s["len"]


def test_every_family_and_hostile_case_is_there():
    names = {c[0] for c in CASES}
    assert set(W.FAMILIES) <= names
    assert {"len0", "len7", "version3", "type07", "ecdh_in_combined", "combined15", "overrun1", "acks6", "una11",
            "una13", "seg1_short", "seg2_short", "seg4_short", "included6", "included_past_end", "trailing1",
            "full_pkgs", "full_sections"} <= names


def test_header_fields_round_trip():
    """seq, sign, flag and type of the package rows are the builder's, also inside ARQ_ASSEMBLED."""
    a = W.package(W.DATA, W.MONITORED, 0xDEADBEEF, b"x" * 9, sign=0x5A)
    b = W.combined([W.component(W.FORCESYNC, 0, b"")] * 2, flag=W.FIRST_PACKAGE, seq=0x01020304, sign=7)
    for dgram, offs in ((a, [0]), (W.assembled([a, b]), [3, 3 + 2 + len(a) - 1])):
        w = W.Walk(dgram)
        assert w.status == W.OK and [p["off"] for p in w.pkgs] == offs
        assert (w.pkgs[0]["seq"], w.pkgs[0]["sign"], w.pkgs[0]["flag"], w.pkgs[0]["type"]) == (0xDEADBEEF, 0x5A, W.MONITORED, W.DATA)
    assert (w.pkgs[1]["seq"], w.pkgs[1]["sign"], w.pkgs[1]["flag"], w.pkgs[1]["nsections"]) == (0x01020304, 7, W.FIRST_PACKAGE, 2)


def test_decrypted_sections():
    """Only DATA that is neither discardable nor cancelled is data-decrypted."""
    by = {c[0]: c for c in CASES}
    assert W.Walk(by["combined_mix"][1]).decrypted(0) == [(60, 30)]
    assert W.Walk(by["cancelled_seg"][1]).decrypted(0) == []
    assert W.Walk(by["combined_close"][1]).decrypted(0) == [(12, 16)]
    two = W.Walk(by["assembled_two"][1])
    assert two.decrypted(0) == [(11, 24)] and two.decrypted(1) == [(56, 12)]
    assert W.Walk(by["heartbeat8"][1]).decrypted(0) == []


def test_long_datagram_and_tables():
    assert W.Walk(bytes(70000)).status == W.LONG
    walks = [W.Walk(c[1], c[2], c[3]) for c in CASES[:3]]
    scan, pkgs, secs, pu, su = W.tables(walks, 4, 8)
    assert scan["pkgs"].tolist() == [1, 1, 1] and pu.sum() == 3 and su.sum() == 3
    assert pkgs[4]["len"] == 44 and secs[8]["package_id"] == 0x1234 and secs[16]["seg_index"] == 0x0102
    assert np.all(pkgs[~pu] == np.zeros(1, W.PKG)) and np.all(secs[~su] == np.zeros(1, W.SECTION))
