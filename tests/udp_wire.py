"""UDP v2 wire datagrams for the receive tests: a builder, and a Python restatement of the
structural walk of ARQParser (core/UDP.v2/UDPParser.v2.cpp; every rule cites the line it
restates) that gives the tables fpnn_aes_udp_recv must write (include/fpnn_aes.h).  It is
written from the reference and the header, not from the kernel, and tests/test_udp_wire.py tests
it by itself, so the GPU tests' expected values stand on their own feet.
"""
import struct

import numpy as np

# ARQType, ARQFlag (core/UDP.v2/UDPCommon.v2.h:18-42)
DATA, ACKS, UNA, ECDH, HEARTBEAT, FORCESYNC, CLOSE, COMBINED, ASSEMBLED = 0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x0F, 0x80, 0x81
DISCARDABLE, MONITORED, SEG1, SEG2, SEG4, LAST_SEGMENT, FIRST_PACKAGE, CANCELLED = 0x01, 0x02, 0x04, 0x08, 0x0C, 0x10, 0x20, 0x80
# FPNN_AES_UDP_* (include/fpnn_aes.h)
OK, SHORT, VERSION, TYPE, BAD_ACKS, CLOSED, FULL, LONG = range(8)

SCAN = np.dtype([("pkgs", "<u2"), ("sections", "<u2"), ("version", "u1"), ("status", "u1"), ("reserved", "<u2")])
PKG = np.dtype([("seq", "<u4"), ("type", "u1"), ("flag", "u1"), ("sign", "u1"), ("status", "u1"), ("off", "<u2"),
                ("len", "<u2"), ("first_section", "<u2"), ("nsections", "<u2")])
SECTION = np.dtype([("type", "u1"), ("flag", "u1"), ("pkg", "<u2"), ("off", "<u2"), ("len", "<u2"),
                    ("package_id", "<u2"), ("reserved", "<u2"), ("seg_index", "<u4")])
assert (SCAN.itemsize, PKG.itemsize, SECTION.itemsize) == (8, 16, 16)


# ---------------------------------------------------------------------------------------
# builder


def header(ptype, flag=0, seq=0, sign=0, version=2):
    """The 8-byte package header: version, type, flag, sign, seq (big endian)."""
    return bytes([version, ptype, flag, sign]) + struct.pack(">I", seq)


def data_body(flag, payload, package_id=0, index=0):
    """What follows a DATA header: for a segmented flag packageId and the index, then the payload."""
    seg = flag & 0x0C
    if seg == 0:
        return bytes(payload)
    return struct.pack(">H", package_id) + index.to_bytes({SEG1: 1, SEG2: 2, SEG4: 4}[seg], "big") + bytes(payload)


def package(ptype, flag=0, seq=0, body=b"", sign=0, version=2):
    return header(ptype, flag, seq, sign, version) + bytes(body)


def component(ctype, flag, body, length=None):
    """[type flag be16 bytes] body; `length` overrides the length field."""
    return bytes([ctype, flag]) + struct.pack(">H", len(body) if length is None else length) + bytes(body)


def combined(components, flag=0, seq=0, sign=0):
    return header(COMBINED, flag, seq, sign) + b"".join(components)


def assembled(packages, version=2, lengths=None):
    """ARQ_ASSEMBLED: [version 0x81] then per included package [be16 length][its bytes from the
    type byte on] (UDPParser.v2.cpp:131-134: length counts them; `lengths` overrides the fields)."""
    out = bytes([version, ASSEMBLED])
    for k, p in enumerate(packages):
        n = len(p) - 1 if lengths is None or lengths[k] is None else lengths[k]
        out += struct.pack(">H", n) + p[1:]
    return out


# ---------------------------------------------------------------------------------------
# the walk


class _Full(Exception):
    pass


class Walk:
    """The tables of one datagram: scan (pkgs, sections, version, status), pkgs and sections as
    lists of dicts with the header's field names."""

    def __init__(self, dgram, max_pkgs=1 << 16, max_sections=1 << 16):
        self.d = bytes(dgram)
        self.max_pkgs, self.max_sections = max_pkgs, max_sections
        self.pkgs, self.sections = [], []
        self.version, self.status = 0, OK
        self._walk()

    def _section(self, stype, flag, pkg, off, n, package_id=0, seg_index=0):
        if len(self.sections) >= self.max_sections:
            raise _Full
        self.sections.append(dict(type=stype, flag=flag, pkg=pkg, off=off, len=n, package_id=package_id,
                                  reserved=0, seg_index=seg_index))

    def _data(self, flag, pkg, at, n):
        """parseDATA :672-742: `n` bytes at `at`."""
        d, seg = self.d, flag & 0x0C                                # :692
        if seg == 0:                                                # :693: no segment header
            self._section(DATA, flag, pkg, at, n)
            return OK
        isz = {SEG1: 1, SEG2: 2, SEG4: 4}[seg]                      # :725-742
        if n < 2 + isz:                                             # `bytes -= 2`, `bytes -= isz` (:712, :729-741) would wrap
            return SHORT
        package_id = int.from_bytes(d[at:at + 2], "big")            # :709
        index = int.from_bytes(d[at + 2:at + 2 + isz], "big")       # :727, :733, :739
        self._section(DATA, flag, pkg, at + 2 + isz, n - 2 - isz, package_id, index)
        return OK

    def _package(self, pkg, ptype, flag, off, n):
        """processPackage :313-346 over d[off:off + n] (_buffer, _bufferLength), n >= 8."""
        d = self.d
        if ptype == COMBINED:                                       # parseCOMBINED :528-587
            if n < 16:                                              # :530
                return SHORT
            o = 8                                                   # :536
            while o < n:                                            # :538
                if o + 4 > n:                                       # :540-542 read 4 bytes
                    return SHORT
                t, f = d[off + o], d[off + o + 1]
                nbytes = int.from_bytes(d[off + o + 2:off + o + 4], "big")
                if o + 4 + nbytes > n:                              # :544
                    return SHORT
                body = off + o + 4
                if t == DATA:                                       # :552
                    st = self._data(f, pkg, body, nbytes)
                    if st != OK:
                        return st
                elif t == ACKS:                                     # :555, parseACKS :856
                    if nbytes % 4:
                        return BAD_ACKS
                    self._section(t, f, pkg, body, nbytes)
                elif t == UNA:                                      # :558, parseUNA :888 reads 4 bytes
                    if o + 8 > n:
                        return SHORT
                    self._section(t, f, pkg, body, nbytes)
                elif t == FORCESYNC:                                # :561
                    self._section(t, f, pkg, body, nbytes)
                elif t == CLOSE:                                    # :567-571: accepted, the package ends
                    self._section(t, f, pkg, body, nbytes)
                    return CLOSED
                else:                                               # :564 ECDH -> :928-933; :573-578
                    return TYPE
                o += 4 + nbytes                                     # :583
            return OK
        if ptype == DATA:                                           # :318; :681-682
            return self._data(flag, pkg, off + 8, n - 8)
        if ptype == ACKS:                                           # :321; :847-861
            if (n - 8) % 4:
                return BAD_ACKS
            self._section(ptype, flag, pkg, off + 8, n - 8)
            return OK
        if ptype == UNA:                                            # :324; :876
            if n != 12:
                return SHORT
            self._section(ptype, flag, pkg, off + 8, 4)
            return OK
        if ptype in (FORCESYNC, HEARTBEAT):                         # :327, :333
            self._section(ptype, flag, pkg, off + 8, n - 8)
            return OK
        if ptype == CLOSE:                                          # :336-340
            self._section(ptype, flag, pkg, off + 8, n - 8)
            return CLOSED
        return TYPE                                                 # :330 ECDH -> :928-933; :342-345

    def _row(self, off, n):
        """One package row and its walk; the status the datagram takes from it."""
        d = self.d
        if len(self.pkgs) >= self.max_pkgs:
            return FULL
        k = len(self.pkgs)
        row = dict(seq=int.from_bytes(d[off + 4:off + 8], "big"), type=d[off + 1], flag=d[off + 2], sign=d[off + 3],
                   status=OK, off=off, len=n, first_section=len(self.sections), nsections=0)
        self.pkgs.append(row)
        try:
            row["status"] = self._package(k, row["type"], row["flag"], off, n)
        except _Full:
            row["status"] = FULL
        row["nsections"] = len(self.sections) - row["first_section"]
        return OK if row["status"] == CLOSED else row["status"]

    def _walk(self):
        d = self.d
        if len(d) < 8:                                              # :67
            self.status = SHORT
            return
        if len(d) > 0xFFFF:                                         # (header: no UDP datagram is)
            self.status = LONG
            return
        if d[0] > 2:                                                # :96-105
            self.status = VERSION
            return
        self.version = d[0]
        if d[1] != ASSEMBLED:                                       # :111
            self.status = self._row(0, len(d))
            return
        at = 2                                                      # :126-127
        while at < len(d) and self.status == OK:                    # :129
            if at + 2 > len(d):                                     # :131 reads 2 bytes
                self.status = SHORT
                return
            plen = int.from_bytes(d[at:at + 2], "big")
            if plen < 7 or at + 2 + plen > len(d):                  # :137-138, :163-164 read its 7 header bytes; :133-134
                self.status = SHORT
                return
            self.status = self._row(at + 1, plen + 1)               # :133-134; a rejection ends the walk (:150-151)
            at += 2 + plen                                          # :154-156

    def decrypted(self, k):
        """(off, len) of package k's sections the data layer decrypts: DATA, neither discardable
        nor cancelled (:695-703, :714, :769-775, :823-829)."""
        p = self.pkgs[k]
        return [(s["off"], s["len"]) for s in self.sections[p["first_section"]:p["first_section"] + p["nsections"]]
                if s["type"] == DATA and not s["flag"] & (DISCARDABLE | CANCELLED)]


def tables(walks, max_pkgs, max_sections):
    """The three tables of a batch as structured arrays, and a mask of their used entries."""
    n = len(walks)
    scan = np.zeros(n, SCAN)
    pkgs, secs = np.zeros(n * max_pkgs, PKG), np.zeros(n * max_sections, SECTION)
    pu, su = np.zeros(n * max_pkgs, bool), np.zeros(n * max_sections, bool)
    for i, w in enumerate(walks):
        scan[i] = (len(w.pkgs), len(w.sections), w.version, w.status, 0)
        for k, p in enumerate(w.pkgs):
            pkgs[i * max_pkgs + k] = tuple(p[f] for f in PKG.names)
            pu[i * max_pkgs + k] = True
        for k, s in enumerate(w.sections):
            secs[i * max_sections + k] = tuple(s[f] for f in SECTION.names)
            su[i * max_sections + k] = True
    return scan, pkgs, secs, pu, su


# ---------------------------------------------------------------------------------------
# the case families of the receive tests.  Every expectation below is worked out by hand from
# the wire layout, so that tests/test_udp_wire.py checks the walk above against it.


def _bytes(n, salt):
    return bytes((salt * 37 + 11 * i + 5) & 0xFF for i in range(n))


def cases():
    """[(name, datagram, max_pkgs, max_sections, status, version,
         [package (type, status, off, len, first_section, nsections)],
         [section (type, flag, pkg, off, len, package_id, seg_index)])]"""
    P = _bytes
    A = package(DATA, 0, 9, P(24, 1))                                        # 32 bytes
    B = combined([component(UNA, 0, P(4, 2)), component(DATA, 0, P(12, 3))], seq=10)   # 8 + 8 + 16 = 32 bytes
    mix = combined([component(UNA, 0, P(4, 4)), component(ACKS, 0, P(8, 5)), component(DATA, DISCARDABLE, P(20, 6)),
                    component(DATA, SEG2 | LAST_SEGMENT, data_body(SEG2, P(30, 7), 0x4321, 0x0102))], seq=77, sign=3)
    two = assembled([A, B])
    out = [
        # ---- the families a receiver meets
        ("data", package(DATA, 0, 5, P(40, 8)), 4, 8, OK, 2, [(DATA, OK, 0, 48, 0, 1)], [(DATA, 0, 0, 8, 40, 0, 0)]),
        ("data_seg1", package(DATA, SEG1 | LAST_SEGMENT, 6, data_body(SEG1, P(33, 9), 0x1234, 7)), 4, 8, OK, 2,
         [(DATA, OK, 0, 44, 0, 1)], [(DATA, SEG1 | LAST_SEGMENT, 0, 11, 33, 0x1234, 7)]),
        ("data_seg2", package(DATA, SEG2, 7, data_body(SEG2, P(17, 10), 0xFFFE, 0x0102), version=1), 4, 8, OK, 1,
         [(DATA, OK, 0, 29, 0, 1)], [(DATA, SEG2, 0, 12, 17, 0xFFFE, 0x0102)]),
        ("data_seg4", package(DATA, SEG4, 8, data_body(SEG4, P(16, 11), 3, 0x01020304)), 4, 8, OK, 2,
         [(DATA, OK, 0, 30, 0, 1)], [(DATA, SEG4, 0, 14, 16, 3, 0x01020304)]),
        ("combined_mix", mix, 4, 8, OK, 2, [(COMBINED, OK, 0, 90, 0, 4)],
         [(UNA, 0, 0, 12, 4, 0, 0), (ACKS, 0, 0, 20, 8, 0, 0), (DATA, DISCARDABLE, 0, 32, 20, 0, 0),
          (DATA, SEG2 | LAST_SEGMENT, 0, 60, 30, 0x4321, 0x0102)]),
        ("combined_close", combined([component(DATA, 0, P(16, 12)), component(CLOSE, 0, b""),
                                     component(DATA, 0, P(10, 13))]), 4, 8, OK, 2, [(COMBINED, CLOSED, 0, 46, 0, 2)],
         [(DATA, 0, 0, 12, 16, 0, 0), (CLOSE, 0, 0, 32, 0, 0, 0)]),
        ("assembled_two", two, 4, 8, OK, 2, [(DATA, OK, 3, 32, 0, 1), (COMBINED, OK, 36, 32, 1, 2)],
         [(DATA, 0, 0, 11, 24, 0, 0), (UNA, 0, 1, 48, 4, 0, 0), (DATA, 0, 1, 56, 12, 0, 0)]),
        ("heartbeat8", package(HEARTBEAT, 0, 1), 4, 8, OK, 2, [(HEARTBEAT, OK, 0, 8, 0, 1)], [(HEARTBEAT, 0, 0, 8, 0, 0, 0)]),
        ("cancelled_seg", package(DATA, SEG2 | CANCELLED, 2, data_body(SEG2, P(10, 14), 5, 1)), 4, 8, OK, 2,
         [(DATA, OK, 0, 22, 0, 1)], [(DATA, SEG2 | CANCELLED, 0, 12, 10, 5, 1)]),
        ("close", package(CLOSE, 0, 3), 4, 8, OK, 2, [(CLOSE, CLOSED, 0, 8, 0, 1)], [(CLOSE, 0, 0, 8, 0, 0, 0)]),
        ("forcesync", package(FORCESYNC, 0, 4), 4, 8, OK, 2, [(FORCESYNC, OK, 0, 8, 0, 1)], [(FORCESYNC, 0, 0, 8, 0, 0, 0)]),
        ("acks", package(ACKS, 0, 4, P(8, 15)), 4, 8, OK, 2, [(ACKS, OK, 0, 16, 0, 1)], [(ACKS, 0, 0, 8, 8, 0, 0)]),
        ("una", package(UNA, 0, 4, P(4, 16)), 4, 8, OK, 2, [(UNA, OK, 0, 12, 0, 1)], [(UNA, 0, 0, 8, 4, 0, 0)]),
        # ---- hostile bytes
        ("len0", b"", 4, 8, SHORT, 0, [], []),
        ("len7", package(DATA, 0, 1)[:7], 4, 8, SHORT, 0, [], []),
        ("version3", package(DATA, 0, 1, P(8, 17), version=3), 4, 8, VERSION, 0, [], []),
        ("type07", package(0x07, 0, 1, P(4, 18)), 4, 8, TYPE, 2, [(0x07, TYPE, 0, 12, 0, 0)], []),
        ("ecdh", package(ECDH, 0, 1, P(40, 19)), 4, 8, TYPE, 2, [(ECDH, TYPE, 0, 48, 0, 0)], []),
        ("ecdh_in_combined", combined([component(DATA, 0, P(8, 20)), component(ECDH, 0, P(4, 21))]), 4, 8, TYPE, 2,
         [(COMBINED, TYPE, 0, 28, 0, 1)], [(DATA, 0, 0, 12, 8, 0, 0)]),
        ("combined15", header(COMBINED) + P(7, 22), 4, 8, SHORT, 2, [(COMBINED, SHORT, 0, 15, 0, 0)], []),
        ("overrun1", combined([component(DATA, 0, P(8, 23)), component(DATA, 0, P(8, 24), length=9)]), 4, 8, SHORT, 2,
         [(COMBINED, SHORT, 0, 32, 0, 1)], [(DATA, 0, 0, 12, 8, 0, 0)]),
        ("component_header_cut", combined([component(DATA, 0, P(8, 25))]) + b"\x01\x00\x00", 4, 8, SHORT, 2,
         [(COMBINED, SHORT, 0, 23, 0, 1)], [(DATA, 0, 0, 12, 8, 0, 0)]),
        ("acks6", package(ACKS, 0, 1, P(6, 26)), 4, 8, BAD_ACKS, 2, [(ACKS, BAD_ACKS, 0, 14, 0, 0)], []),
        ("acks6_in_combined", combined([component(DATA, 0, P(8, 27)), component(ACKS, 0, P(6, 28))]), 4, 8, BAD_ACKS, 2,
         [(COMBINED, BAD_ACKS, 0, 30, 0, 1)], [(DATA, 0, 0, 12, 8, 0, 0)]),
        ("una11", package(UNA, 0, 1, P(3, 29)), 4, 8, SHORT, 2, [(UNA, SHORT, 0, 11, 0, 0)], []),
        ("una13", package(UNA, 0, 1, P(5, 30)), 4, 8, SHORT, 2, [(UNA, SHORT, 0, 13, 0, 0)], []),
        ("una_cut_in_combined", combined([component(DATA, 0, P(4, 31)), component(UNA, 0, P(2, 32))]), 4, 8, SHORT, 2,
         [(COMBINED, SHORT, 0, 22, 0, 1)], [(DATA, 0, 0, 12, 4, 0, 0)]),
        # (accepted as the reference accepts it: :888 reads its 4 bytes inside the package; the section is 2 long)
        ("una2_then_data", combined([component(UNA, 0, P(2, 40)), component(DATA, 0, P(8, 41))]), 4, 8, OK, 2,
         [(COMBINED, OK, 0, 26, 0, 2)], [(UNA, 0, 0, 12, 2, 0, 0), (DATA, 0, 0, 18, 8, 0, 0)]),
        ("seg1_short", package(DATA, SEG1, 1, P(2, 33)), 4, 8, SHORT, 2, [(DATA, SHORT, 0, 10, 0, 0)], []),
        ("seg2_short", package(DATA, SEG2, 1, P(3, 34)), 4, 8, SHORT, 2, [(DATA, SHORT, 0, 11, 0, 0)], []),
        ("seg4_short", package(DATA, SEG4, 1, P(5, 35)), 4, 8, SHORT, 2, [(DATA, SHORT, 0, 13, 0, 0)], []),
        ("seg4_short_in_combined", combined([component(DATA, 0, P(8, 36)), component(DATA, SEG4, P(5, 37))]), 4, 8, SHORT,
         2, [(COMBINED, SHORT, 0, 29, 0, 1)], [(DATA, 0, 0, 12, 8, 0, 0)]),
        ("included6", assembled([A]) + b"\x00\x06" + P(6, 38), 4, 8, SHORT, 2, [(DATA, OK, 3, 32, 0, 1)],
         [(DATA, 0, 0, 11, 24, 0, 0)]),
        ("included_past_end", assembled([A, B], lengths=[None, 32]), 4, 8, SHORT, 2, [(DATA, OK, 3, 32, 0, 1)],
         [(DATA, 0, 0, 11, 24, 0, 0)]),
        ("trailing1", assembled([A]) + b"\x00", 4, 8, SHORT, 2, [(DATA, OK, 3, 32, 0, 1)], [(DATA, 0, 0, 11, 24, 0, 0)]),
        ("rejected_included_ends_walk", assembled([package(0x07, 0, 1, P(4, 39)), A]), 4, 8, TYPE, 2,
         [(0x07, TYPE, 3, 12, 0, 0)], []),
        ("full_pkgs", two, 1, 8, FULL, 2, [(DATA, OK, 3, 32, 0, 1)], [(DATA, 0, 0, 11, 24, 0, 0)]),
        ("full_sections", mix, 4, 3, FULL, 2, [(COMBINED, FULL, 0, 90, 0, 3)],
         [(UNA, 0, 0, 12, 4, 0, 0), (ACKS, 0, 0, 20, 8, 0, 0), (DATA, DISCARDABLE, 0, 32, 20, 0, 0)]),
    ]
    return out


FAMILIES = ("data", "data_seg1", "data_seg2", "data_seg4", "combined_mix", "combined_close", "assembled_two",
            "heartbeat8", "cancelled_seg")
