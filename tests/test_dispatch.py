"""Egress dispatch, CPU side (include/pptk_rx.h "Egress dispatch"):
pptk_tx_dispatch_host against the literal replay of ldp/ldpswitch.c:276-318 in
tests/dispatchgen.py, exact, sentinels before and after every output array --
every distribution, port counts 1, 2, 3, 32, 33, 63 and 64, scalar and
per-frame ingress ports with values at or above nports, caps around the total
and cuts inside a run and between the entries of one flood frame, null out_off
/ out_len / list, the stride form, the idx form under every kind of miss_code
with indices at and above `flows` and flows == 0, n = 0; the binding; every
-EINVAL of the contract; the ctypes layout of struct pptk_dispatch against
gcc's; and a stand-alone C program that drives the call under
-fsanitize=address,undefined."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

import dispatchgen as dg
from conftest import ROOT
from pptk_amd.records import (DISPATCH_HDR_DTYPE, DISPATCH_PORT_DTYPE, FLOW_NONE, PORT_DROP,
                              PORT_FLOOD, PORT_MAX)
from pptk_amd.rx import (EXPORTS, Dispatch, lib, tx_dispatch_host, tx_dispatch_scratch_bytes,
                         tx_dispatch_shape)

EINVAL = -errno.EINVAL
INCLUDE = os.path.join(ROOT, "include")


def check(c, cap, out_off=True, out_len=True, null_list=False):
    """The host call equals the replay, sentinels included; returns the Outputs."""
    rc, got = dg.host_call(lib(), c, cap, out_off, out_len, null_list)
    assert rc == 0
    want = dg.expected(c, cap if not null_list else 0, out_off, out_len)
    assert got.same(want), (got.differing(want), got.header(), want.header())
    h = got.header()
    assert h["unicast"] + h["flood"] + h["dropped"] + h["bad"] == c.n and h["reserved"] == 0
    return got


def test_exports_and_sizes():
    for s in ("pptk_tx_dispatch_scratch_bytes", "pptk_tx_dispatch_device",
              "pptk_tx_dispatch_host", "pptk_tx_dispatch_shape"):
        assert s in EXPORTS and hasattr(lib(), s), s
    assert DISPATCH_PORT_DTYPE.names == ("start", "count", "bytes", "flooded")
    assert DISPATCH_HDR_DTYPE.names == ("total", "written", "unicast", "flood", "dropped", "bad",
                                        "hairpin", "reserved")
    assert (PORT_MAX, PORT_FLOOD, PORT_DROP) == (64, 0xFF, 0xFE)
    B, W = tx_dispatch_shape()
    assert B >= 64 and B % 16 == 0 and W >= 64
    assert tx_dispatch_scratch_bytes(0, 4) == 0
    assert tx_dispatch_scratch_bytes(100, 0) == 0 == tx_dispatch_scratch_bytes(100, 65)
    assert tx_dispatch_scratch_bytes(2**32, 4) == 0
    a, b, c = (tx_dispatch_scratch_bytes(*x) for x in ((1000, 4), (1000, 64), (10**7, 64)))
    assert 0 < a < b < c and a % 256 == 0


def test_header_constants_match():
    txt = open(os.path.join(INCLUDE, "pptk_rx.h")).read()
    for name, val in (("PPTK_PORT_MAX", "64u"), ("PPTK_PORT_FLOOD", "0xffu"),
                      ("PPTK_PORT_DROP", "0xfeu")):
        assert f"#define {name} " in txt and val in txt[txt.index(f"#define {name} "):][:40]
    assert txt.index("Flow learning:") < txt.index("Egress dispatch:") < txt.index("/* Tuning:")


def test_tiny_by_hand():
    """Seven frames, three ports, everything from port 1."""
    c = dg.Case(3, port=[0, 1, PORT_FLOOD, 2, PORT_DROP, 9, 1], in_port_all=1, stride=64,
                fixed_len=60)
    got = check(c, 7)
    assert tuple(got.header()) == (6, 6, 4, 1, 1, 1, 2, 0)
    assert [tuple(e) for e in got.port_entries()] == [(0, 2, 120, 1), (2, 2, 120, 0), (4, 2, 120, 1)]
    lst, off, ln = got.written()
    assert lst.tolist() == [0, 2, 1, 6, 2, 3] and off.tolist() == [0, 128, 64, 384, 128, 192]
    assert (ln == 60).all()


@pytest.mark.parametrize("name", dg.DISTRIBUTIONS)
@pytest.mark.parametrize("nports", (1, 2, 3, 32, 33, 63, 64))
def test_distributions(name, nports):
    rng = np.random.default_rng(sum(name.encode()) * 100 + nports)
    c = dg.case(name, 700, nports, rng, block=256, subject=nports % 2 == 1)
    got = check(c, 700 * nports)
    h, pe = got.header(), got.port_entries()
    assert h["written"] == h["total"] == pe["count"].sum()
    if name == "one_port":
        assert pe["count"][nports - 1] == h["unicast"] and h["flood"] == 0
    if name == "all_flood":
        assert h["unicast"] == 0 and (pe["flooded"] == pe["count"]).all()
        assert c.subject is not None or h["flood"] == 700
    if name in ("no_flood", "round_robin", "hairpin"):
        assert h["flood"] == 0 and not pe["flooded"].any()
    if name == "hairpin":
        assert h["hairpin"] == h["unicast"] > 500
    if name == "all_dropped":
        assert h["dropped"] == 700 and h["total"] == 0 and got.untouched()
    if name == "all_bad":
        assert h["total"] == 0 and h["bad"] + h["dropped"] == 700 and h["bad"] > 600
    if name == "random":
        assert min(h["unicast"], h["flood"], h["dropped"], h["bad"]) > 10


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 1000, 4097))
def test_sizes(n):
    rng = np.random.default_rng(50 + n)
    check(dg.case("random", n, 5, rng, block=64, subject=True), 3 * n + 1)
    check(dg.case("random", n, 64, rng, block=64, per_frame_in=False, lens=False), 70 * n)


def test_ingress():
    rng = np.random.default_rng(61)
    port = dg.codes("alternating", 500, 4, rng)
    for in_all in (0, 3, 4, 63, 64, 255, 2**32 - 1):     # at or above nports: "none"
        got = check(dg.Case(4, port=port, in_port_all=in_all, **dg.describe(500, rng)), 2000)
        pe = got.port_entries()
        assert pe["flooded"].tolist() == [0 if p == in_all else 250 for p in range(4)]
    inp = dg.ingress(500, 4, rng, none_share=0.3)
    assert (inp >= 4).sum() > 100
    check(dg.Case(4, port=port, in_port=inp, in_port_all=1, **dg.describe(500, rng)), 2000)
    # nports == 1 flooding from port 0: reaches nobody, still counts
    got = check(dg.Case(1, port=np.full(40, PORT_FLOOD, np.uint8), in_port_all=0, fixed_len=9), 40)
    assert tuple(got.header()) == (0, 0, 0, 40, 0, 0, 0, 0) and got.untouched()
    got = check(dg.Case(1, port=np.full(40, PORT_FLOOD, np.uint8), in_port_all=1, fixed_len=9), 40)
    assert got.header()["total"] == 40 and got.port_entries()["bytes"][0] == 360


def test_cap_and_nullable_outputs():
    rng = np.random.default_rng(62)
    c = dg.case("random", 900, 6, rng, block=128)
    full = check(c, 6000)
    total, pe = int(full.header()["total"]), full.port_entries()
    assert total > 1000
    inside = int(pe["start"][2] + pe["count"][2] // 2)               # a cut inside port 2's run
    between = int(pe["start"][3])                                    # and between two runs
    for cap in (1, total - 1, total, total + 5, inside, between):
        for oo, ol in ((True, True), (False, True), (True, False), (False, False)):
            got = check(c, cap, out_off=oo, out_len=ol)
            assert got.header()["written"] == min(cap, total) and got.header()["total"] == total
            assert oo or got.untouched(("out_off",))
            assert ol or got.untouched(("out_len",))
    got = check(c, 0, null_list=True)                                # the call only counts
    assert got.header()["written"] == 0 and got.untouched()
    assert np.array_equal(got.port_entries(), pe)
    # one flood frame's entries lie in different runs: a cap that keeps its
    # entry in port 0's run and cuts the one in port 1's
    f = dg.Case(3, port=[0, PORT_FLOOD, 1, 2], in_port_all=2, stride=1, fixed_len=1)
    got = check(f, 3)
    assert got.written()[0].tolist() == [0, 1, 1] and got.header()["total"] == 5
    got = check(f, 2)
    assert got.written()[0].tolist() == [0, 1]
    # the stride form
    check(dg.case("random", 300, 3, rng, lens=False), 1000)


@pytest.mark.parametrize("miss", (0, 2, PORT_FLOOD, PORT_DROP))
def test_idx_form(miss):
    rng = np.random.default_rng(63 + miss)
    c = dg.idx_case(1500, 3, 40, miss, rng)
    assert (c.idx == FLOW_NONE).sum() > 200 and ((c.idx >= 40) & (c.idx != FLOW_NONE)).sum() > 30
    got = check(c, 5000)
    assert got.header()["bad"] > 30
    c0 = dg.idx_case(300, 3, 0, miss, rng)                          # flows == 0, no table
    assert c0.flow_port is None
    got = check(c0, 1000)
    subj = c0.subject != 0
    assert got.header()["bad"] == (subj & (c0.idx != FLOW_NONE)).sum() > 100


def test_n0():
    o = dg.Outputs(4, 5)
    a = o.addresses()
    d = Dispatch(n=0, nports=5, miss_code=0, list=a["list"], out_off=a["out_off"],
                 out_len=a["out_len"], cap=4, ports=a["ports"], hdr=a["hdr"])
    assert lib().pptk_tx_dispatch_host(ctypes.byref(d)) == 0
    assert not o.hdr[64:128].any() and not o.ports[64:64 + 160].any() and o.untouched()
    assert (o.hdr[:64] == dg.SENT).all() and (o.hdr[128:] == dg.SENT).all()
    assert (o.ports[:64] == dg.SENT).all() and (o.ports[64 + 160:] == dg.SENT).all()


def test_binding():
    rng = np.random.default_rng(64)
    c = dg.case("random", 400, 4, rng)
    pktout_tbl, cls = dg.replay(c)
    h, ports, lst, off, ln = tx_dispatch_host(4, port=c.port, in_port=c.in_port, off=c.off,
                                              lens=c.lens, cap=50)
    flat = [j for t in pktout_tbl for j in t]
    assert h["total"] == len(flat) and h["written"] == 50 and lst.tolist() == flat[:50]
    assert ports["count"].tolist() == [len(t) for t in pktout_tbl]
    assert off.tolist() == [int(c.off[j]) for j in flat[:50]]
    assert ln.tolist() == [int(c.lens[j]) for j in flat[:50]]
    h, _, lst, _, _ = tx_dispatch_host(4, port=c.port)              # cap defaults to n
    assert h["written"] == min(400, len(flat))
    with pytest.raises(ValueError):
        tx_dispatch_host(4, port=c.port, idx=np.zeros(400, np.uint32))
    with pytest.raises(ValueError):
        tx_dispatch_host(4, port=c.port, subject=np.ones(399, np.uint8))
    with pytest.raises(OSError) as e:
        tx_dispatch_host(65, port=c.port)
    assert e.value.errno == errno.EINVAL


def test_einval():
    call = lib().pptk_tx_dispatch_host
    rng = np.random.default_rng(65)
    c = dg.idx_case(16, 4, 8, PORT_FLOOD, rng)
    cp = dg.case("random", 16, 4, rng)
    o = dg.Outputs(64, 4)

    def rc(case=c, cap=64, outs=o, **change):
        d = dg.arguments(case, case.addresses(), outs.addresses(), cap)
        for k, v in change.items():
            setattr(d, k, v)
        return call(ctypes.byref(d))

    out, inp = o.addresses(), c.addresses()
    assert rc() == 0 and rc(cp) == 0
    assert call(None) == EINVAL                                      # a null d
    assert rc(ports=None) == EINVAL and rc(hdr=None) == EINVAL
    assert rc(port=cp.port.ctypes.data) == EINVAL                    # both of port / idx
    assert rc(idx=None) == EINVAL                                    # neither
    assert rc(flow_port=None) == EINVAL                              # idx without flow_port, flows > 0
    assert rc(flow_port=None, flows=0) == 0
    for code in (4, 5, 64, 0xFD):                                    # miss_code: below nports, FLOOD, DROP
        assert rc(miss_code=code) == EINVAL
        assert rc(cp, miss_code=code) == EINVAL
    assert rc(miss_code=3) == 0 and rc(miss_code=PORT_DROP) == 0
    assert rc(nports=0) == EINVAL and rc(nports=65) == EINVAL and rc(cp, nports=2**31) == EINVAL
    assert rc(n=2**32) == EINVAL and rc(n=2**40) == EINVAL
    assert rc(list=None) == EINVAL                                   # a null list with cap > 0
    assert rc(list=None, cap=0) == 0
    for name, step in (("idx", 1), ("idx", 2), ("list", 2), ("off", 4), ("out_off", 4),
                       ("ports", 4), ("hdr", 4), ("len", 1), ("out_len", 1)):
        base = dict(out, idx=inp["idx"], off=inp["off"], len=inp["lens"])[name]
        assert rc(**{name: base + step}) == EINVAL, name
    o2 = dg.Outputs(64, 4)                                          # a rejected call writes nothing
    assert rc(n=2**32, outs=o2) == EINVAL and rc(nports=0, outs=o2) == EINVAL
    assert rc(miss_code=4, outs=o2) == EINVAL and o2.untouched(dg.Outputs.ARRAYS)
    # n = 0 checks too, but not port / idx
    d = Dispatch(n=0, nports=4, miss_code=9, ports=out["ports"], hdr=out["hdr"])
    assert call(ctypes.byref(d)) == EINVAL
    d.miss_code = 0
    assert call(ctypes.byref(d)) == 0
    # port, subject, in_port and flow_port may have any alignment
    raw = np.zeros(64, np.uint8)
    raw[1:17], raw[20:36] = cp.port, cp.in_port
    rc1, want = dg.host_call(lib(), cp, 64)
    assert rc(cp, outs=o2, port=raw.ctypes.data + 1, in_port=raw.ctypes.data + 20) == 0
    assert rc1 == 0 and o2.same(want)


def test_ctypes_layout_matches_gcc(tmp_path):
    """Dispatch (pptk_amd/rx.py) has the size and field offsets gcc gives
    struct pptk_dispatch, and the two result structs their stated sizes."""
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "pptk_rx.h"', "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(struct pptk_dispatch));',
             '  printf("port_entry %zu\\n", sizeof(struct pptk_dispatch_port));',
             '  printf("header %zu\\n", sizeof(struct pptk_dispatch_hdr));']
    for fname, _ in Dispatch._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(struct pptk_dispatch, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", exe])
    got = dict(line.split() for line in
               subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["sizeof"]) == ctypes.sizeof(Dispatch) == 152
    assert int(got["port_entry"]) == DISPATCH_PORT_DTYPE.itemsize
    assert int(got["header"]) == DISPATCH_HDR_DTYPE.itemsize
    assert len(Dispatch._fields_) == 22
    for fname, _ in Dispatch._fields_:
        assert int(got[fname]) == getattr(Dispatch, fname).offset, fname


def test_sanitized_host_program(tmp_path):
    """tests/c/dispatch_asan.c with host/dispatch.c alone under ASan + UBSan,
    run as a program of its own."""
    exe = str(tmp_path / "dispatch_asan")
    subprocess.check_call(
        ["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O1", "-g",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
         "-static-libubsan", "-I", INCLUDE, os.path.join(ROOT, "tests", "c", "dispatch_asan.c"),
         os.path.join(ROOT, "pptk_amd", "csrc", "host", "dispatch.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "dispatch ok" in out.stdout, out.stdout + out.stderr


def test_perf_tool_compiles():
    """tools/dispatch_perf.py (the measurement driver of DESIGN.md section 19)
    compiles and states its options without a GPU."""
    import py_compile
    import sys
    tool = os.path.join(ROOT, "tools", "dispatch_perf.py")
    py_compile.compile(tool, doraise=True)
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--frames" in out.stdout and "--calls" in out.stdout
