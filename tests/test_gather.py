"""Egress gather, CPU side (include/pptk_rx.h "Egress gather"):
pptk_tx_gather_host against the NumPy model of tests/gathergen.py, byte for
byte, sentinels around every array -- the edge lengths 0 .. 65535,
offset-described, stride and fixed-length batches, a null, permuted, repeating
and out-of-range list, port counts 1, 2, 3 and 64 with empty runs and null
runs, caps at 0, inside a slot, at a slot end, at a region start, need - 1 and
need, d_entries null, 0, inside a run and above max_entries, runs that are not
back to back; every -EINVAL of the contract; the ctypes layout of the three
structs against gcc's; the chain dispatch -> gather on tests/golden/flow.npz
against a replay of the reference's per-port copy loop; and a stand-alone C
program that drives the call under -fsanitize=address,undefined."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

import dispatchgen as dg
import gathergen as gg
from conftest import ROOT, load_golden
from pptk_amd.records import (GATHER_HDR_DTYPE, GATHER_PORT_DTYPE, GATHER_REGION_ALIGN,
                              GATHER_SLOT_ALIGN, GATHER_ST_BADRUNS, PORT_FLOOD)
from pptk_amd.rx import (EXPORTS, Gather, RxContext, lib, tx_dispatch_host, tx_gather_host,
                         tx_gather_scratch_bytes, tx_gather_shape)

EINVAL = -errno.EINVAL
INCLUDE = os.path.join(ROOT, "include")


def check(c, out_cap, pk_off=True, pk_len=True):
    """The host call equals the model, sentinels included; returns the Outputs."""
    rc, got = gg.host_call(lib(), c, out_cap, pk_off, pk_len)
    assert rc == 0
    want = gg.expected(c, out_cap, pk_off, pk_len)
    assert got.same(want), (got.differing(want), got.header(), want.header())
    return got


def test_exports_and_sizes():
    for s in ("pptk_tx_gather_scratch_bytes", "pptk_tx_gather_device", "pptk_tx_gather_host",
              "pptk_tx_gather_shape"):
        assert s in EXPORTS and hasattr(lib(), s), s
    for name in ("tx_gather_device", "tx_gather_host", "tx_gather_scratch_bytes", "tx_gather_shape"):
        assert hasattr(RxContext, name), name
    assert GATHER_PORT_DTYPE.names == ("start", "bytes", "entries", "packed")
    assert GATHER_HDR_DTYPE.names == ("entries", "packed", "need", "bytes", "frame_bytes", "bad",
                                      "status", "reserved")
    assert (GATHER_SLOT_ALIGN, GATHER_REGION_ALIGN, GATHER_ST_BADRUNS) == (16, 256, 1)
    B, W = tx_gather_shape()
    assert B >= 64 and B % 4 == 0 and W >= 64
    assert tx_gather_scratch_bytes(0, 4) == 0
    assert tx_gather_scratch_bytes(100, 0) == 0 == tx_gather_scratch_bytes(100, 65)
    assert tx_gather_scratch_bytes(2**32, 4) == 0
    a, b, c = (tx_gather_scratch_bytes(*x) for x in ((1000, 1), (1000, 64), (10**7, 64)))
    assert 0 < a <= b < c and a % 256 == 0
    txt = open(os.path.join(INCLUDE, "pptk_rx.h")).read()
    for name, val in (("PPTK_GATHER_SLOT_ALIGN", "16u"), ("PPTK_GATHER_REGION_ALIGN", "256u"),
                      ("PPTK_GATHER_ST_BADRUNS", "1u")):
        assert f"#define {name} " in txt and val in txt[txt.index(f"#define {name} "):][:48]
    assert txt.index("Egress dispatch:") < txt.index("Egress gather:") < txt.index("/* Tuning:")


def test_tiny_by_hand():
    """Four frames of 1, 16, 17 and 0 bytes, two ports, a flood frame."""
    frames = np.arange(100, dtype=np.uint8)
    c = gg.Case(frames, 4, off=[3, 10, 40, 90], lens=[1, 16, 17, 0], list=[2, 0, 3, 0, 1],
                runs=[2, 3], nports=2)
    got = check(c, 1024)
    assert tuple(got.header()) == (5, 5, 256 + 32, 48 + 32, 17 + 1 + 0 + 1 + 16, 0, 0, 0)
    assert [tuple(e) for e in got.port_entries()] == [(0, 48, 2, 2), (256, 32, 3, 3)]
    off, ln = got.considered()
    assert off.tolist() == [0, 32, 256, 256, 272] and ln.tolist() == [17, 1, 0, 1, 16]
    body = got.packed_bytes()
    assert body[:32].tolist() == list(range(40, 57)) + [0] * 15
    assert body[32:48].tolist() == [3] + [0] * 15 and body[272:288].tolist() == list(range(10, 26))
    assert (body[48:256] == gg.SENT).all() and (body[288:] == gg.SENT).all()


@pytest.mark.parametrize("form", ("off", "stride"))
def test_edge_lengths(form):
    rng = np.random.default_rng(len(form))
    b = gg.batch(list(gg.LENGTHS) * 2, rng, form)
    got = check(gg.Case(**b), 1 << 20)
    h = got.header()
    assert h["packed"] == h["entries"] == 22 and h["frame_bytes"] == 2 * sum(gg.LENGTHS)
    assert h["need"] == h["bytes"] == 2 * sum((x + 15) // 16 * 16 for x in gg.LENGTHS)


@pytest.mark.parametrize("length", gg.LENGTHS)
def test_fixed_len(length):
    rng = np.random.default_rng(100 + length)
    c = gg.Case(**gg.batch([length] * 5, rng, "fixed"), list=[4, 4, 0, 7, 2])
    got = check(c, 5 * 65536)
    assert got.header()["bad"] == 1 and got.header()["frame_bytes"] == 4 * length


@pytest.mark.parametrize("kind", ("null", "permuted", "flood", "bad"))
@pytest.mark.parametrize("nports", (1, 2, 3, 64))
def test_lists_and_ports(kind, nports):
    rng = np.random.default_rng(sum(kind.encode()) + nports)
    b = gg.batch(gg.mixed_lengths(300, rng), rng, "off")
    count = 300 if kind == "null" else 450
    lst = None if kind == "null" else gg.entry_list(kind, 300, count, rng)
    for runs in ([None] if nports == 1 else []) + [gg.split_runs(count, nports, rng)]:
        c = gg.Case(**b, list=lst, max_entries=count, runs=runs, nports=nports)
        got = check(c, 1 << 20)
        h, pe = got.header(), got.port_entries()
        assert h["packed"] == h["entries"] == count == pe["entries"].sum() and h["status"] == 0
        assert (pe["start"] % 256 == 0).all() and h["bytes"] == pe["bytes"].sum()
        assert (h["bad"] > 20) == (kind == "bad")
        if runs is not None and nports > 2:
            assert pe["entries"][0] == 0 and pe["start"][1] == 0
    if kind == "flood":                                          # a repeated frame is copied per entry
        off, ln = got.considered()
        body, a, b2 = got.packed_bytes(), int(off[0]), int(off[1])
        assert lst[0] == lst[1] and ln[0] == ln[1]
        assert np.array_equal(body[a:a + int(ln[0])], body[b2:b2 + int(ln[1])])


def test_caps():
    rng = np.random.default_rng(7)
    b = gg.batch(gg.mixed_lengths(200, rng), rng, "off")
    c = gg.Case(**b, list=gg.entry_list("flood", 200, 260, rng), runs=[100, 0, 90, 70], nports=4)
    full = check(c, 1 << 20)
    need, pe = int(full.header()["need"]), full.port_entries()
    off, ln = full.considered()
    g = 130                                                       # an entry of port 2 with a long slot
    while ln[g] < 40:
        g += 1
    inside, slot_end = int(off[g]) + 20, int(off[g]) + (int(ln[g]) + 15) // 16 * 16
    region = int(pe["start"][2])
    assert 0 < region < inside < slot_end < need and need % 16 == 0
    for cap, packed in ((inside, g), (slot_end, g + 1), (slot_end - 1, g), (need - 1, None),
                        (need, 260), (need + 300, 260)):
        for po, pl in ((True, True), (False, True), (True, False), (False, False)):
            got = check(c, cap, po, pl)
            h = got.header()
            assert h["need"] == need and h["entries"] == 260 and h["packed"] < 260 + (cap >= need)
            assert packed is None or h["packed"] == packed
            assert po or got.untouched(("pk_off",))
            assert pl or got.untouched(("pk_len",))
            assert np.array_equal(got.port_entries()["start"], pe["start"])
    got = check(c, region)                                        # at a region start: port 2 holds none
    assert got.port_entries()["packed"].tolist()[2:] == [0, 0] or ln[100] == 0
    assert got.port_entries()["packed"][0] == 100
    got = check(c, 0)                                             # count only, a null out
    assert got.header()["need"] == need and got.untouched(("out",))
    assert got.header()["packed"] == int(np.argmax(ln > 0))       # empty frames at offset 0 "fit"
    assert np.array_equal(got.considered()[0], off)


def test_d_entries():
    rng = np.random.default_rng(8)
    b = gg.batch(gg.mixed_lengths(120, rng, top=200), rng, "stride")
    lst = gg.entry_list("permuted", 120, 120, rng)
    for d, want in ((None, 120), (0, 0), (1, 1), (50, 50), (70, 70), (120, 120), (121, 120),
                    (2**40, 120)):
        c = gg.Case(**b, list=lst, d_entries=d, runs=[40, 40, 60], nports=3)
        got = check(c, 1 << 16)
        assert got.header()["entries"] == want
        assert got.port_entries()["entries"].tolist() == [min(want, 40), min(max(want - 40, 0), 40),
                                                          max(want - 80, 0)]
        c1 = gg.Case(**b, list=lst, d_entries=d)                  # null runs
        assert check(c1, 1 << 16).header()["entries"] == want
    # runs that end below max_entries cut too
    c = gg.Case(**b, list=lst, runs=[10, 20], nports=2)
    assert check(c, 1 << 16).header()["entries"] == 30


def test_bad_runs():
    rng = np.random.default_rng(9)
    b = gg.batch(gg.mixed_lengths(50, rng, top=100), rng, "off")
    for runs in (gg.make_runs([10, 20, 20], first=1), gg.make_runs([10, 20, 20], first=2**63),
                 np.array([(0, 10, 0, 0), (11, 20, 0, 0)], gg.DTYPES["runs"]),
                 np.array([(0, 10, 0, 0), (9, 20, 0, 0)], gg.DTYPES["runs"]),
                 np.array([(0, 2**64 - 1, 0, 0), (2**64 - 1, 5, 0, 0)], gg.DTYPES["runs"])):
        c = gg.Case(**b, runs=runs, nports=len(runs))
        got = check(c, 1 << 16)
        assert tuple(got.header()) == (0, 0, 0, 0, 0, 0, GATHER_ST_BADRUNS, 0)
        assert got.untouched() and not got.port_entries().view(np.uint8).any()


def test_empty_call():
    o = gg.Outputs(4, 5, 64)
    a = o.addresses()
    junk = gg.make_runs([3, 3, 3, 3, 3], first=7)                 # not looked at
    g = Gather(n=0, nports=5, max_entries=0, runs=junk.ctypes.data, out=a["out"], out_cap=64,
               pk_off=a["pk_off"], pk_len=a["pk_len"], ports=a["ports"], hdr=a["hdr"])
    assert lib().pptk_tx_gather_host(ctypes.byref(g)) == 0
    assert not o.hdr[64:128].any() and not o.ports[64:64 + 160].any() and o.untouched()
    assert (o.hdr[:64] == gg.SENT).all() and (o.hdr[128:] == gg.SENT).all()
    assert (o.ports[:64] == gg.SENT).all() and (o.ports[64 + 160:] == gg.SENT).all()
    # n == 0 with entries: every entry is bad, nothing is read
    c = gg.Case(None, 0, list=[0, 1, 2], fixed_len=70000)
    got = check(c, 64)
    assert tuple(got.header()) == (3, 3, 0, 0, 0, 3, 0, 0)


def test_binding():
    rng = np.random.default_rng(10)
    b = gg.batch(gg.mixed_lengths(90, rng, top=300), rng, "off")
    lst = gg.entry_list("flood", 90, 140, rng)
    c = gg.Case(**b, list=lst, runs=[50, 90], nports=2)
    want = gg.expected(c, 4096)
    h, ports, out, off, ln = tx_gather_host(b["frames"], 90, 4096, nports=2, off=b["off"],
                                            lens=b["lens"], entries=lst, runs=c.runs)
    assert tuple(h) == tuple(want.header()) and np.array_equal(ports, want.port_entries())
    assert np.array_equal(off, want.considered()[0]) and np.array_equal(ln, want.considered()[1])
    body = want.packed_bytes()
    assert np.array_equal(out[body != gg.SENT], body[body != gg.SENT]) and h["packed"] < 140
    h, _, _, off, _ = tx_gather_host(b["frames"], 90, 0, off=b["off"], lens=b["lens"], d_entries=7)
    assert h["entries"] == 7 == len(off) and h["need"] == want.header()["need"] * 0 + h["need"]
    with pytest.raises(ValueError):
        tx_gather_host(b["frames"], 90, 0, off=b["off"][:5], lens=b["lens"])
    with pytest.raises(OSError) as e:
        tx_gather_host(b["frames"], 90, 0, nports=2, off=b["off"], lens=b["lens"])
    assert e.value.errno == errno.EINVAL


def test_einval():
    call = lib().pptk_tx_gather_host
    rng = np.random.default_rng(11)
    b = gg.batch(gg.mixed_lengths(16, rng, top=100), rng, "off")
    c = gg.Case(**b, list=gg.entry_list("permuted", 16, 16, rng), d_entries=12, runs=[8, 8],
                nports=2)
    o = gg.Outputs(16, 2, 4096)

    def rc(case=c, cap=4096, outs=o, **change):
        g = gg.arguments(case, case.addresses(), outs.addresses(), cap)
        for k, v in change.items():
            setattr(g, k, v)
        return call(ctypes.byref(g))

    out, inp = o.addresses(), c.addresses()
    assert rc() == 0
    assert call(None) == EINVAL                                      # a null g
    assert rc(ports=None) == EINVAL and rc(hdr=None) == EINVAL
    assert rc(nports=0) == EINVAL and rc(nports=65) == EINVAL and rc(nports=2**31) == EINVAL
    assert rc(runs=None) == EINVAL                                   # null runs with nports != 1
    assert rc(runs=None, nports=1) == 0
    assert rc(frames=None) == EINVAL                                 # the source batch
    assert rc(off=None, stride=0) == EINVAL and rc(off=None, stride=0, n=1) == 0
    assert rc(len=None, fixed_len=65536) == EINVAL and rc(len=None, fixed_len=65535, cap=0) == 0
    assert rc(max_entries=2**32) == EINVAL and rc(n=2**32) == EINVAL and rc(n=2**40) == EINVAL
    assert rc(out=None) == EINVAL                                    # a null out with out_cap > 0
    assert rc(out=None, out_cap=0) == 0
    for step in (1, 16, 128):
        assert rc(out=out["out"] + step) == EINVAL, step
    for name, step in (("list", 2), ("off", 4), ("pk_off", 4), ("runs", 4), ("ports", 4),
                       ("hdr", 4), ("d_entries", 4), ("len", 1), ("pk_len", 1)):
        base = dict(out, list=inp["list"], off=inp["off"], len=inp["lens"], runs=inp["runs"],
                    d_entries=inp["d_entries"])[name]
        assert rc(**{name: base + step}) == EINVAL, name
    o2 = gg.Outputs(16, 2, 4096)                                     # a rejected call writes nothing
    assert rc(n=2**32, outs=o2) == EINVAL and rc(nports=0, outs=o2) == EINVAL
    assert rc(max_entries=2**32, outs=o2) == EINVAL and o2.untouched(gg.Outputs.ARRAYS)
    # frames may have any alignment
    rc1, want = gg.host_call(lib(), c, 4096)
    raw = np.zeros(len(c.frames) + 8, np.uint8)
    raw[3:3 + len(c.frames)] = c.frames
    assert rc(outs=o2, frames=raw.ctypes.data + 3) == 0 and rc1 == 0 and o2.same(want)


def test_ctypes_layout_matches_gcc(tmp_path):
    """Gather (pptk_amd/rx.py) has the size and field offsets gcc gives struct
    pptk_gather, and the two result structs their stated sizes and order."""
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "pptk_rx.h"', "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(struct pptk_gather));',
             '  printf("port_entry %zu\\n", sizeof(struct pptk_gather_port));',
             '  printf("header %zu\\n", sizeof(struct pptk_gather_hdr));']
    for fname, _ in Gather._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(struct pptk_gather, {fname}));')
    for dtype, struct in ((GATHER_PORT_DTYPE, "pptk_gather_port"), (GATHER_HDR_DTYPE, "pptk_gather_hdr")):
        for fname in dtype.names:
            lines.append(f'  printf("{struct}.{fname} %zu\\n", offsetof(struct {struct}, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", exe])
    got = dict(line.split() for line in
               subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["sizeof"]) == ctypes.sizeof(Gather) == 136
    assert int(got["port_entry"]) == GATHER_PORT_DTYPE.itemsize
    assert int(got["header"]) == GATHER_HDR_DTYPE.itemsize
    assert len(Gather._fields_) == 19
    for fname, _ in Gather._fields_:
        assert int(got[fname]) == getattr(Gather, fname).offset, fname
    for dtype, struct in ((GATHER_PORT_DTYPE, "pptk_gather_port"), (GATHER_HDR_DTYPE, "pptk_gather_hdr")):
        for fname in dtype.names:
            assert int(got[f"{struct}.{fname}"]) == dtype.fields[fname][1], fname


def test_chain_dispatch_gather_on_golden_flow():
    """tx_dispatch_host -> tx_gather_host on the flow fixture: every port's
    region equals what a replay of the reference's per-port copy loop over the
    replayed output tables leaves."""
    z = load_golden("flow")
    n, nports = len(z["off"]), 4
    rng = np.random.default_rng(12)
    port = rng.integers(0, nports, n).astype(np.uint8)
    port[::7] = PORT_FLOOD
    case = dg.Case(nports, port=port, subject=z["subject"], in_port_all=1, off=z["off"], lens=z["len"])
    tables, cls = dg.replay(case)
    h, runs, lst, _, _ = tx_dispatch_host(nports, port=port, subject=z["subject"], in_port_all=1,
                                          off=z["off"], lens=z["len"], cap=nports * n)
    assert cls["flood"] > 20 and h["written"] == h["total"] == sum(len(t) for t in tables)
    c = gg.Case(z["frames"], n, off=z["off"], lens=z["len"], list=lst, max_entries=len(lst),
                d_entries=int(h["written"]), runs=runs, nports=nports)
    got = check(c, 1 << 22)
    gh, pe, body = got.header(), got.port_entries(), got.packed_bytes()
    assert gh["packed"] == gh["entries"] == h["written"] and gh["bad"] == 0
    regions = gg.replay_regions(c, tables)
    for p in range(nports):
        s, nb = int(pe["start"][p]), int(pe["bytes"][p])
        assert nb == len(regions[p]) > 0 and bytes(body[s:s + nb]) == regions[p], p
    assert pe["entries"].tolist() == [len(t) for t in tables]


def test_sanitized_host_program(tmp_path):
    """tests/c/gather_asan.c with host/gather.c alone under ASan + UBSan, run
    as a program of its own."""
    exe = str(tmp_path / "gather_asan")
    subprocess.check_call(
        ["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O1", "-g",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
         "-static-libubsan", "-I", INCLUDE, os.path.join(ROOT, "tests", "c", "gather_asan.c"),
         os.path.join(ROOT, "pptk_amd", "csrc", "host", "gather.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "gather ok" in out.stdout, out.stdout + out.stderr


def test_perf_tool_compiles():
    """tools/gather_perf.py (the measurement driver of the DESIGN.md section)
    compiles and states its options without a GPU."""
    import py_compile
    import sys
    tool = os.path.join(ROOT, "tools", "gather_perf.py")
    py_compile.compile(tool, doraise=True)
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--frames" in out.stdout and "--sweep" in out.stdout
