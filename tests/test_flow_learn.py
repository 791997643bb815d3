"""Flow learning, CPU side (include/pptk_rx.h "Flow learning"):
pptk_flow_learn_host against the dict model of tests/learngen.py -- a seeded
mix with non-subject and hit statuses in between, one flow, all distinct, no
candidates, forged hashes 0 and 2^64 - 1, three keys under one forged hash,
max_candidates below, at and above the candidate count, cap 0 with null
outputs, cap below and at `flows`, null first / packets, sentinels after
`written` and around every array, n = 0; every -EINVAL case; the host chain
lookup -> learn -> insert_recs -> lookup -> learn; and a stand-alone C program
that drives the call under -fsanitize=address,undefined."""
import errno
import os
import subprocess

import numpy as np
import pytest

import flowgen
import learngen as lg
from conftest import ROOT
from pptk_amd.records import (FLOW_LEARN_HDR_DTYPE, FLOW_NONE, FLOW_ST_HIT, FLOW_ST_SUBJECT,
                              REC_DTYPE)
from pptk_amd.rx import (EXPORTS, FlowTable, flow_learn_host, flow_learn_scratch_bytes,
                         flow_learn_shape, lib)

EINVAL = -errno.EINVAL
BIG = 1 << 30


def check(recs, status, maxc, cap, first=True, packets=True):
    """The host call equals the model, sentinels included; returns the header."""
    rc, got = lg.host_call(lib(), recs, status, maxc, cap, first=first, packets=packets)
    assert rc == 0
    want = lg.expected(recs, status, maxc, cap, first=first, packets=packets)
    assert got.same(want), (got.header(), want.header())
    return got.header()


def test_exports_and_sizes():
    for s in ("pptk_flow_learn_scratch_bytes", "pptk_flow_learn_device", "pptk_flow_learn_host",
              "pptk_flow_learn_shape"):
        assert s in EXPORTS and hasattr(lib(), s), s
    assert FLOW_LEARN_HDR_DTYPE.itemsize == 32 and REC_DTYPE.itemsize == 64
    assert FLOW_LEARN_HDR_DTYPE.names == ("candidates", "considered", "flows", "written")
    B, W = flow_learn_shape()
    assert B >= 64 and B % 16 == 0 and W >= 64
    # the scratch grows with both arguments, is 0 for what the call rejects
    assert flow_learn_scratch_bytes(0, 100) == 0
    assert flow_learn_scratch_bytes(100, 0) == 0 == flow_learn_scratch_bytes(100, BIG + 1)
    assert flow_learn_scratch_bytes(2**32, 100) == 0
    a, b, c = (flow_learn_scratch_bytes(*x) for x in ((1000, 10), (1000, 1000), (10**6, 1000)))
    assert 0 < a < b < c and a % 256 == 0
    assert flow_learn_scratch_bytes(1000, BIG) == b           # only min(n, max_candidates) counts


def test_seeded_mix():
    rng = np.random.default_rng(0x1EA2)
    recs, status = lg.mix(5000, 300, 0.3, rng)
    h = check(recs, status, BIG, 5000)
    assert 1300 < h["candidates"] < 1700 and h["considered"] == h["candidates"]
    assert 290 <= h["flows"] <= 300 and h["written"] == h["flows"]
    assert (status == (FLOW_ST_SUBJECT | FLOW_ST_HIT)).sum() > 1000 and (status == 0).sum() > 1000
    assert (status == 0xFF).sum() > 10
    rc, got = lg.host_call(lib(), recs, status, BIG, 5000)
    nr, first, packets = got.written()
    assert packets.sum() == h["candidates"] and (np.diff(first.astype(np.int64)) > 0).all()
    assert (status[first] == FLOW_ST_SUBJECT).all() and packets.max() > 3
    assert np.array_equal(nr.view(np.uint8), recs[first].view(np.uint8))


@pytest.mark.parametrize("name", ["one_flow", "all_distinct", "no_candidates", "edge_hashes",
                                  "three_under_one_hash", "cluster"])
def test_shapes(name):
    rng = np.random.default_rng(sum(name.encode()))
    if name == "one_flow":
        recs, status = lg.one_flow(700, rng)
    elif name == "all_distinct":
        recs, status = lg.all_distinct(700, rng)
    elif name == "no_candidates":
        recs, status = lg.no_candidates(700, rng)
    elif name == "edge_hashes":
        recs, status = lg.edge_hashes(rng)
    elif name == "three_under_one_hash":
        recs, status = lg.three_under_one_hash(rng)
    else:
        recs, status = lg.cluster(300, rng)
    n = len(status)
    h = check(recs, status, BIG, n)
    rc, got = lg.host_call(lib(), recs, status, BIG, n)
    _, first, packets = got.written()
    if name == "one_flow":
        assert h["flows"] == 1 and first.tolist() == [0] and packets.tolist() == [700]
    if name == "all_distinct":
        assert h["flows"] == 700 and (packets == 1).all() and first.tolist() == list(range(700))
    if name == "no_candidates":
        assert tuple(h) == (0, 0, 0, 0) and got.untouched()
    if name == "edge_hashes":
        # 8 flows of 5 frames; under hash 0 and under 2^64 - 1 the second key's
        # 5 frames each report alone: 2 + 2 * 5 + 4 entries
        assert set(recs["flow_hash"].tolist()) >= {0, lg.M64} and h["flows"] == 2 + 10 + 4
        assert sorted(packets.tolist()) == [1] * 10 + [5] * 6
    if name == "three_under_one_hash":
        # frames 0, 1, 2 are B, A, C: B leads the hash, every A and C frame is alone
        assert h["flows"] == 1 + 2 * 5 + 2 and first[:3].tolist() == [0, 1, 2]
        assert packets[0] == 5 and packets[1] == 1 and packets[2] == 1
    if name == "cluster":
        assert h["flows"] == 300 and (packets == 3).all()
        assert np.unique(recs["flow_hash"] & np.uint64(0xFFFFFFFF)).size == 1


def test_max_candidates_and_cap():
    rng = np.random.default_rng(0xCA9)
    recs, status = lg.mix(3000, 120, 0.4, rng)
    c = int((status == FLOW_ST_SUBJECT).sum())
    flows_at = {}
    for maxc in (1, 7, c - 1, c, c + 1, BIG):
        h = check(recs, status, maxc, 3000)
        assert h["candidates"] == c and h["considered"] == min(c, maxc)
        flows_at[maxc] = int(h["flows"])
    assert flows_at[1] == 1 and flows_at[7] <= 7 and flows_at[c] == flows_at[c + 1] == flows_at[BIG]
    f = flows_at[c]
    for cap in (1, f - 1, f, f + 5):
        for fp in ((True, True), (False, True), (True, False), (False, False)):
            h = check(recs, status, c, cap, first=fp[0], packets=fp[1])
            assert h["written"] == min(f, cap) and h["flows"] == f
    # cap 0 with null outputs: the call only counts
    rc, got = lg.host_call(lib(), recs, status, c, 0, first=False, packets=False, null_new=True)
    assert rc == 0 and got.untouched()
    assert tuple(got.header()) == (c, c, f, 0)
    # a repeat past the cap's entry is counted nowhere: packets of written entries are whole
    h = check(recs, status, BIG, 3)
    assert h["written"] == 3


def test_n0():
    L = lib()
    o = lg.Outputs(4)
    pn, pf, pp, ph = o.pointers()
    assert L.pptk_flow_learn_host(None, None, 0, 10, pn, pf, pp, 4, ph) == 0
    assert tuple(o.header()) == (0, 0, 0, 0) and o.untouched()
    assert (o.hdr[:32] == lg.SENT).all() and (o.hdr[64:] == lg.SENT).all()
    assert L.pptk_flow_learn_host(None, None, 0, 10, None, None, None, 0, None) == 0
    h, nr, first, packets = flow_learn_host(np.zeros(0, REC_DTYPE), np.zeros(0, np.uint8), 5, 3)
    assert tuple(h) == (0, 0, 0, 0) and len(nr) == len(first) == len(packets) == 0


def test_binding():
    rng = np.random.default_rng(8)
    recs, status = lg.mix(500, 30, 0.5, rng)
    h, nr, first, packets = flow_learn_host(recs, status, BIG, 10)
    hdr, entries = lg.model(recs, status, BIG)
    assert h["flows"] == len(entries) == 30 and h["written"] == 10 and len(nr) == 10
    assert first.tolist() == [e[0] for e in entries[:10]]
    assert packets.tolist() == [e[1] for e in entries[:10]]
    assert np.array_equal(nr.view(np.uint8), recs[first].view(np.uint8))
    with pytest.raises(ValueError):
        flow_learn_host(recs, status[:-1], BIG, 10)
    with pytest.raises(OSError) as e:
        flow_learn_host(recs, status, 0, 10)
    assert e.value.errno == errno.EINVAL


def test_einval():
    call = lib().pptk_flow_learn_host
    rng = np.random.default_rng(9)
    recs, status = lg.one_flow(8, rng)
    r = lg.aligned_records(recs)
    o = lg.Outputs(8)
    pn, pf, pp, ph = o.pointers()
    rp, sp = r.ctypes.data, status.ctypes.data
    good = (rp, sp, 8, 100, pn, pf, pp, 8, ph)

    def bad(pos, val):
        a = list(good)
        a[pos] = val
        return a

    for a in (bad(0, None), bad(1, None), bad(8, None),     # null recs, status, hdr with n > 0
              bad(4, None),                                  # null new_recs with cap > 0
              bad(2, 2**32), bad(2, 2**40),                  # n >= 2^32
              bad(3, 0), bad(3, BIG + 1),                    # max_candidates 0 or above 2^30
              bad(0, rp + 8), bad(4, pn + 8),                # recs / new_recs not 16-byte aligned
              bad(8, ph + 4),                                # hdr not 8-byte aligned
              bad(5, pf + 2), bad(6, pp + 1)):               # first / packets not 4-byte aligned
        assert call(*a) == EINVAL, a
    assert call(None, None, 0, 0, None, None, None, 0, None) == EINVAL      # n = 0 checks too
    assert call(None, None, 0, 5, None, None, None, 3, None) == EINVAL
    assert o.untouched(hdr=True)
    # status may have any alignment
    st = np.zeros(9, np.uint8)
    st[1:] = status
    assert call(rp, st.ctypes.data + 1, 8, BIG, pn, pf, pp, 8, ph) == 0
    assert tuple(o.header()) == (8, 8, 1, 1) and o.written()[2].tolist() == [8]


def test_host_chain():
    """lookup on an empty table -> learn -> insert_recs of the written records
    -> lookup again: every former candidate hits; a second learn finds nothing."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "flow.npz"))
    keys = np.ascontiguousarray(z["keys"]).view(flowgen.FLOW_KEY_DTYPE).reshape(-1)
    flags = np.where(z["subject"] != 0, flowgen.F_PARSED, 0).astype(np.uint16)
    recs = flowgen.records_of(keys, z["hashes"], flags=flags)
    t = FlowTable(1024)
    idx, st = t.lookup_host(recs)
    assert (idx == FLOW_NONE).all() and np.array_equal(st, z["subject"] * FLOW_ST_SUBJECT)
    h, nr, first, packets = flow_learn_host(recs, st, BIG, len(recs))
    assert h["candidates"] == int(z["subject"].sum()) > 100 and h["written"] == h["flows"] > 40
    assert packets.sum() == h["candidates"] and packets.max() >= 3
    done, res = t.insert_recs(nr, np.arange(len(nr), dtype=np.uint32))
    assert done == len(nr) and not res.any()
    idx2, st2 = t.lookup_host(recs)
    was = st == FLOW_ST_SUBJECT
    assert (st2[was] == (FLOW_ST_SUBJECT | FLOW_ST_HIT)).all() and (st2[~was] == 0).all()
    # a frame's flow value is the report entry of its flow's first frame
    assert np.array_equal(first[idx2[was]] <= np.nonzero(was)[0], np.ones(was.sum(), bool))
    assert np.array_equal(np.bincount(idx2[was], minlength=len(nr)), packets)
    h2, nr2, _, _ = flow_learn_host(recs, st2, BIG, len(recs))
    assert tuple(h2) == (0, 0, 0, 0) and len(nr2) == 0
    t.close()


def test_sanitized_host_program(tmp_path):
    """tests/c/flow_learn_asan.c with host/flowlearn.c alone under ASan +
    UBSan, run as a program of its own."""
    exe = str(tmp_path / "flow_learn_asan")
    subprocess.check_call(
        ["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O1", "-g",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
         "-static-libubsan", "-I", os.path.join(ROOT, "include"),
         os.path.join(ROOT, "tests", "c", "flow_learn_asan.c"),
         os.path.join(ROOT, "pptk_amd", "csrc", "host", "flowlearn.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "flow learn ok" in out.stdout, out.stdout + out.stderr
