"""The flow table, CPU side: the committed fixture (tests/golden/flow.npz)
against its generators and the model of tests/flowgen.py; keys and hashes
pinned to the oracle and to the reference through rx_batch and siphash;
pptk_flow_key_hash / pptk_flow_key_from_rec against the records;
pptk_flow_lookup_host on the fixture table; a seeded random sequence of 20 000
operations on a 256-slot host-only table checked against the model after every
step; forged hashes (the table never hashes, so the test chooses them): a
cluster that wraps around the end of a 16-slot table and is deleted in every
order, two keys under one 64-bit hash, and a key one byte off an inserted one
at each of the 37 key positions; the -EINVAL cases; and a stand-alone C
program that runs the host half under -fsanitize=address,undefined.

The fixture: 210 frames -- IPv4 and IPv6 TCP and UDP flows with and without a
VLAN tag, several frames per flow and both directions of every second one,
ICMP, a first fragment and its follow-up, IPv6 behind a hop-by-hop header, a
TCP segment too short for its header, malformed, runt and non-IP frames -- and
a 64-slot table of 24 of their tuples, at least three pairs of which share a
home slot, with values that include 0 and 0xfffffffe."""
import ctypes
import errno
import importlib.util
import itertools
import os
import subprocess

import numpy as np
import pytest

import flowgen
from conftest import GOLDEN, ROOT, load_golden
from pptk_amd.records import (FLOW_KEY_DTYPE, FLOW_NONE, FLOW_ST_HIT, FLOW_ST_SUBJECT, REC_DTYPE,
                              F_MALFORMED, F_PARSED)

EINVAL, EEXIST, ENOSPC, ENOENT = -errno.EINVAL, -errno.EEXIST, -errno.ENOSPC, -errno.ENOENT


@pytest.fixture(scope="module")
def gold():
    z = load_golden("flow")
    z["k"] = np.ascontiguousarray(z["keys"]).view(FLOW_KEY_DTYPE).reshape(-1)
    z["fk"] = np.ascontiguousarray(z["flow_keys"]).view(FLOW_KEY_DTYPE).reshape(-1)
    return z


@pytest.fixture(scope="module")
def gen_golden():
    spec = importlib.util.spec_from_file_location(
        "gen_flow_golden", os.path.join(GOLDEN, "gen_flow_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def gold_recs(gold, oracle_lib):
    """The oracle's records of the fixture frames."""
    from oracle.oracle import make_opts
    return oracle_lib.rx_batch(gold["frames"], gold["off"], gold["len"],
                               opts=make_opts(bytes(gold["key"])))


def fixture_table(gold, **kw):
    from pptk_amd.rx import FlowTable
    t = FlowTable(int(gold["slots"][0]), **kw)
    for k, h, v in zip(gold["fk"], gold["flow_hashes"], gold["flow_values"]):
        t.insert(k, int(h), int(v))
    return t


def test_fixture_is_the_generators(gold):
    z = flowgen.fixture()
    assert sorted(z) == sorted(k for k in gold if k not in ("k", "fk"))
    for name, a in z.items():
        assert a.dtype == gold[name].dtype and np.array_equal(a, gold[name]), name
    assert bytes(gold["key"]) == flowgen.KEY and int(gold["slots"][0]) == flowgen.SLOTS


def test_fixture_covers_the_shapes(gold, gold_recs):
    z, r = gold, gold_recs
    assert 190 <= len(z["off"]) <= 230 and len(z["flow_values"]) == 24
    assert flowgen.shared_home_pairs(flowgen.fixture_flows()) >= 3
    assert {0, 0xFFFFFFFE} <= set(int(v) for v in z["flow_values"])
    st = z["status"]
    for want in (0, FLOW_ST_SUBJECT, FLOW_ST_SUBJECT | FLOW_ST_HIT):
        assert (st == want).sum() >= 9, want
    assert ((z["idx"] == FLOW_NONE) == (st != 3)).all()
    fl = r["flags"]
    sub = z["subject"] != 0
    from pptk_amd.records import F_FRAGMENT, F_IPV6, F_L4, F_V6_EXT, F_VLAN
    for bit in (F_IPV6, F_VLAN, F_FRAGMENT, F_V6_EXT, F_L4):
        assert (fl[sub] & bit).any() and not (fl[sub] & bit).all(), bit
    assert {1, 6, 17} <= set(int(p) for p in r["proto"][sub])
    assert (fl & F_MALFORMED).any() and ((fl & F_PARSED) == 0).any()
    # several frames per flow, and both directions of some
    keys = [bytes(k) for k in z["keys"][sub]]
    assert max(keys.count(k) for k in set(keys)) >= 4
    rev = {k[16:32] + k[:16] + k[34:36] + k[32:34] + k[36:] for k in keys}
    assert len(rev & set(keys)) >= 10


def test_restatement_matches_fixture(gold):
    m = flowgen.Model(int(gold["slots"][0]))
    for k, h, v in zip(gold["fk"], gold["flow_hashes"], gold["flow_values"]):
        assert m.insert(k, int(h), int(v)) == 0
    idx, st = m.lookup(gold["k"], gold["hashes"], gold["subject"])
    assert np.array_equal(idx, gold["idx"]) and np.array_equal(st, gold["status"])
    for k, h in zip(gold["k"][gold["subject"] != 0], gold["hashes"][gold["subject"] != 0]):
        t = k.tobytes()
        assert flowgen.siphash24(flowgen.KEY, flowgen.tuple40(
            t[:16], t[16:32], int(k["sport"]), int(k["dport"]), int(k["proto"]))) == int(h)


def test_pinned_to_oracle(gold, gen_golden, oracle_lib):
    assert gen_golden.check_pinned(oracle_lib, gold) == int((gold["subject"] != 0).sum()) > 150


def test_pinned_to_reference(gold, gen_golden, reference_lib):
    assert gen_golden.check_pinned(reference_lib, gold) == int((gold["subject"] != 0).sum()) > 150


def test_key_hash_and_key_from_rec(gold, gold_recs):
    from pptk_amd.rx import flow_key_from_rec, flow_key_hash
    sub = gold["subject"] != 0
    for i in np.nonzero(sub)[0]:
        k = flow_key_from_rec(gold_recs[i])
        assert k.tobytes() == gold["k"][i].tobytes()
        assert flow_key_hash(flowgen.KEY, k) == int(gold_recs["flow_hash"][i]) == int(gold["hashes"][i])
    # another SipHash key gives other hashes, the ones of a context with that key
    other = bytes(range(100, 116))
    k = gold["k"][np.nonzero(sub)[0][0]]
    t = k.tobytes()
    assert flow_key_hash(other, k) == flowgen.siphash24(other, flowgen.tuple40(
        t[:16], t[16:32], int(k["sport"]), int(k["dport"]), int(k["proto"])))
    # every record gives its tuple, subject or not
    rk, _ = flowgen.keys_of_records(gold_recs)
    for i in np.nonzero(~sub)[0]:
        assert flow_key_from_rec(gold_recs[i]).tobytes() == rk[i].tobytes()


def test_lookup_host_matches_fixture(gold, gold_recs):
    t = fixture_table(gold)
    idx, st = t.lookup_host(gold_recs)
    assert np.array_equal(idx, gold["idx"]) and np.array_equal(st, gold["status"])
    assert t.stats() == dict(slots=64, count=24, probe_limit=t.stats()["probe_limit"])
    assert 2 <= t.stats()["probe_limit"] <= 24
    for k, h, v in zip(gold["fk"], gold["flow_hashes"], gold["flow_values"]):
        assert t.find(k, int(h)) == int(v)
    # a subject array takes frames out; 0xff counts as set
    sub = (np.arange(len(idx)) % 3).astype(np.uint8) * 0xFF
    idx2, st2 = t.lookup_host(gold_recs, subject=sub)
    off = sub == 0
    assert (idx2[off] == FLOW_NONE).all() and (st2[off] == 0).all()
    assert np.array_equal(idx2[~off], gold["idx"][~off]) and np.array_equal(st2[~off], gold["status"][~off])
    # insert_recs builds the same table: first frame of a flow wins, the rest EEXIST
    t2 = fixture_table(dict(gold, fk=gold["fk"][:0]))
    hit = gold["status"] == 3
    vals = np.where(hit, gold["idx"], 5).astype(np.uint32)
    vals[np.nonzero(hit)[0][3]] = FLOW_NONE                   # a bad value: skipped
    recs = gold_recs.copy()
    done, res = t2.insert_recs(recs[hit | (gold["subject"] == 0)], vals[hit | (gold["subject"] == 0)])
    sel = np.nonzero(hit | (gold["subject"] == 0))[0]
    assert done == 24 and (res == 0).sum() == 24
    assert (res[gold["subject"][sel] == 0] == EINVAL).all()
    assert res[list(sel).index(np.nonzero(hit)[0][3])] == EINVAL
    assert set(res.tolist()) == {0, EINVAL, EEXIST}
    i2, s2 = t2.lookup_host(gold_recs)
    assert np.array_equal(i2, gold["idx"]) and np.array_equal(s2, gold["status"])
    t.close()
    t2.close()


def test_random_operations_against_the_model():
    """20 000 seeded operations on a 256-slot host-only table: return code,
    find and count after every step.  The keys come from a universe of 200
    (the table holds 128), their hashes from 40 home slots around the end of
    the array with five 64-bit hashes per home slot shared by several keys."""
    from pptk_amd.rx import FlowTable
    rng = np.random.default_rng(0xF107AB)
    keys = [flowgen.rand_key(rng) for _ in range(200)]
    hashes = [(int(rng.integers(0, 5)) << 33) | ((256 - 20 + int(rng.integers(0, 40))) & 0xFFFFFFFF)
              for _ in keys]
    t, m = FlowTable(256), flowgen.Model(256)
    seen = set()
    for step in range(20000):
        j = int(rng.integers(0, len(keys)))
        k, h = keys[j], hashes[j]
        op = int(rng.integers(0, 8))
        v = int(rng.integers(0, 2**32 - 1)) if rng.integers(0, 8) else (0, 0xFFFFFFFE, FLOW_NONE)[
            int(rng.integers(0, 3))]
        if op < 3:
            got, want = t.insert_rc(k, h, v), m.insert(k, h, v)
        elif op == 3:
            got, want = t.update_rc(k, h, v), m.update(k, h, v)
        elif op < 6:
            got, want = t.delete_rc(k, h), m.delete(k, h)
        else:
            got = want = 0
        assert got == want, (step, op, got, want)
        seen.add((op if op < 3 else 3 if op == 3 else 4 if op < 6 else 6, got))
        assert t.find(k, h) == m.find(k, h), step
        s = t.stats()
        assert s["count"] == m.count and s["probe_limit"] <= 256, step
    assert {(0, 0), (0, EEXIST), (0, ENOSPC), (0, EINVAL), (3, 0), (3, ENOENT), (3, EINVAL),
            (4, 0), (4, ENOENT)} <= seen
    for k, h in zip(keys, hashes):
        assert t.find(k, h) == m.find(k, h)
    t.clear()
    assert t.stats() == dict(slots=256, count=0, probe_limit=0)
    assert all(t.find(k, h) is None for k, h in zip(keys, hashes))
    t.close()


def _raw(t, keys):
    """The C calls with prepared key pointers (the loop below makes 1.8 M)."""
    L, tp = t._L, t._t
    bufs = [np.frombuffer(k.tobytes(), np.uint8).copy() for k in keys]
    ptrs = [ctypes.c_void_p(b.ctypes.data) for b in bufs]
    return L, tp, ptrs, bufs


def test_wrapping_cluster_deleted_in_every_order():
    """8 keys whose forged hash has home slot 15 of a 16-slot table: they
    occupy slots 15, 0, 1 .. 6 and probe_limit is 8; the 9th insert is
    -ENOSPC.  Every one of the 8! deletion orders keeps the rest findable
    after each delete (backward shift across the wrap)."""
    from pptk_amd.rx import FlowTable
    rng = np.random.default_rng(15)
    keys = [flowgen.rand_key(rng) for _ in range(9)]
    h = 0x0123456700000000 | 0xFFFFFFEF            # low half & 15 == 15
    t = FlowTable(16)
    L, tp, ptrs, _keep = _raw(t, keys)
    got = ctypes.c_uint32()
    for order in itertools.permutations(range(8)):
        for j in range(8):
            assert L.pptk_flow_table_insert(tp, ptrs[j], h, 100 + j) == 0
        left = list(range(8))
        for d in order:
            assert L.pptk_flow_table_delete(tp, ptrs[d], h) == 0
            left.remove(d)
            for j in left:
                assert L.pptk_flow_table_find(tp, ptrs[j], h, ctypes.byref(got)) == 0 \
                    and got.value == 100 + j, (order, d, j)
        assert L.pptk_flow_table_find(tp, ptrs[order[-1]], h, None) == ENOENT
    assert t.stats() == dict(slots=16, count=0, probe_limit=8)
    for j in range(8):
        t.insert(keys[j], h, j)
    assert t.stats() == dict(slots=16, count=8, probe_limit=8)
    assert t.insert_rc(keys[8], h, 8) == ENOSPC and t.insert_rc(keys[8], h + 1, 8) == ENOSPC
    assert t.insert_rc(keys[2], h, 8) == EEXIST and t.find(keys[2], h) == 2
    t.close()


def test_same_hash_pair_and_one_byte_off_keys():
    from pptk_amd.rx import FlowTable
    ins, look = flowgen.forged_cases(np.random.default_rng(37))
    t = FlowTable(64)
    for k, h, v in ins:
        t.insert(k, h, v)
    assert len(look) == 7 + 37
    for k, h, want in look:
        assert t.find(k, h) == want
    t.close()


def test_einval_cases():
    from pptk_amd.rx import FlowTable
    for slots in (0, 8, 24, 1 << 27, 17, (1 << 26) + 1):
        with pytest.raises(OSError) as e:
            FlowTable(slots)
        assert e.value.errno == errno.EINVAL, slots
    t = FlowTable(16)
    k = flowgen.rand_key(np.random.default_rng(1))
    assert t.insert_rc(k, 5, FLOW_NONE) == EINVAL and t.stats()["count"] == 0
    t.insert(k, 5, 1)
    assert t.update_rc(k, 5, FLOW_NONE) == EINVAL and t.find(k, 5) == 1
    for z in range(3):
        bad = k.copy()
        bad["zero"][z] = 0x80
        assert t.insert_rc(bad, 6, 1) == EINVAL and t.update_rc(bad, 5, 2) == EINVAL
        assert t.delete_rc(bad, 5) == EINVAL
        with pytest.raises(OSError):
            t.find(bad, 5)
    assert t.find(k, 5) == 1 and t.stats()["count"] == 1
    with pytest.raises(OSError) as e:
        t.sync()                                   # a host-only table
    assert e.value.errno == errno.EINVAL
    with pytest.raises(ValueError):
        t.find(bytes(39), 5)
    t.close()
    t.close()                                      # idempotent


def test_sanitized_host_program(tmp_path):
    """tests/c/flowtab_asan.c with host/flowtab.c alone under ASan + UBSan,
    run as a program of its own."""
    exe = str(tmp_path / "flowtab_asan")
    subprocess.check_call(
        ["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O1", "-g",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
         "-static-libubsan", "-I", os.path.join(ROOT, "include"),
         os.path.join(ROOT, "tests", "c", "flowtab_asan.c"),
         os.path.join(ROOT, "pptk_amd", "csrc", "host", "flowtab.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "flowtab ok" in out.stdout, out.stdout + out.stderr
