"""Flow state, CPU side (include/pptk_rx.h "Flow state"):
pptk_flow_account_host against the NumPy model of tests/flowstatgen.py --
indices on both sides of the array's end and PPTK_FLOW_NONE, lengths 0 and
65535, fixed_len, a null unmatched, accumulation, a smaller `now`, a counter
that wraps, sentinels where nothing may be written, n = 0, every -EINVAL
case; pptk_flow_table_expire on host-only tables against the dict model of
tests/flowgen.py -- a seeded random run on a 256-slot table, a forged cluster
that wraps round the end of a 16-slot table with every subset idle, the
strict boundary, a stamp near 2^64, values past the array, cap; and a
stand-alone C program that drives both under -fsanitize=address,undefined."""
import ctypes
import errno
import itertools
import os
import subprocess

import numpy as np
import pytest

import flowgen
import flowstatgen as fs
from conftest import ROOT
from pptk_amd.records import FLOW_NONE, FLOW_STATS_DTYPE, RW_ST_NOFLOW
from pptk_amd.rx import (EXPORTS, FlowTable, flow_account_host, flow_account_shape,
                         flow_stats_array, lib)

EINVAL, ENOENT = -errno.EINVAL, -errno.ENOENT
FIELDS = FLOW_STATS_DTYPE.names


def same(a, b):
    return all(np.array_equal(a[f], b[f]) for f in FIELDS)


def test_exports_and_constants():
    for s in ("pptk_flow_account_device", "pptk_flow_account_host", "pptk_flow_stats_reset_device",
              "pptk_flow_account_shape", "pptk_flow_table_expire", "pptk_tx_rewrite_flow_device"):
        assert s in EXPORTS and hasattr(lib(), s), s
    assert FLOW_STATS_DTYPE.itemsize == 32 and RW_ST_NOFLOW == 0x80
    S, K = flow_account_shape()
    assert 0 < S <= 65536 and S * 65535 < 2**32 and K & (K - 1) == 0


# ---------------------------------------------------------------- accounting
@pytest.mark.parametrize("with_len", [True, False])
@pytest.mark.parametrize("with_um", [True, False])
def test_account_host_matches_model(with_len, with_um):
    rng = np.random.default_rng(0xACC0 + 2 * with_len + with_um)
    count, n, pad = 300, 5000, 3
    idx = rng.integers(0, count + 40, n).astype(np.uint32)
    idx[rng.integers(0, n, 200)] = FLOW_NONE
    idx[:3] = (count - 1, count, FLOW_NONE)
    lens = fs.lengths(n, rng) if with_len else None
    whole, st = fs.stats_array(count, pad)
    mw, ms = fs.stats_array(count, pad)
    um = mum = None
    if with_um:
        _, um = fs.stats_array(1)
        _, mum = fs.stats_array(1)
    # two calls accumulate; the second, with a smaller `now`, leaves last_seen alone
    for now, lo, hi in ((1000, 0, 3000), (400, 3000, n)):
        flow_account_host(idx[lo:hi], st, now, lens=None if lens is None else lens[lo:hi],
                          fixed_len=0 if with_len else 1514, unmatched=um)
        fs.account(ms, idx[lo:hi], now, lens=None if lens is None else lens[lo:hi],
                   fixed_len=0 if with_len else 1514, unmatched=mum)
    assert same(whole, mw)
    assert (st["reserved"] == fs.SENT).all() and all((whole[f][:pad] == fs.SENT).all() and
                                                     (whole[f][-pad:] == fs.SENT).all() for f in FIELDS)
    assert int(st["packets"].sum()) == int((idx < count).sum()) and st["last_seen"].max() == 1000
    assert st["packets"][count - 1] >= 1
    if with_um:
        assert same(um, mum) and int(um["packets"][0]) == int((idx >= count).sum())
        assert um["reserved"][0] == fs.SENT and um["last_seen"][0] == 1000
    if with_len:
        assert int(st["bytes"].sum()) == int(lens[idx < count].astype(np.int64).sum())
    else:
        assert np.array_equal(st["bytes"], st["packets"] * np.uint64(1514))


def test_account_host_wrap_and_n0():
    _, st = fs.stats_array(4)
    st["packets"][2] = 2**64 - 1
    st["bytes"][2] = 2**64 - 10
    flow_account_host(np.array([2], np.uint32), st, 5, fixed_len=65535)
    assert st["packets"][2] == 0 and st["bytes"][2] == 65535 - 10 and st["last_seen"][2] == 5
    before = st.copy()
    flow_account_host(np.zeros(0, np.uint32), st, 99, fixed_len=64)      # n = 0
    L = lib()
    assert L.pptk_flow_account_host(None, None, 64, 0, st.ctypes.data, 4, None, 99) == 0
    assert same(st, before)
    # now = 0 counts and leaves the stamp
    flow_account_host(np.array([1], np.uint32), st, 0, fixed_len=1)
    assert st["packets"][1] == 1 and st["last_seen"][1] == 0


def test_account_host_einval():
    call = lib().pptk_flow_account_host
    _, st = fs.stats_array(8)
    _, um = fs.stats_array(1)
    idx = np.zeros(9, np.uint32)
    lens = np.zeros(9, np.uint16)
    before = st.copy()
    p, ip, lp, up = st.ctypes.data, idx.ctypes.data, lens.ctypes.data, um.ctypes.data
    assert call(ip, lp, 0, 8, p, 8, up, 1) == 0
    st[:] = before
    for args in ((None, lp, 0, 8, p, 8, up, 1),            # null idx
                 (ip, lp, 0, 8, None, 8, up, 1),           # null stats
                 (ip, lp, 0, 8, p, 0, up, 1),              # stats_count 0
                 (ip, lp, 0, 8, p, 2**32 + 1, up, 1),      # stats_count above 2^32
                 (ip + 2, lp, 0, 8, p, 8, up, 1),          # idx not 4-byte aligned
                 (ip, lp + 1, 0, 8, p, 8, up, 1),          # len not 2-byte aligned
                 (ip, lp, 0, 8, p + 16, 7, up, 1),         # stats not 32-byte aligned
                 (ip, lp, 0, 8, p, 8, up + 8, 1),          # unmatched not 32-byte aligned
                 (ip, None, 65536, 8, p, 8, up, 1),        # fixed_len above 65535
                 (ip, lp, 65536, 8, p, 8, up, 1)):
        assert call(*args) == EINVAL, args
    assert same(st, before) and um["packets"][0] == 0
    assert call(ip, None, 65535, 8, p, 2**32, None, 1) == 0 and st["bytes"][0] == 8 * 65535


# -------------------------------------------------------------------- expire
def check_table(t, m, keys, hashes):
    for k, h in zip(keys, hashes):
        assert t.find(k, h) == m.find(k, h)
    assert t.stats()["count"] == m.count


def test_expire_random_against_model():
    """A seeded run on a 256-slot host-only table whose hashes fall into 40
    home slots around the end of the array: rounds of inserts, deletes,
    accounting with a moving clock and an expire (sometimes capped), the
    table equal to the dict model after every call."""
    rng = np.random.default_rng(0xE8917E)
    keys = [flowgen.rand_key(rng) for _ in range(200)]
    hashes = [(int(rng.integers(0, 5)) << 33) | ((256 - 20 + int(rng.integers(0, 40))) & 0xFFFFFFFF)
              for _ in keys]
    count = 150                          # values 150..199 lie past the stats array
    t, m = FlowTable(256), flowgen.Model(256)
    _, st = fs.stats_array(count)
    expired_total = capped = past = 0
    for rnd in range(300):
        now = 1000 + 10 * rnd
        for j in rng.integers(0, 200, 12):
            j = int(j)
            if rng.integers(0, 4):
                rc = t.insert_rc(keys[j], hashes[j], j)
                assert rc == m.insert(keys[j], hashes[j], j)
                if rc == 0 and j < count:
                    st[j] = (0, 0, now, fs.SENT)         # what stats_reset does
            else:
                assert t.delete_rc(keys[j], hashes[j]) == m.delete(keys[j], hashes[j])
        live = rng.integers(0, 200, 30).astype(np.uint32)
        flow_account_host(live, st, now, fixed_len=100)
        idle = int(rng.integers(0, 60))
        want = fs.idle_entries(m, st, now, idle)
        cap = None if rng.integers(0, 3) else int(rng.integers(0, 4))
        got = t.expire(st, now, idle, cap=cap)
        if cap is not None and cap < len(want):
            capped += 1
            assert len(got) == cap
            chosen = [e for e in want if e[2] in set(got.tolist())]
            assert len(chosen) == cap == len(set(got.tolist()))
            fs.model_drop(m, chosen)
            check_table(t, m, keys, hashes)
            rest = t.expire(st, now, idle)               # the rest in one more call
            assert sorted(got.tolist() + rest.tolist()) == sorted(e[2] for e in want)
            fs.model_drop(m, [e for e in want if e not in chosen])
        else:
            assert sorted(got.tolist()) == sorted(e[2] for e in want)
            fs.model_drop(m, want)
        expired_total += len(want)
        check_table(t, m, keys, hashes)
        for e in want:                                   # every expired key is gone
            assert t.find(e[1] + bytes(3), e[0]) is None
        past += sum(1 for b in m.buckets.values() for e in b if e[2] >= count)
        assert t.stats()["probe_limit"] <= 256
    assert expired_total > 300 and capped > 10 and past > 100
    # probe_limit is still a valid bound: the record lookup agrees with the model
    recs = flowgen.records_of(np.array(keys), hashes)
    wi, ws = m.lookup_recs(recs)
    gi, gs = t.lookup_host(recs)
    assert np.array_equal(gi, wi) and np.array_equal(gs, ws) and (wi != FLOW_NONE).sum() > 20
    t.close()


def test_expire_wrapping_cluster_every_subset():
    """5 keys whose forged hash has home slot 14 of a 16-slot table (slots 14,
    15, 0, 1, 2) beside a sixth at home slot 0 (pushed to slot 3): each of the
    32 subsets of the five idle in one call, the rest findable afterwards."""
    rng = np.random.default_rng(14)
    keys = [flowgen.rand_key(rng) for _ in range(6)]
    h = 0x0123456700000000 | 0xFFFFFFEE              # low half & 15 == 14
    hs = [h] * 5 + [0x7700000000000010]              # & 15 == 0
    for subset in itertools.product((0, 1), repeat=5):
        t = FlowTable(16)
        for j in range(6):
            t.insert(keys[j], hs[j], j)
        assert t.stats() == dict(slots=16, count=6, probe_limit=5)
        _, st = fs.stats_array(6)
        st["last_seen"] = [10 if subset[j] else 100 for j in range(5)] + [100]
        got = t.expire(st, 111, 100)                 # 10 + 100 < 111 <= 100 + 100
        assert sorted(got.tolist()) == [j for j in range(5) if subset[j]], subset
        for j in range(6):
            want = None if j < 5 and subset[j] else j
            assert t.find(keys[j], hs[j]) == want, (subset, j)
        assert t.stats()["count"] == 6 - sum(subset)
        assert len(t.expire(st, 111, 100)) == 0
        t.close()


def test_expire_boundaries():
    rng = np.random.default_rng(3)
    keys = [flowgen.rand_key(rng) for _ in range(4)]
    t = FlowTable(16)
    for j, k in enumerate(keys):
        t.insert(k, 0x100 + j, (0, 1, 2, 9)[j])     # value 9 lies past the array
    _, st = fs.stats_array(3)
    st["last_seen"] = [5_000_000, 2**64 - 5, 2**64 - 1]
    # last_seen + idle == now stays; one microsecond later it goes
    assert len(t.expire(st, 5_000_000 + 30_000_000, 30_000_000)) == 0
    assert t.expire(st, 5_000_000 + 30_000_001, 30_000_000).tolist() == [0]
    assert t.find(keys[0], 0x100) is None and t.find(keys[1], 0x101) == 1
    # last_seen + idle wraps past 2^64: not idle, at any `now`
    for now in (0, 3, 2**64 - 6, 2**64 - 1):
        assert len(t.expire(st, now, 100)) == 0
    assert len(t.expire(st, 2**64 - 1, 2**64 - 1)) == 0
    # a value at or past stats_count never expires, however old the clock
    st["last_seen"] = [0, 0, 0]
    assert sorted(t.expire(st, 2**63, 1).tolist()) == [1, 2]
    assert t.find(keys[3], 0x103) == 9 and t.stats()["count"] == 1
    # cap 0 deletes nothing and takes a null array; null t or stats are -EINVAL
    L = lib()
    assert L.pptk_flow_table_expire(t._t, st.ctypes.data, 16, 2**63, 1, None, 0) == 0
    assert L.pptk_flow_table_expire(None, st.ctypes.data, 3, 1, 1, None, 0) == EINVAL
    assert L.pptk_flow_table_expire(t._t, None, 3, 1, 1, None, 0) == EINVAL
    assert L.pptk_flow_table_expire(t._t, st.ctypes.data, 3, 1, 1, None, 4) == EINVAL
    assert t.stats()["count"] == 1
    t.close()


def test_expire_cap():
    rng = np.random.default_rng(77)
    keys = [flowgen.rand_key(rng) for _ in range(100)]
    hs = [int(x) for x in rng.integers(0, 2**63, 100)]
    t = FlowTable(256)
    for j in range(100):
        t.insert(keys[j], hs[j], j)
    _, st = fs.stats_array(100)
    st["last_seen"] = np.where(np.arange(100) % 3 == 0, 50, 500)
    idle = set(range(0, 100, 3))
    seen, calls = [], 0
    while True:
        got = t.expire(st, 600, 200, cap=7).tolist()
        calls += 1
        seen += got
        assert len(got) <= 7 and t.stats()["count"] == 100 - len(seen)
        if len(got) < 7:
            break
    assert calls == len(idle) // 7 + 1 and sorted(seen) == sorted(idle)
    for j in range(100):
        assert t.find(keys[j], hs[j]) == (None if j in idle else j)
    t.close()


def test_flow_stats_array_and_binding_checks():
    a = flow_stats_array(5)
    assert a.dtype == FLOW_STATS_DTYPE and a.size == 5 and a.ctypes.data % 32 == 0
    assert not a.view(np.uint8).any()
    with pytest.raises(ValueError):
        flow_account_host(np.zeros(1, np.uint32), np.zeros(4, np.uint64), 1)
    with pytest.raises(OSError) as e:
        flow_account_host(np.zeros(1, np.uint32), a, 1, fixed_len=70000)
    assert e.value.errno == errno.EINVAL


def test_sanitized_host_program(tmp_path):
    """tests/c/flowstate_asan.c with host/flowtab.c alone under ASan + UBSan,
    run as a program of its own."""
    exe = str(tmp_path / "flowstate_asan")
    subprocess.check_call(
        ["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-O1", "-g",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
         "-static-libubsan", "-I", os.path.join(ROOT, "include"),
         os.path.join(ROOT, "tests", "c", "flowstate_asan.c"),
         os.path.join(ROOT, "pptk_amd", "csrc", "host", "flowtab.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "flowstate ok" in out.stdout, out.stdout + out.stderr
