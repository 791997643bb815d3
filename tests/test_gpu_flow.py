"""The flow-table lookup on the GPU (pptk_flow_lookup_device) against the
committed fixture (tests/golden/flow.npz), the model of tests/flowgen.py and
pptk_flow_lookup_host -- idx and status, no tolerance -- with everything the
call must not touch (entries past n, the records): the fixture through the
receive transform, batch tails at several record alignments, forged hashes
(a cluster that wraps around the end of a 16-slot table, two keys under one
64-bit hash, keys one byte off an inserted one), non-subjects, what sync makes
visible and how much it uploads, 100 000 records on a 2^16-slot table, the two
chains the lookup exists for (rx -> lookup -> seq-translate, rx -> lookup ->
tunnel encap) and the argument checks.  Needs an MI355X.

In the chains the lookup's idx stands in for the hand-made idx of
tests/seqgen.py / tests/tungen.py: the table maps every subject frame's tuple
to that frame's hand-made index (no two frames of one tuple disagree, which
the tests assert).  A frame that is no subject of the lookup (not IP,
malformed) gets PPTK_FLOW_NONE and with it the consumers' NOFLOW status, where
the hand-made idx named a flow: there the two runs agree in every byte and the
statuses are 0 / RUNT / DONE by hand and NOFLOW through the lookup; on every
other frame bytes and statuses are equal."""
import numpy as np
import pytest

import flowgen
import seqgen
import tungen
from conftest import load_golden
from pptk_amd.records import (F_MALFORMED, F_PARSED, FLOW_KEY_DTYPE, FLOW_NONE, FLOW_ST_HIT,
                              FLOW_ST_SUBJECT, REC_DTYPE, SEQ_ST_NOFLOW, as_records,
                              seqxlate_dtype)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PAD = 8
HIT = FLOW_ST_SUBJECT | FLOW_ST_HIT
NS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000)
SHIFTS = (0, 64, 128, 192, 16, 48)     # 64 * k for k in 0..3, and 16-byte-only alignment


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ctx():
    from pptk_amd.rx import RxContext
    c = RxContext(0, flowgen.KEY)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gold():
    z = load_golden("flow")
    z["fk"] = np.ascontiguousarray(z["flow_keys"]).view(FLOW_KEY_DTYPE).reshape(-1)
    return z


def rx_records(ctx, dev, buf, off, lens):
    """The receive transform's records of a packed batch: (device tensor,
    numpy REC_DTYPE copy)."""
    recs = ctx.batch_device(torch.from_numpy(buf).to(dev), len(off),
                            off=torch.from_numpy(off.view(np.int64)).to(dev),
                            lens=torch.from_numpy(lens.view(np.int16)).to(dev),
                            max_len=int(lens.max()))
    torch.cuda.synchronize()
    return recs, as_records(recs.cpu().numpy().reshape(-1)).copy()


def put_recs(dev, recs, shift=0):
    """Records on the device, starting `shift` bytes into an allocation."""
    raw = np.ascontiguousarray(recs).view(np.uint8).reshape(-1)
    big = torch.zeros(raw.size + shift + 64, dtype=torch.uint8, device=dev)
    big[shift:shift + raw.size] = torch.from_numpy(raw.copy()).to(dev)
    return big[shift:shift + raw.size]


def lookup(ctx, dev, table, d_recs, n, subject=None):
    """One launch on 0xEE-filled outputs n + PAD long: (idx uint32, status
    uint8, both whole)."""
    idx = torch.full((n + PAD,), -286331154, dtype=torch.int32, device=dev)   # 0xEEEEEEEE
    st = torch.full((n + PAD,), 0xEE, dtype=torch.uint8, device=dev)
    sub = None if subject is None else torch.from_numpy(np.ascontiguousarray(subject)).to(dev)
    ctx.flow_lookup_device(table, d_recs[:n * 64], subject=sub, idx=idx, status=st)
    torch.cuda.synchronize()
    return idx.cpu().numpy().view(np.uint32), st.cpu().numpy()


def check(got, n, want_idx, want_st):
    idx, st = got
    assert np.array_equal(idx[:n], want_idx[:n]), np.nonzero(idx[:n] != want_idx[:n])[0][:8]
    assert np.array_equal(st[:n], want_st[:n]), np.nonzero(st[:n] != want_st[:n])[0][:8]
    assert (idx[n:] == 0xEEEEEEEE).all() and (st[n:] == 0xEE).all()


def table_of(ctx, slots, keys, hashes, values):
    t = ctx.flow_table(slots)
    for k, h, v in zip(keys, hashes, values):
        t.insert(k, int(h), int(v))
    return t


# ------------------------------------------------------------------ fixture
def test_fixture_parity(ctx, dev, gold):
    z = gold
    t = table_of(ctx, int(z["slots"][0]), z["fk"], z["flow_hashes"], z["flow_values"])
    assert t.sync() == 64 * 64
    d_recs, recs = rx_records(ctx, dev, z["frames"], z["off"], z["len"])
    n = len(recs)
    got = lookup(ctx, dev, t, d_recs.reshape(-1), n)
    check(got, n, z["idx"], z["status"])
    hi, hs = t.lookup_host(recs)
    check(got, n, hi, hs)
    assert (z["status"] == HIT).sum() > 60 and (z["status"] == FLOW_ST_SUBJECT).sum() > 60
    # the default outputs: int32 idx, -1 = no flow
    idx, st = ctx.flow_lookup_device(t, d_recs)
    torch.cuda.synchronize()
    assert idx.dtype == torch.int32 and st.dtype == torch.uint8 and idx.numel() == n
    assert np.array_equal(idx.cpu().numpy().view(np.uint32), z["idx"])
    assert np.array_equal(st.cpu().numpy(), z["status"])
    t.close()


# ----------------------------------------------------------- tails and guards
@pytest.fixture(scope="module")
def small():
    """1000 records over a 2048-slot table of 600 flows: about half hit, one
    in eleven no subject.  (keys, hashes, values, records, want idx, want
    status), the expectation from the model, computed once."""
    rng = np.random.default_rng(0x7A115)
    pool = [flowgen.rand_key(rng) for _ in range(1200)]
    ph = [int(x) for x in rng.integers(0, 2**63, 1200, dtype=np.uint64) * 2 + 1]
    pick = rng.integers(0, 1200, 1000)
    flags = np.where(np.arange(1000) % 11 == 7, 0, F_PARSED).astype(np.uint16)
    recs = flowgen.records_of(np.array([pool[i] for i in pick]), [ph[i] for i in pick], flags)
    vals = [int(v) for v in rng.integers(0, 2**32 - 1, 600, dtype=np.uint64)]
    m = flowgen.Model(2048)
    for k, h, v in zip(pool[:600], ph[:600], vals):
        assert m.insert(k, h, v) == 0
    wi, ws = m.lookup_recs(recs)
    assert 350 < (ws == HIT).sum() < 600 and (ws == 0).sum() > 80
    return pool[:600], ph[:600], vals, recs, wi, ws


@pytest.fixture(scope="module")
def small_table(ctx, small):
    t = table_of(ctx, 2048, *small[:3])
    t.sync()
    yield t
    t.close()


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("n", NS)
def test_tails_and_guards(ctx, dev, small, small_table, n, shift):
    _, _, _, recs, wi, ws = small
    d = put_recs(dev, recs, shift)
    before = d.clone()
    check(lookup(ctx, dev, small_table, d, n), n, wi, ws)
    assert torch.equal(d, before)


# ------------------------------------------------------------ forged records
def test_forged_wrap_cluster(ctx, dev):
    """8 keys at home slot 15 of a 16-slot table (slots 15, 0 .. 6; the probe
    limit is 8): each is found, a 9th key with that hash is not, and after
    three of them are deleted (backward shift across the wrap) the rest are."""
    rng = np.random.default_rng(15)
    keys = [flowgen.rand_key(rng) for _ in range(9)]
    h = 0x0123456700000000 | 0xFFFFFFEF
    t = table_of(ctx, 16, keys[:8], [h] * 8, range(100, 108))
    assert t.stats() == dict(slots=16, count=8, probe_limit=8)
    t.sync()
    recs = flowgen.records_of(np.array(keys), [h] * 9)
    d = put_recs(dev, recs)
    want = np.array(list(range(100, 108)) + [FLOW_NONE], np.uint32)
    check(lookup(ctx, dev, t, d, 9), 9, want, np.array([HIT] * 8 + [FLOW_ST_SUBJECT], np.uint8))
    for j in (0, 3, 7):
        t.delete(keys[j], h)
        want[j] = FLOW_NONE
    t.sync()
    got = lookup(ctx, dev, t, d, 9)
    check(got, 9, want, np.where(want == FLOW_NONE, FLOW_ST_SUBJECT, HIT).astype(np.uint8))
    check(got, 9, *t.lookup_host(recs))
    t.close()


def test_forged_same_hash_and_one_byte_off(ctx, dev):
    ins, look = flowgen.forged_cases(np.random.default_rng(37))
    t = table_of(ctx, 64, *zip(*ins))
    t.sync()
    recs = flowgen.records_of(np.array([k for k, _, _ in look]), [h for _, h, _ in look])
    want = np.array([FLOW_NONE if v is None else v for _, _, v in look], np.uint32)
    assert len(look) == 44 and (want != FLOW_NONE).sum() == 3
    got = lookup(ctx, dev, t, put_recs(dev, recs), len(look))
    check(got, len(look), want, np.where(want == FLOW_NONE, FLOW_ST_SUBJECT, HIT).astype(np.uint8))
    check(got, len(look), *t.lookup_host(recs))
    t.close()


def test_non_subjects(ctx, dev, gold):
    """Records whose key and hash are an inserted flow's but that are not
    PARSED, are MALFORMED, or have d_subject 0."""
    z = gold
    t = table_of(ctx, 64, z["fk"], z["flow_hashes"], z["flow_values"])
    t.sync()
    m = len(z["fk"])
    keys = np.concatenate([z["fk"]] * 4)
    hashes = np.concatenate([z["flow_hashes"]] * 4)
    flags = np.concatenate([np.full(m, F_PARSED | 0x00FE), np.full(m, 0x00FE),
                            np.full(m, F_PARSED | F_MALFORMED), np.full(m, F_PARSED)])
    recs = flowgen.records_of(keys, hashes, flags.astype(np.uint16))
    sub = np.ones(4 * m, np.uint8)
    sub[3 * m:] = 0
    sub[:m:2] = 0x80
    want = np.full(4 * m, FLOW_NONE, np.uint32)
    want[:m] = z["flow_values"]
    ws = np.zeros(4 * m, np.uint8)
    ws[:m] = HIT
    d = put_recs(dev, recs)
    got = lookup(ctx, dev, t, d, 4 * m, subject=sub)
    check(got, 4 * m, want, ws)
    check(got, 4 * m, *t.lookup_host(recs, subject=sub))
    # without d_subject the last quarter are subjects again
    want[3 * m:], ws[3 * m:] = z["flow_values"], HIT
    check(lookup(ctx, dev, t, d, 4 * m), 4 * m, want, ws)
    t.close()


# --------------------------------------------------------------------- sync
def test_sync_semantics(ctx, dev, gold):
    z = gold
    fk, fh, fv = z["fk"], z["flow_hashes"], z["flow_values"]
    t = table_of(ctx, 64, fk, fh, fv)
    recs = flowgen.records_of(fk, fh)
    d = put_recs(dev, recs)
    n = len(fk)
    assert t.sync() == 4096 and t.sync() == 0
    old = (fv.copy(), np.full(n, HIT, np.uint8))
    check(lookup(ctx, dev, t, d, n), n, *old)
    t.delete(fk[2], int(fh[2]))
    t.update(fk[5], int(fh[5]), 0x55AA55AA)
    check(lookup(ctx, dev, t, d, n), n, *old)               # not synced: the old answers
    assert 0 < t.sync() <= 4096
    wi, ws = old[0].copy(), old[1].copy()
    wi[2], ws[2], wi[5] = FLOW_NONE, FLOW_ST_SUBJECT, 0x55AA55AA
    check(lookup(ctx, dev, t, d, n), n, wi, ws)
    t.clear()
    check(lookup(ctx, dev, t, d, n), n, wi, ws)             # a clear is invisible until synced
    t.sync()
    check(lookup(ctx, dev, t, d, n), n, np.full(n, FLOW_NONE, np.uint32),
          np.full(n, FLOW_ST_SUBJECT, np.uint8))
    t.close()


def test_sync_uploads_dirty_pages_only(ctx, dev, gold):
    z = gold
    t = ctx.flow_table(1 << 16)
    assert t.sync() == (1 << 16) * 64
    t.insert(z["fk"][0], int(z["flow_hashes"][0]), 7)
    assert 0 < t.sync() <= 4096
    assert t.sync() == 0
    recs = flowgen.records_of(z["fk"][:2], z["flow_hashes"][:2])
    check(lookup(ctx, dev, t, put_recs(dev, recs), 2), 2, np.array([7, FLOW_NONE], np.uint32),
          np.array([HIT, FLOW_ST_SUBJECT], np.uint8))
    t.close()


# --------------------------------------------------------------------- mass
MASS_SEED = 0x3A55


def mass_data():
    """30 000 flows and 100 000 records over a pool of 60 000 tuples (so about
    half hit and flows repeat), every 13th record no subject; hashes from
    pptk_flow_key_hash."""
    from pptk_amd.rx import flow_key_hash
    rng = np.random.default_rng(MASS_SEED)
    pool = np.zeros(60000, FLOW_KEY_DTYPE)
    pool["src"][:, :4] = rng.integers(0, 256, (60000, 4))
    pool["dst"][:, :4] = rng.integers(0, 256, (60000, 4))
    pool["sport"], pool["dport"] = rng.integers(0, 65536, 60000), rng.integers(0, 65536, 60000)
    pool["proto"] = np.where(rng.integers(0, 2, 60000), 6, 17)
    ph = np.array([flow_key_hash(flowgen.KEY, k) for k in pool], np.uint64)
    vals = rng.integers(0, 2**32 - 1, 30000, dtype=np.uint64).astype(np.uint32)
    pick = rng.integers(0, 60000, 100000)
    flags = np.where(np.arange(100000) % 13 == 5, 0, F_PARSED).astype(np.uint16)
    return pool[:30000], ph[:30000], vals, flowgen.records_of(pool[pick], ph[pick], flags)


def test_mass(ctx, dev):
    fk, fh, fv, recs = mass_data()
    for k, h in zip(fk[:50], fh[:50]):
        t40 = k.tobytes()
        assert flowgen.siphash24(flowgen.KEY, flowgen.tuple40(
            t40[:4], t40[16:20], int(k["sport"]), int(k["dport"]), int(k["proto"]))) == int(h)
    assert flowgen.linear_probe_limit(1 << 16, fh) <= 64     # before anything is launched
    m = flowgen.Model(1 << 16)
    t = ctx.flow_table(1 << 16)
    kb = fk.view(np.uint8).reshape(-1, 40)
    for j in range(len(fk)):
        assert m.insert(kb[j], int(fh[j]), int(fv[j])) == 0
    done, res = t.insert_recs(flowgen.records_of(fk, fh), fv)
    assert done == 30000 and not res.any()
    s = t.stats()
    assert s["count"] == 30000 and 1 <= s["probe_limit"] <= 64
    t.sync()
    wi, ws = m.lookup_recs(recs)
    assert 40000 < (ws == HIT).sum() < 52000 and (ws == 0).sum() > 7000
    n = len(recs)
    got = lookup(ctx, dev, t, put_recs(dev, recs), n)
    check(got, n, wi, ws)
    check(got, n, *t.lookup_host(recs))
    t.close()


# ------------------------------------------------------------------- chains
def test_chain_seq_translate(ctx, dev):
    z = load_golden("seqxlate")
    buf, off, lens, hand = z["buf"], z["off"], z["len"], z["idx"].astype(np.uint32)
    table = np.ascontiguousarray(z["table"]).view(seqxlate_dtype).reshape(-1)
    n = len(off)
    d_recs, recs = rx_records(ctx, dev, buf, off, lens)
    sub = (recs["flags"] & (F_PARSED | F_MALFORMED)) == F_PARSED
    assert (seqgen.is_subject(recs) & ~sub).sum() == 0 and sub.sum() > 3400
    t = ctx.flow_table(8192)
    done, res = t.insert_recs(recs, hand)
    assert done == sub.sum() and (res[sub] == 0).all()       # one frame per tuple: no EEXIST
    t.sync()
    idx, fst = ctx.flow_lookup_device(t, d_recs)
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy().view(np.uint32), np.where(sub, hand, FLOW_NONE))
    assert np.array_equal(fst.cpu().numpy(), np.where(sub, HIT, 0))

    def run(d_idx):
        frames = torch.from_numpy(buf).to(dev)
        st = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        ctx.seq_translate_device(
            frames, n, torch.from_numpy(table.view(np.uint8).copy()).to(dev), idx=d_idx,
            off=torch.from_numpy(off.view(np.int64)).to(dev),
            lens=torch.from_numpy(lens.view(np.int16)).to(dev), status=st)
        torch.cuda.synchronize()
        return frames.cpu().numpy(), st.cpu().numpy()

    hb, hs = run(torch.from_numpy(hand.view(np.int32)).to(dev))
    cb, cs = run(idx)
    assert (hb != buf).sum() > 3000
    assert np.array_equal(cb, hb)
    assert np.array_equal(cs[sub], hs[sub])
    assert (hs[~sub] == 0).all() and (cs[~sub] == SEQ_ST_NOFLOW).all()
    t.close()


def test_chain_tunnel_encap(ctx, dev):
    z = load_golden("tunnel")
    buf, off, lens = z["frames"], z["off"], z["len"]
    frames = [bytes(buf[int(o):int(o) + int(l)]) for o, l in zip(off, lens)]
    n = len(frames)
    tun, hand = tungen.modes(n)["idx"]
    d_recs, recs = rx_records(ctx, dev, buf, off, lens)
    sub = (recs["flags"] & (F_PARSED | F_MALFORMED)) == F_PARSED
    flow = sub & (hand != tungen.NOFLOW)
    assert flow.sum() >= 12 and (sub & ~flow).sum() >= 2
    t = ctx.flow_table(64)
    done, res = t.insert_recs(recs[flow], hand[flow])
    assert done == flow.sum() and not res.any()
    t.sync()
    idx, _ = ctx.flow_lookup_device(t, d_recs)
    eff = np.where(flow, hand, tungen.NOFLOW).astype(np.uint32)
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy().view(np.uint32), eff)

    stride = tungen.FULL_STRIDE

    def run(d_idx):
        out = torch.full((n * stride,), 0xEE, dtype=torch.uint8, device=dev)
        r = ctx.tunnel_encap_device(
            torch.from_numpy(buf).to(dev), n, tun, idx=d_idx, id_base=tungen.ID_BASE,
            off=torch.from_numpy(off.view(np.int64)).to(dev),
            lens=torch.from_numpy(lens.view(np.int16)).to(dev), out=out, out_stride=stride)
        torch.cuda.synchronize()
        return (out.cpu().numpy().reshape(n, stride), r["out_len"].cpu().numpy().view(np.uint16),
                r["status"].cpu().numpy())

    co, cl, cs = run(idx)
    want = tungen.encap_batch(frames, tun, eff, tungen.ID_BASE)
    assert np.array_equal(cs, want["status"]) and np.array_equal(cl, want["out_len"])
    assert np.array_equal(co.reshape(-1), tungen.slot_buffer(want["slots"], stride))
    ho, hl, hs = run(torch.from_numpy(hand.view(np.int32)).to(dev))
    same = sub | (hand == tungen.NOFLOW)      # every frame but the non-subjects a tunnel was named for
    assert np.array_equal(co[same], ho[same]) and np.array_equal(cl[same], hl[same])
    assert np.array_equal(cs[same], hs[same]) and (cs[~same] == tungen.ST_NOFLOW).all()
    assert (cs[flow] == tungen.ST_DONE).sum() >= 10
    t.close()


# ---------------------------------------------------------------- arguments
def test_argument_checks(ctx, dev, gold):
    from pptk_amd.rx import FlowTable, _dp
    z = gold
    call = ctx._L.pptk_flow_lookup_device
    recs = flowgen.records_of(z["fk"], z["flow_hashes"])
    n = len(recs)
    big = put_recs(dev, np.concatenate([recs, recs[:1]]))
    idx = torch.full((n + PAD,), -286331154, dtype=torch.int32, device=dev)
    st = torch.full((n + PAD,), 0xEE, dtype=torch.uint8, device=dev)
    t = table_of(ctx, 64, z["fk"], z["flow_hashes"], z["flow_values"])
    host = FlowTable(64)
    args = (_dp(big), n, None, _dp(idx), _dp(st), None)
    assert call(ctx._ctx, t._t, *args) == -22                      # never synced
    t.sync()
    assert call(ctx._ctx, host._t, *args) == -22                   # host-only
    assert call(ctx._ctx, None, *args) == -22
    assert call(None, t._t, *args) == -22
    assert call(ctx._ctx, t._t, None, n, None, _dp(idx), _dp(st), None) == -22
    assert call(ctx._ctx, t._t, _dp(big), n, None, None, _dp(st), None) == -22
    for k in (1, 4, 8):                                            # d_recs not 16-byte aligned
        assert call(ctx._ctx, t._t, _dp(big[k:]), n, None, _dp(idx), _dp(st), None) == -22
    i8 = idx.view(torch.uint8)
    assert call(ctx._ctx, t._t, _dp(big), n, None, _dp(i8[2:]), _dp(st), None) == -22
    with pytest.raises(OSError):
        ctx.flow_lookup_device(host, big[:n * 64])
    with pytest.raises(OSError):
        host.sync()
    torch.cuda.synchronize()
    assert (idx.cpu().numpy().view(np.uint32) == 0xEEEEEEEE).all() and (st.cpu().numpy() == 0xEE).all()
    assert call(ctx._ctx, t._t, _dp(big), 0, None, _dp(idx), _dp(st), None) == 0   # n = 0: nothing
    assert call(ctx._ctx, t._t, _dp(big[64:]), n, None, _dp(idx), None, None) == 0  # no status
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0xEE).all()
    got = idx.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:n - 1], z["flow_values"][1:]) and got[n - 1] == z["flow_values"][0]
    assert (got[n:] == 0xEEEEEEEE).all()
    t.close()
    host.close()
