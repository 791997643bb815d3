"""The header-kernel sweeps of tests/hdrsweep.py, on the CPU: that the
generated batches reach every image / chunk geometry they are built for
(conditions on the inputs), that the oracle equals the live reference on
every one of them, and that the checksum-corner frames end where their tags
say (from the oracle's output alone).  test_gpu_hdr_sweep.py runs the same
batches through the kernels."""
import numpy as np

import hdrsweep as H

TWO_BYTE = ("sport", "dport", "tcpck", "udpck", "icmpck", "icmpid")
ALL_M = set(range(16))


# ------------------------------------------------------ coverage conditions
def test_rewrite_placed_coverage():
    b = H.rewrite_placed()
    frames, tab = H.rewrite_bases()
    assert len(frames) == 2 * 11 * 11 + 18 and b.n == len(frames) * 16 * 64
    # every (base, m, ops) triple exactly once
    key = (b.meta["fidx"] * 16 + b.meta["m"]) * 64 + b.meta["ops"]
    assert len(np.unique(key)) == b.n
    # neighbours share chunks: every gap 0..15 occurs, and nothing else
    gaps = b.starts()[1:] - (b.starts()[:-1] + b.frame_lens()[:-1])
    assert set(np.unique(gaps).tolist()) == ALL_M
    c = H.coverage(b)
    assert c["m"] == ALL_M
    # the IP header's fields cannot leave the image: m + l3 + 20 <= 15 + 18 +
    # 20 = 53 < RW_SLOT.  (A smaller RW_SLOT makes this fail: then they need
    # the straddle / past cases too.)
    assert int((b.meta["m"] + b.meta["l3"]).max()) + 20 <= H.RW_SLOT
    for f in H.IP_FIELDS:
        assert c[f]["in"] == ALL_M and not c[f]["straddle"] and not c[f]["past"], f
    for f in TWO_BYTE:
        assert c[f]["in"] and c[f]["straddle"] and c[f]["past"], f
        assert c[f]["straddle_vlan"] and c[f]["straddle_plain"], f
    for f in H.RW_FIELDS:
        assert c[f]["chunk_out"], f


def test_rewrite_fixed_coverage():
    fx = dict(H.rewrite_fixed())
    assert set(fx) == {"L42_s42", "L42_s43", "L42_s45", "L42_s64", "L98_s98", "L98_s99",
                       "L98_s101", "L98_s128", "L1500_s1501"}
    for name, b in fx.items():
        c = H.coverage(b)
        odd = b.stride & 1
        assert (c["m"] == ALL_M) if odd else (0 in c["m"]), name
        if b.stride % 16:
            assert len(c["m"]) > 1, name        # the layout the old tests never had
    # tight 42-byte frames: chunks shared with the neighbour, in fixed stride
    c = H.coverage(fx["L42_s43"])
    for f in ("ipck", "src", "dst", "sport", "dport", "udpck", "icmpck", "icmpid"):
        assert c[f]["chunk_out"], f
    c = H.coverage(fx["L98_s99"])
    for f in TWO_BYTE:
        assert c[f]["straddle"] and c[f]["past"] and c[f]["in"], f
    assert fx["L1500_s1501"].n == 2048 and fx["L1500_s1501"].fixed_len == 1500


def test_mss_coverage():
    b = H.mss_placed()
    c = H.coverage(b)
    assert c["m"] == ALL_M
    assert c["mss_dist"] == set(range(-4, 5))
    frames, tab = H.mss_bases()
    assert set(np.unique(tab["end"]).tolist()) == set(range(20, 61, 4))   # data offset 5..15
    assert set(np.unique(tab["syn"]).tolist()) == {0, 1}
    for li in range(len(H._mss_lists())):
        assert set(np.unique(tab["syn"][tab["list"] == li]).tolist()) == {0, 1}, li
    for name, fb in H.mss_fixed():
        cf = H.coverage(fb)
        if fb.stride & 1:
            assert cf["m"] == ALL_M and cf["mss_dist"] == set(range(-4, 5)), name


def test_upd16_restatement_matches_oracle(oracle_lib):
    """hdrsweep.upd16 (used to find the corner start values) against the
    oracle's update_cksum16, which test_update_cksum_kat and
    test_rewrite_oracle_vs_live_reference tie to the reference."""
    rng = np.random.default_rng(5)
    cases = [(c, o, n) for c in H.CORNER_VALUES for o in H.CORNER_VALUES for n in H.CORNER_VALUES]
    cases += [tuple(int(x) for x in rng.integers(0, 65536, 3)) for _ in range(2000)]
    for c, o, n in cases:
        assert int(H.upd16(c, o, n)) == oracle_lib.update_cksum16(c, o, n), (c, o, n)


# --------------------------------------------- oracle against live reference
def _rw_both(o, r, b, rw):
    fr = b.buf[b.origin:]
    a, sa = o.rewrite_batch(fr, rw, **b.layout())
    c, sc = r.rewrite_batch(fr, rw, **b.layout())   # TTL 0 under DECR_TTL: skipped, not aborted
    assert np.array_equal(sa, sc) and np.array_equal(a, c)


def test_rewrite_sweeps_oracle_vs_live_reference(oracle_lib, reference_lib):
    b = H.rewrite_placed()
    _rw_both(oracle_lib, reference_lib, b, b.rw)
    for _, fb in H.rewrite_fixed():
        _rw_both(oracle_lib, reference_lib, fb, fb.rw)
        _rw_both(oracle_lib, reference_lib, fb, fb.rw_one)
    cb, _ = H.corners()
    _rw_both(oracle_lib, reference_lib, cb, cb.rw)


def test_mss_sweeps_oracle_vs_live_reference(oracle_lib, reference_lib):
    for b in [H.mss_placed()] + [fb for _, fb in H.mss_fixed()]:
        fr = b.buf[b.origin:]
        for mss in H.MSS_CLAMPS:
            for flags in (0, 1):
                a, sa = oracle_lib.mss_clamp_batch(fr, mss, flags, **b.layout())
                c, sc = reference_lib.mss_clamp_batch(fr, mss, flags, **b.layout())
                assert np.array_equal(sa, sc) and np.array_equal(a, c), (mss, flags)


# ------------------------------------------------------ expected statuses
def test_rewrite_placed_statuses(oracle_lib):
    """The oracle's statuses over the placed sweep, by base kind: what the
    base set is meant to produce."""
    b = H.rewrite_placed()
    _, st = oracle_lib.rewrite_batch(b.buf, b.rw, **b.layout())
    kind, ops = b.meta["kind"], b.meta["ops"]
    ttl = (ops & H.OP_TTL) != 0
    icmp = (ops & H.OP_ICMP) != 0
    assert (st[(kind == H.K_TTL0) & ttl] == 4).all() and ((kind == H.K_TTL0) & ttl).sum() > 1000
    assert (st[(kind == H.K_TTL1) & ttl] == 1 + 2 + 8).all()
    assert (st[(kind == H.K_TCP) | (kind == H.K_UDP) | (kind == H.K_UDP0)] == 3).all()
    for k in (H.K_ICMP8, H.K_ICMP0):
        assert (st[(kind == k) & icmp] == 0x11).all() and (st[(kind == k) & ~icmp] == 1).all()
    for k in (H.K_ICMPX, H.K_ICMPCUT, H.K_P47, H.K_FRAG):
        assert (st[kind == k] == 1).all(), k


def test_mss_placed_statuses(oracle_lib):
    b = H.mss_placed()
    names = [x[0] for x in H._mss_lists()]
    _, st = oracle_lib.mss_clamp_batch(b.buf, 536, 0, **b.layout())
    want = {"none": 1, "k2l3": 1, "k2l5": 1, "toolong": 1, "eol": 1,
            "kindlast": 9, "len0": 9, "len1": 9, "k2len0": 9, "past": 9, "past1": 9}
    for li, nm in enumerate(names):
        assert (st[b.meta["list"] == li] == want.get(nm, 7)).all(), nm
    out, st = oracle_lib.mss_clamp_batch(b.buf, H.MSS_PRESENT, 0, **b.layout())
    assert not (st & 4).any() and np.array_equal(out, b.buf)      # equal: not clamped
    _, st = oracle_lib.mss_clamp_batch(b.buf, H.MSS_PRESENT - 1, 1, **b.layout())
    assert (st[b.meta["syn"] == 0] == 0).all() and (st & 4).sum() > 5000


# ---------------------------------------------------- corner expectations
def _be16(buf, pos):
    return (buf[pos].astype(np.int64) << 8) | buf[pos + 1]


def test_corner_expectations(oracle_lib):
    b, unreachable = H.corners()
    # RFC 1624 eqn. 3 gives 0xffff only from 0xffff with old 0xffff, new 0:
    # the TTL word (ttl << 8 | proto) is never rewritten to 0
    assert unreachable == {(H.F_IP, 0, 0xFFFF)}
    out, st = oracle_lib.rewrite_batch(b.buf, b.rw, **b.layout())
    assert not (st & 4).any()
    t, meta = b.tags, b.meta
    off = b.starts()
    ipck = _be16(out, off + meta["l3"] + 10)
    l4ck = _be16(out, off + meta["l4"] + meta["cko"])
    final = np.where(t["field"] == H.F_IP, ipck, l4ck)
    # every (field, update, target) is present (but the unreachable one), in
    # at least one variant whose final field must be the target, 16 m each
    # (ICMP echo has the identifier update alone: 8 bases x 16 m would be
    # 128 frames, of 5 TCP/UDP/echo bases x 16 m at least 64 are asked for)
    for field, ks in ((H.F_IP, range(5)), (H.F_L4, range(1, 8))):
        for k in ks:
            for target in (0x0000, 0xFFFF):
                if (field, k, target) in unreachable:
                    continue
                sel = (t["field"] == field) & (t["k"] == k) & (t["target"] == target)
                assert sel.sum() >= 64, (field, k, target)
                pred = sel & (t["predict"] != 0)
                if k in (1, 3):
                    # a 32-bit update does not stop between its halves (nor
                    # is a UDP checksum's 0 looked at there)
                    assert not pred.any()
                    continue
                assert pred.sum() >= 64, (field, k, target)
                assert (final[pred] == target).all(), (field, k, target)
    # UDP: the running checksum became 0 at an update before the last one.
    # The field is 0, addresses and ports are the new ones, and the later
    # updates were skipped: carried on from 0 they would have left a
    # non-zero value.
    rw = b.rw
    stuck = ((t["field"] == H.F_L4) & (t["udp"] != 0) & (t["target"] == 0)
             & np.isin(t["k"], (2, 4, 5)) & (rw["ops"] == 0x3F))
    assert stuck.sum() >= 3 * 4 * 16            # k = 2, 4, 5; four UDP bases; 16 m
    assert (l4ck[stuck] == 0).all() and (st[stuck] == 3).all()
    o3, o4 = off[stuck] + meta["l3"][stuck], off[stuck] + meta["l4"][stuck]
    for i in range(4):
        assert (out[o3 + 12 + i] == ((rw["src"][stuck] >> (24 - 8 * i)) & 0xFF)).all()
        assert (out[o3 + 16 + i] == ((rw["dst"][stuck] >> (24 - 8 * i)) & 0xFF)).all()
    assert (_be16(out, o4) == rw["sport"][stuck]).all()
    assert (_be16(out, o4 + 2) == rw["dport"][stuck]).all()
    n_carried = 0
    for i in np.nonzero(stuck)[0][:200]:
        f = b.buf[int(off[i]):int(off[i]) + int(b.lens[i])]
        _, l4u = H._pairs(f, int(meta["l3"][i]), int(meta["l4"][i]), H.K_UDP, rw[i], 0x3F)
        c0 = int(_be16(b.buf, off[i:i + 1] + meta["l4"][i] + 6)[0])
        n_carried += int(H.run_updates(c0, l4u, False)[0][-1]) != 0
    assert n_carried >= 190
    # plain value pairs: a transmitted UDP checksum of 0 stays 0
    sets = (t["field"] == H.F_SET) & (t["udp"] != 0)
    l4in = _be16(b.buf, off + meta["l4"] + meta["cko"])
    assert ((l4in == 0) & sets).sum() >= 6 * 4 * 16
    assert (l4ck[sets & (l4in == 0)] == 0).all()
