"""Writes tests/golden/tunnel.npz: the fixture frames of tests/tungen.py and
what the GRE tunnel contracts make of them.  Encap: frames, the tunnel table,
idx, id_base and, per way of choosing the tunnel (tungen.modes), out = the
DONE slots back to back, out_len, status; nr_* = the lengths and statuses of
the 'idx' mode at the out_stride that gives some frames NOROOM.  Decap:
dframes and their statuses and descriptors.  The expected bytes come from
tungen's NumPy restatement; before anything is written every DONE slot is
pinned to the reference (oracle/_ref/libpptkref.so, tungen.check_with): its
ip_hdr_cksum_calc is 0 on the outer header, its ip_set_hdr_cksum_calc changes
no byte, its receive parse sees a valid IPv4 packet of protocol 47 between
the tunnel's addresses at l3_off 14, and its records of slot[38:] are those
of the original frame.

    python tests/golden/gen_tunnel_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import framegen  # noqa: E402
import tungen    # noqa: E402


def main():
    from oracle.oracle import Reference
    ref = Reference()
    frames = tungen.encap_frames()
    n = len(frames)
    buf, off, lens = framegen.pack(frames)
    z = dict(frames=buf, off=off, len=lens, tun=tungen.tunnels().view(np.uint8),
             idx=tungen.encap_idx(n), id_base=np.array([tungen.ID_BASE], np.uint32))
    checked = 0
    for name, (tun, idx) in tungen.modes(n).items():
        r = tungen.encap_batch(frames, tun, idx, tungen.ID_BASE)
        checked += tungen.check_with(ref, frames, r, tun, tungen.mode_idx(name, n))
        z[f"{name}_out"] = np.frombuffer(b"".join(s for s in r["slots"] if s), np.uint8)
        z[f"{name}_out_len"], z[f"{name}_status"] = r["out_len"], r["status"]
    tun, idx = tungen.modes(n)["idx"]
    r = tungen.encap_batch(frames, tun, idx, tungen.ID_BASE, tungen.NR_STRIDE)
    z["nr_out_len"], z["nr_status"] = r["out_len"], r["status"]

    dframes = tungen.decap_frames()
    dbuf, doff, dlen = framegen.pack(dframes)
    d = tungen.decap_batch(dframes, doff)
    z.update(dframes=dbuf, doff=doff, dlen=dlen, d_status=d["status"], d_in_off=d["in_off"],
             d_in_len=d["in_len"])
    path = os.path.join(HERE, "tunnel.npz")
    np.savez_compressed(path, **z)
    print(f"{n} encap frames, {checked} slots checked against the reference, "
          f"{len(dframes)} decap frames, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
