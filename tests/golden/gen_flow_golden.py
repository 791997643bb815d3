"""Writes tests/golden/flow.npz: the fixture frames of tests/flowgen.py, the
key, flow hash and subject flag the flow-table lookup takes from each, the
flows the fixture table holds (64 slots) with their values, and the lookup's
idx and status.  Everything comes from flowgen's own model; before anything is
written every key and hash is pinned two ways to the reference
(oracle/_ref/libpptkref.so): to the records of Reference.rx_batch over the
frames (tuple, flow_hash and the PARSED / MALFORMED flags of the subject
rule), and to Reference.siphash over the 40 tuple bytes.  At least three pairs
of the inserted flows must share a home slot.

    python tests/golden/gen_flow_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import flowgen  # noqa: E402


def check_pinned(lib, z):
    """Keys, hashes and subject flags of fixture dict z against a per-packet
    implementation (`lib`: the Reference or the Oracle of oracle/oracle.py).
    Returns the number of subjects."""
    from oracle.oracle import make_opts
    from pptk_amd.records import FLOW_KEY_DTYPE
    key = bytes(z["key"])
    recs = lib.rx_batch(z["frames"], z["off"], z["len"], opts=make_opts(key))
    rk, sub = flowgen.keys_of_records(recs)
    assert np.array_equal(sub, z["subject"] != 0), np.nonzero(sub != (z["subject"] != 0))[0]
    keys = np.ascontiguousarray(z["keys"]).view(FLOW_KEY_DTYPE).reshape(-1)
    assert np.array_equal(rk[sub], keys[sub])
    assert np.array_equal(recs["flow_hash"][sub], z["hashes"][sub])
    for k, h in zip(z["keys"][sub], z["hashes"][sub]):
        t = bytes(k)
        tup = t[:32] + t[33:34] + t[32:33] + t[35:36] + t[34:35] + t[36:]   # ports big-endian
        assert lib.siphash(key, tup) == int(h)
    for k, h in zip(z["flow_keys"], z["flow_hashes"]):
        t = bytes(k)
        tup = t[:32] + t[33:34] + t[32:33] + t[35:36] + t[34:35] + t[36:]
        assert lib.siphash(key, tup) == int(h)
    return int(sub.sum())


def main():
    from oracle.oracle import Reference
    z = flowgen.fixture()
    nsub = check_pinned(Reference(), z)
    pairs = flowgen.shared_home_pairs(flowgen.fixture_flows())
    assert pairs >= 3, pairs
    assert 0 in z["flow_values"] and 0xFFFFFFFE in z["flow_values"]
    path = os.path.join(HERE, "flow.npz")
    np.savez_compressed(path, **z)
    hits = int((z["status"] == 3).sum())
    print(f"{len(z['off'])} frames, {nsub} subjects, {len(z['flow_values'])} flows "
          f"({pairs} pairs share a home slot), {hits} hits, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 100_000


if __name__ == "__main__":
    main()
