"""Models and input generators for the flow-state tests (include/pptk_rx.h
"Flow state"): the accounting rule in NumPy (np.add.at; 64-bit sums wrap as
the C ones do), the idle rule of pptk_flow_table_expire in Python integers
over the dict model of tests/flowgen.py, and the index distributions the
accounting kernel is aimed at."""
import numpy as np

from pptk_amd.records import FLOW_NONE, FLOW_STATS_DTYPE
from pptk_amd.rx import flow_stats_array

SENT = 0xA5A5A5A5A5A5A5A5   # what a test puts where nothing may be written


def stats_array(count, pad=0):
    """(whole, stats): an aligned FLOW_STATS_DTYPE array of pad + count + pad
    entries, every word SENT, and its middle count entries with packets,
    bytes and last_seen zeroed (reserved keeps SENT)."""
    whole = flow_stats_array(count + 2 * pad)
    for f in FLOW_STATS_DTYPE.names:
        whole[f] = SENT
    st = whole[pad:pad + count]
    for f in ("packets", "bytes", "last_seen"):
        st[f] = 0
    return whole, st


def account(stats, idx, now, lens=None, fixed_len=0, unmatched=None):
    """The accounting rule, in place on FLOW_STATS_DTYPE arrays."""
    idx = np.asarray(idx, np.uint32)
    L = (np.full(idx.size, fixed_len, np.uint64) if lens is None
         else np.asarray(lens, np.uint16).astype(np.uint64))
    hit = idx.astype(np.uint64) < np.uint64(len(stats))
    with np.errstate(over="ignore"):
        np.add.at(stats["packets"], idx[hit], np.uint64(1))
        np.add.at(stats["bytes"], idx[hit], L[hit])
        seen = np.unique(idx[hit])
        stats["last_seen"][seen] = np.maximum(stats["last_seen"][seen], np.uint64(now))
        miss = int((~hit).sum())
        if unmatched is not None and miss:
            unmatched["packets"][0] += np.uint64(miss)
            unmatched["bytes"][0] += L[~hit].sum(dtype=np.uint64)
            unmatched["last_seen"][0] = max(int(unmatched["last_seen"][0]), now)


def is_idle(value, stats, now, idle):
    """pptk_flow_table_expire's rule for one flow value, in Python integers."""
    return value < len(stats) and int(stats["last_seen"][value]) + idle < now


def idle_entries(model, stats, now, idle):
    """The (hash, key37, value) entries of a flowgen.Model that the rule expires."""
    return [tuple(e) for b in model.buckets.values() for e in b if is_idle(e[2], stats, now, idle)]


def model_drop(model, entries):
    for h, k37, _ in entries:
        assert model.delete(k37 + bytes(3), h) == 0


# ------------------------------------------------------------- distributions
def one_flow(n, count, rng):
    return np.full(n, count // 3, np.uint32)


def all_unmatched(n, count, rng):
    v = np.full(n, FLOW_NONE, np.uint32)
    v[::3] = count            # the first index past the array
    v[1::5] = count + 7
    return v


def distinct(n, count, per_segment, rng):
    """per_segment distinct flows in every run of per_segment frames."""
    assert count >= per_segment
    return ((np.arange(n) % per_segment) * (count // per_segment)).astype(np.uint32)


def strided(n, count, step, rng):
    """Multiples of `step`: colliding homes for any power-of-two mask."""
    m = max(count // step, 1)
    return (rng.integers(0, m, n) * step).astype(np.uint32)


def runs(n, count, rng):
    """Runs of 1..200 equal indices."""
    out = np.empty(0, np.uint32)
    while out.size < n:
        ls = rng.integers(1, 201, 64)
        vs = rng.integers(0, count, 64)
        out = np.concatenate([out, np.repeat(vs, ls).astype(np.uint32)])
    return out[:n]


def mix(n, count, per_segment, rng):
    """All of the above in pieces of random length, with PPTK_FLOW_NONE and
    count - 1, count sprinkled in."""
    parts, have = [], 0
    gens = (one_flow, all_unmatched, runs,
            lambda m, c, r: distinct(m, c, per_segment, r),
            lambda m, c, r: strided(m, c, 4096, r),
            lambda m, c, r: strided(m, c, 65536, r),
            lambda m, c, r: r.integers(0, c, m).astype(np.uint32))
    while have < n:
        m = int(rng.integers(1, max(n // 6, 2)))
        parts.append(gens[int(rng.integers(0, len(gens)))](m, count, rng))
        have += m
    v = np.concatenate(parts)[:n].copy()
    spots = rng.integers(0, n, max(n // 9, 3))
    v[spots] = rng.choice(np.array([FLOW_NONE, count - 1, count], np.uint32), spots.size)
    return v


def lengths(n, rng):
    """uint16 lengths that include 0 and 65535."""
    L = rng.integers(0, 65536, n).astype(np.uint16)
    L[rng.integers(0, n, max(n // 50, 1))] = 65535
    L[rng.integers(0, n, max(n // 50, 1))] = 0
    return L
