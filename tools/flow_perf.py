"""MEASUREMENT (DESIGN.md section 14 "Flow table"): pptk_flow_lookup_device
over 16 M records resident in HBM, timed with device events, beside
harness/rwmix.py's speed-of-light kernels reading 64 B and writing 5 B per
record on the same GPU in the same run, and beside pptk_flow_lookup_host on
one host core over 1 M of the same records.

    python tools/flow_perf.py [--n 16777216] [--reps 9] [--lib PATH ...]

Records.  harness/synth.py C64 frames go through the receive kernel; the
subjects among their records, one per flow hash, in random order, are the
pool of flows.  A table of S slots at load L holds the first S * L flows of
the pool.  The n records looked up are drawn from the pool: nine in ten from
the flows in the table (uniformly, so flows repeat), one in ten from flows
that are never inserted -- a hit rate of about 0.9.  Tables: 2^16 slots (4 MB,
L2-sized), 2^21 (128 MB, inside the Infinity Cache), 2^24 (1 GB, HBM), each
at load 0.25 and 0.5.

--lib: A/B builds of the library (make abvariant NAME=flow4
DEFS=-DPPTK_FLOW_TEAM=4); every library looks up in the same table (the image
is plain data) in the same process, the repetitions alternating between them:
two warm-up rounds, then the median of --reps.  One JSON line per case.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--lib", action="append", default=[])
    ap.add_argument("--slots", type=int, nargs="*", default=[1 << 16, 1 << 21, 1 << 24])
    ap.add_argument("--no-sol", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch
    from harness import rwmix, synth
    from pptk_amd.records import F_MALFORMED, F_PARSED, FLOW_ST_HIT
    from pptk_amd.rx import RxContext

    assert torch.cuda.is_available(), "flow_perf needs a GPU"
    dev = torch.device("cuda:0")
    n = args.n
    libs = args.lib or [None]
    ctxs = {os.path.basename(os.path.dirname(p)) if p else "product": RxContext(0, lib_path=p)
            for p in libs}
    first = next(iter(ctxs.values()))
    fmax = max(args.slots) // 2            # the most flows any table holds

    # the pool: one subject record per flow hash, in random order
    npool = max(n, 2 * fmax + (1 << 20))
    b = synth.make_batch("c64", npool, dev)
    pool = first.batch_device(b["frames"], npool, stride=b["stride"], fixed_len=b["fixed_len"],
                              max_len=b["max_len"])
    torch.cuda.synchronize()
    del b
    p64 = pool.view(torch.int64)           # (npool, 8): word 0 the hash, word 6 holds the flags
    flags = (p64[:, 6] >> 48) & 0xFFFF
    subject = (flags & (F_PARSED | F_MALFORMED)) == F_PARSED
    hs, order = torch.sort(p64[:, 0])
    keep = torch.ones(npool, dtype=torch.bool, device=dev)
    keep[1:] = hs[1:] != hs[:-1]
    ids = order[keep & subject[order]]
    g = torch.Generator(device=dev)
    g.manual_seed(0xF10)
    ids = ids[torch.randperm(ids.numel(), device=dev, generator=g)]
    nflows = ids.numel()
    assert nflows >= fmax + (1 << 16), (nflows, fmax)
    del hs, order, keep, flags, subject

    # the records looked up: 0.9 from flows [0, F), 0.1 from flows [fmax, nflows)
    host_flows = p64[ids[:fmax]].cpu().numpy().view(np.uint8).reshape(-1, 64)
    u = torch.rand(n, device=dev, generator=g)
    miss = fmax + (torch.rand(n, device=dev, generator=g) * (nflows - fmax)).long()
    d_idx = torch.empty(n, dtype=torch.int32, device=dev)
    d_st = torch.empty(n, dtype=torch.uint8, device=dev)
    sol = None

    for slots in args.slots:
        t = first.flow_table(slots)
        held = 0
        for load in (0.25, 0.5):
            F = int(slots * load)
            t0 = time.perf_counter()
            done, _ = t.insert_recs(host_flows[held:F], np.arange(held, F, dtype=np.uint32))
            assert done == F - held
            held = F
            insert_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            up = t.sync()
            sync_s = time.perf_counter() - t0
            pick = torch.where(u < 0.9, (torch.rand(n, device=dev, generator=g) * F).long(), miss)
            recs = p64[ids[pick]].view(torch.uint8)     # (n, 64), resident in HBM
            del pick
            st = t.stats()
            res = {"slots": slots, "image_MB": slots * 64 >> 20, "load": load, "flows": F, "n": n,
                   "probe_limit": st["probe_limit"], "insert_s": round(insert_s, 3),
                   "sync_s": round(sync_s, 3), "sync_bytes": up}
            ts = {k: [] for k in ctxs}
            for r in range(args.reps + 2):          # two warm-up rounds
                for k, c in ctxs.items():           # alternating between the libraries
                    ms = timed(lambda: c.flow_lookup_device(t, recs, idx=d_idx, status=d_st), torch)
                    if r >= 2:
                        ts[k].append(ms)
            res["lookup_ms"] = {k: round(median(v), 4) for k, v in ts.items()}
            res["lookup_ms_min_max"] = {k: [round(min(v), 4), round(max(v), 4)]
                                        for k, v in ts.items()}
            res["Mrec_per_s"] = {k: round(n / v / 1e3, 1) for k, v in res["lookup_ms"].items()}
            res["hit_rate"] = round(float(((d_st & FLOW_ST_HIT) != 0).float().mean().item()), 4)
            # one host core over 1 M of the same records, and the same answers
            m = min(n, 1 << 20)
            hrecs = recs[:m].cpu().numpy()
            t0 = time.perf_counter()
            hi, hst = t.lookup_host(hrecs)
            host_s = time.perf_counter() - t0
            assert np.array_equal(hi, d_idx[:m].cpu().numpy().view(np.uint32))
            assert np.array_equal(hst, d_st[:m].cpu().numpy())
            res["host_ms_per_1M"] = round(host_s * 1e3 * (1 << 20) / m, 2)
            res["host_Mrec_per_s"] = round(m / host_s / 1e6, 2)
            if not args.no_sol:
                if sol is None:     # the same bytes for every case: 64 B read, 5 B written per record
                    out = torch.empty((n // 64) * 320, dtype=torch.uint8, device=dev)
                    ms, how = rwmix.sol_ms(recs.reshape(-1), n, out, 320, rb=4096)
                    sol = (round(ms, 4), how)
                    del out
                res["sol_ms"], res["sol_shape"] = sol
                res["over_sol"] = {k: round(v / sol[0], 3) for k, v in res["lookup_ms"].items()}
            print(json.dumps(res), flush=True)
            del recs
        t.close()
        torch.cuda.empty_cache()
    for c in ctxs.values():
        c.close()


if __name__ == "__main__":
    main()
