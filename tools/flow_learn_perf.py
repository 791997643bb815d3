"""MEASUREMENT (DESIGN.md section 16 "Flow learning"): pptk_flow_learn_device
over 16 M records resident in HBM, timed with device events, beside three
yardsticks taken in the same process: harness/rwmix.py's fastest stream kernel
over the n status bytes (the floor: the call is eight launches and does not
reach it), pptk_flow_lookup_device on the same batch (the step before this
one, which reads 64 B per frame where this call reads 1 B), and
pptk_flow_learn_host on one host core over the first 1 M records, whose
answer the device's must equal.

    python tools/flow_learn_perf.py [--n 16777216] [--reps 9] [--lib PATH]

Records.  harness/synth.py C64 frames go through the receive kernel; the
subjects among their records, one per flow hash, in random order, are the
pool of flows.  A table of 2^21 slots holds the first 2^19 of them.  A batch
with miss share p draws each of its n records from those flows with
probability 1 - p and from 2^16 flows that are not in the table with
probability p; the lookup writes the status bytes the learn call reads.
Cases: p = 0, 0.001, 0.01, 0.1 with max_candidates 2^21 (every candidate
considered) and cap 2^16; and a flood, every frame a candidate (the status
forced to SUBJECT) of a distinct flow as far as the pool reaches, with
max_candidates 2^16.  Two warm-up rounds, then the median of --reps, lookup
and learn alternating.  One JSON line per case, also appended to
profiles/flow_learn/flow_learn_perf.jsonl.
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
    ap.add_argument("--lib", default=None)
    ap.add_argument("--no-sol", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_learn",
                                                  "flow_learn_perf.jsonl"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from harness import rwmix, synth
    from pptk_amd.records import (F_MALFORMED, F_PARSED, FLOW_LEARN_HDR_DTYPE, FLOW_ST_SUBJECT,
                                  REC_DTYPE)
    from pptk_amd.rx import (RxContext, flow_learn_host, flow_learn_scratch_bytes,
                             flow_learn_shape)

    assert torch.cuda.is_available(), "flow_learn_perf needs a GPU"
    dev = torch.device("cuda:0")
    n = args.n
    ctx = RxContext(0, lib_path=args.lib)
    slots, known, fresh, cap = 1 << 21, 1 << 19, 1 << 16, 1 << 16
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    # the pool: one subject record per flow hash, in random order
    npool = n + (1 << 20)
    b = synth.make_batch("c64", npool, dev)
    pool = ctx.batch_device(b["frames"], npool, stride=b["stride"], fixed_len=b["fixed_len"],
                            max_len=b["max_len"])
    torch.cuda.synchronize()
    del b
    p64 = pool.view(torch.int64).view(-1, 8)   # word 0 the hash, word 6 holds the flags
    flags = (p64[:, 6] >> 48) & 0xFFFF
    subject = (flags & (F_PARSED | F_MALFORMED)) == F_PARSED
    hs, order = torch.sort(p64[:, 0])
    keep = torch.ones(npool, dtype=torch.bool, device=dev)
    keep[1:] = hs[1:] != hs[:-1]
    ids = order[keep & subject[order]]
    g = torch.Generator(device=dev)
    g.manual_seed(0x1EA2)
    ids = ids[torch.randperm(ids.numel(), device=dev, generator=g)]
    nflows = ids.numel()
    assert nflows >= known + fresh, (nflows, known + fresh)
    del hs, order, keep, flags, subject

    t = ctx.flow_table(slots)
    host_flows = p64[ids[:known]].cpu().numpy().view(np.uint8).reshape(-1, 64)
    done, _ = t.insert_recs(host_flows, np.arange(known, dtype=np.uint32))
    assert done == known
    t.sync()
    del host_flows

    d_idx = torch.empty(n, dtype=torch.int32, device=dev)
    d_st = torch.empty(n, dtype=torch.uint8, device=dev)
    sol = None
    if not args.no_sol:   # the bytes every case reads for all n frames: 1 per frame, in 4 KB tiles
        tiles = n // 4096
        inp = torch.empty(tiles * 4096, dtype=torch.uint8, device=dev)
        out = torch.empty(tiles * 16, dtype=torch.uint8, device=dev)
        ms, how = rwmix.sol_ms(inp, tiles * 64, out, 16, rb=4096)
        sol = (round(ms, 4), how)
        del inp, out

    def case_batch(name, share):
        if name == "flood":
            pick = torch.arange(n, device=dev) % nflows
            recs = p64[ids[pick]].view(torch.uint8)
            return recs, 1 << 16, True
        u = torch.rand(n, device=dev, generator=g)
        hit = (torch.rand(n, device=dev, generator=g) * known).long()
        miss = known + (torch.rand(n, device=dev, generator=g) * fresh).long()
        recs = p64[ids[torch.where(u < share, miss, hit)]].view(torch.uint8)
        return recs, 1 << 21, False

    with open(args.out, "a") as log:
        for name, share in (("miss_0", 0.0), ("miss_0.001", 0.001), ("miss_0.01", 0.01),
                            ("miss_0.1", 0.1), ("flood", 1.0)):
            recs, maxc, force = case_batch(name, share)
            need = flow_learn_scratch_bytes(n, maxc)
            bufs = dict(new_recs=torch.empty(cap * 64, dtype=torch.uint8, device=dev),
                        first=torch.empty(cap, dtype=torch.int32, device=dev),
                        packets=torch.empty(cap, dtype=torch.int32, device=dev),
                        hdr=torch.empty(4, dtype=torch.int64, device=dev),
                        scratch=torch.empty(need, dtype=torch.uint8, device=dev))
            res = {"case": name, "n": n, "miss_share": share, "max_candidates": maxc, "cap": cap,
                   "table_slots": slots, "table_flows": known, "new_flows": fresh,
                   "shape": list(flow_learn_shape(args.lib)), "scratch_MB": round(need / 2**20, 2)}
            lk, ln = [], []
            for r in range(args.reps + 2):          # two warm-up rounds
                ms = timed(lambda: ctx.flow_lookup_device(t, recs, idx=d_idx, status=d_st), torch)
                if force:
                    d_st.fill_(FLOW_ST_SUBJECT)
                    torch.cuda.synchronize()
                ms2 = timed(lambda: ctx.flow_learn_device(recs, d_st, maxc, cap, **bufs), torch)
                if r >= 2:
                    lk.append(ms)
                    ln.append(ms2)
            hdr = bufs["hdr"].cpu().numpy().view(FLOW_LEARN_HDR_DTYPE)[0]
            res["hdr"] = [int(x) for x in hdr]
            res["learn_ms"] = round(median(ln), 4)
            res["learn_ms_min_max"] = [round(min(ln), 4), round(max(ln), 4)]
            res["lookup_ms"] = round(median(lk), 4)
            res["lookup_ms_min_max"] = [round(min(lk), 4), round(max(lk), 4)]
            res["learn_over_lookup"] = round(res["learn_ms"] / res["lookup_ms"], 3)
            res["Mframes_per_s"] = round(n / res["learn_ms"] / 1e3, 1)
            res["download_bytes"] = 32 + int(hdr["written"]) * 72
            # one host core over the first 1 M records, and the same answer from the device
            m = min(n, 1 << 20)
            hrecs = recs[:m].cpu().numpy().reshape(-1).view(REC_DTYPE)
            hst = d_st[:m].cpu().numpy()
            t0 = time.perf_counter()
            hh, hnr, hfirst, hpk = flow_learn_host(hrecs, hst, maxc, cap)
            host_s = time.perf_counter() - t0
            res["host_ms_per_1M"] = round(host_s * 1e3 * (1 << 20) / m, 2)
            ctx.flow_learn_device(recs[:m], d_st[:m], maxc, cap, n=m, **bufs)
            torch.cuda.synchronize()
            w = int(hh["written"])
            assert bufs["hdr"].cpu().numpy().view(np.uint64).tolist() == [int(x) for x in hh], name
            assert np.array_equal(bufs["new_recs"][:64 * w].cpu().numpy(), hnr.view(np.uint8)), name
            assert np.array_equal(bufs["first"][:w].cpu().numpy().view(np.uint32), hfirst), name
            assert np.array_equal(bufs["packets"][:w].cpu().numpy().view(np.uint32), hpk), name
            res["equals_host"] = True
            if sol:
                res["sol_ms"], res["sol_shape"] = sol
                res["over_sol"] = round(res["learn_ms"] / sol[0], 2)
            line = json.dumps(res)
            print(line, flush=True)
            log.write(line + "\n")
            del recs, bufs
            torch.cuda.empty_cache()
    t.close()
    ctx.close()


if __name__ == "__main__":
    main()
