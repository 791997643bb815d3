"""MEASUREMENT (DESIGN.md section 15 "Flow state"): pptk_flow_account_device
over 16 M flow indices resident in HBM, timed with device events, the
aggregated (default) and the direct build alternating in one process, beside
harness/rwmix.py's fastest stream kernel over the bytes the call reads (6 B
per frame: a floor no accounting reaches) and beside pptk_flow_account_host
on one host core over 1 M of the same indices, whose answer the device's must
equal.

    make abvariant NAME=flowstat_direct DEFS=-DPPTK_FLOWSTAT_DIRECT=1
    python tools/flowstats_perf.py --lib pptk_amd/libpptkrx.so \\
        --lib build/ab_flowstat_direct/libpptkrx.so [--n 16777216] [--reps 9]

Cases: uniform over 2^10, 2^16, 2^20 and 2^24 flows; 90 % of the frames in 64
flows over a uniform 2^20 background; every frame in one flow; every frame
unmatched; bursts of 32 frames per flow (uniform over 2^20).  The indices are
generated on the device from a seed; the lengths are uniform in [64, 1518].
Two warm-up rounds, then the median of --reps.  One JSON line per case, also
appended to profiles/flowstats/flowstats_perf.jsonl.
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


def cases(n, dev, g, torch):
    """(name, stats_count, idx int32 tensor) one at a time."""
    def uni(flows):
        return torch.randint(0, flows, (n,), device=dev, generator=g, dtype=torch.int32)

    for bits in (10, 16, 20, 24):
        yield f"uniform_2^{bits}", 1 << bits, uni(1 << bits)
    hot = torch.rand(n, device=dev, generator=g) < 0.9
    yield "hot64_over_2^20", 1 << 20, torch.where(hot, uni(64) * 16381, uni(1 << 20))
    yield "one_flow", 1 << 20, torch.full((n,), 12345, dtype=torch.int32, device=dev)
    yield "all_unmatched", 1 << 20, torch.full((n,), -1, dtype=torch.int32, device=dev)
    yield "bursts_of_32", 1 << 20, uni(1 << 20)[: (n + 31) // 32].repeat_interleave(32)[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--lib", action="append", default=[])
    ap.add_argument("--no-sol", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flowstats",
                                                  "flowstats_perf.jsonl"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from harness import rwmix
    from pptk_amd.records import FLOW_STATS_DTYPE
    from pptk_amd.rx import RxContext, flow_account_host, flow_account_shape, flow_stats_array

    assert torch.cuda.is_available(), "flowstats_perf needs a GPU"
    dev = torch.device("cuda:0")
    n = args.n
    libs = args.lib or [None]
    ctxs, shapes = {}, {}
    for p in libs:
        S, K = flow_account_shape(p)
        name = "direct" if K == 0 else "aggregated"
        assert name not in ctxs, "two libraries of one shape"
        ctxs[name] = RxContext(0, lib_path=p)
        shapes[name] = [S, K]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    g = torch.Generator(device=dev)
    g.manual_seed(0xF105)
    d_len = torch.randint(64, 1519, (n,), device=dev, generator=g, dtype=torch.int16)
    sol = None
    if not args.no_sol:   # the bytes every case reads: 4 + 2 per frame, in 4 KB tiles
        tiles = n * 6 // 4096
        inp = torch.empty(tiles * 4096, dtype=torch.uint8, device=dev)
        out = torch.empty(tiles * 16, dtype=torch.uint8, device=dev)
        ms, how = rwmix.sol_ms(inp, tiles * 64, out, 16, rb=4096)
        sol = (round(ms, 4), how)
        del inp, out
    total = {k: 0.0 for k in ctxs}
    with open(args.out, "a") as log:
        for name, count, d_idx in cases(n, dev, g, torch):
            d_stats = torch.zeros(count * 32, dtype=torch.uint8, device=dev)
            d_um = torch.zeros(32, dtype=torch.uint8, device=dev)
            res = {"case": name, "n": n, "stats_count": count, "shapes": shapes}
            ts = {k: [] for k in ctxs}
            for r in range(args.reps + 2):          # two warm-up rounds
                for k, c in ctxs.items():           # alternating between the builds
                    ms = timed(lambda: c.flow_account_device(d_idx, d_stats, 1000 + r, lens=d_len,
                                                             unmatched=d_um), torch)
                    if r >= 2:
                        ts[k].append(ms)
            res["account_ms"] = {k: round(median(v), 4) for k, v in ts.items()}
            res["account_ms_min_max"] = {k: [round(min(v), 4), round(max(v), 4)]
                                         for k, v in ts.items()}
            res["Mframes_per_s"] = {k: round(n / v / 1e3, 1) for k, v in res["account_ms"].items()}
            # 24 bytes of read-modify-write per frame when every frame is its own three atomics
            res["direct_atomic_GB_per_s"] = (round(n * 24 / res["account_ms"]["direct"] / 1e6, 1)
                                             if "direct" in ctxs else None)
            for k, v in res["account_ms"].items():
                total[k] += v
            # every build against one host core over 1 M of the same indices
            m = min(n, 1 << 20)
            h_idx = d_idx[:m].cpu().numpy().view(np.uint32)
            h_len = d_len[:m].cpu().numpy().view(np.uint16)
            want, wum = flow_stats_array(count), flow_stats_array(1)
            t0 = time.perf_counter()
            flow_account_host(h_idx, want, 7, lens=h_len, unmatched=wum)
            host_s = time.perf_counter() - t0
            res["host_ms_per_1M"] = round(host_s * 1e3 * (1 << 20) / m, 2)
            for k, c in ctxs.items():
                d_stats.zero_()
                d_um.zero_()
                c.flow_account_device(d_idx[:m], d_stats, 7, lens=d_len[:m], unmatched=d_um)
                torch.cuda.synchronize()
                got = d_stats.cpu().numpy().view(FLOW_STATS_DTYPE)
                gum = d_um.cpu().numpy().view(FLOW_STATS_DTYPE)
                assert all(np.array_equal(got[f], want[f]) and np.array_equal(gum[f], wum[f])
                           for f in FLOW_STATS_DTYPE.names), (name, k)
            res["equals_host"] = True
            if sol:
                res["sol_ms"], res["sol_shape"] = sol
                res["over_sol"] = {k: round(v / sol[0], 2) for k, v in res["account_ms"].items()}
            line = json.dumps(res)
            print(line, flush=True)
            log.write(line + "\n")
            del d_idx, d_stats
            torch.cuda.empty_cache()
        line = json.dumps({"case": "total", "account_ms": {k: round(v, 4) for k, v in total.items()}})
        print(line, flush=True)
        log.write(line + "\n")
    for c in ctxs.values():
        c.close()


if __name__ == "__main__":
    main()
