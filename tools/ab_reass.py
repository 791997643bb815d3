"""BENCH TOOLING: pptk_ip_reass_device on resident batches larger than the
256 MiB cache, hipEvent-timed (median of AB_REPS >= 20 calls after warm-up),
beside -- in the same run -- the harness's trivial read/write stream
(harness/rwmix mix_ms) moving the same read and write bytes and
pptk_ip_fragment_device on the forward case.  The counterpart of
tools/ab_fragment.py: the inputs are the inverse of its cases a and b.

    python tools/ab_reass.py            # cases a, b
    AB_CASES=a AB_REPS=40 python tools/ab_reass.py

  a  the fragments of 1 M x 1500-byte IPv4/UDP frames at mtu 576 (3 each)
  b  the fragments of 128 K x 9000-byte frames at mtu 1500 (7 each)

Every frame is its own datagram (ident and source address count up).  The
fragments are what pptk_ip_fragment_device wrote; they stay in its slots and
are handed on through d_off / d_len descriptors shuffled within windows of 64
datagrams; the records are pptk_rx_batch_device's.  Per case one JSON line:
ms of the call; count_ms = the same call with out_cap = 0 and report_cap = 0
(every pass but the emit's copies runs in full), so ms - count_ms is the emit
kernel's share; read_bytes (every fragment once, plus the 48 record bytes
and one 16-byte side record per fragment) and write_bytes (every slot up to
its length rounded up to 16, plus the per-slot, per-datagram and per-frame
words); sol_ms of the trivial stream and sol_frac = sol_ms / ms; frag_ms of
the forward fragmentation and ratio_to_frag = ms / frag_ms.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tools.ab_fragment import timed   # noqa: E402

WINDOW = 64   # datagrams whose fragments are shuffled among each other


def make_frames(n, length, dev):
    """n frames of `length` bytes from one template, ident = i & 0xffff and
    two source-address bytes = i >> 16, header checksums recomputed."""
    import torch
    import fraggen
    tmpl = np.frombuffer(fraggen.frame4(np.random.default_rng(1), length - 14), np.uint8)
    fr = torch.from_numpy(tmpl.copy()).to(dev).repeat(n).view(n, length)
    i = torch.arange(n, dtype=torch.int64, device=dev)
    fr[:, 18], fr[:, 19] = ((i >> 8) & 255).to(torch.uint8), (i & 255).to(torch.uint8)
    fr[:, 27], fr[:, 28] = ((i >> 16) & 255).to(torch.uint8), ((i >> 24) & 255).to(torch.uint8)
    fr[:, 24:26] = 0
    h = fr[:, 14:34].to(torch.int64)
    s = ((h[:, 0::2] << 8) | h[:, 1::2]).sum(dim=1)
    s = (s & 0xFFFF) + (s >> 16)
    s = ~((s & 0xFFFF) + (s >> 16)) & 0xFFFF
    fr[:, 24], fr[:, 25] = (s >> 8).to(torch.uint8), (s & 255).to(torch.uint8)
    return torch.cat([fr.view(-1), torch.zeros(64, dtype=torch.uint8, device=dev)])


def main():
    import torch
    from harness.rwmix import mix_ms
    from pptk_amd.records import REASS_HDR_DTYPE
    from pptk_amd.rx import RxContext
    dev = torch.device("cuda", 0)
    reps = max(20, int(os.environ.get("AB_REPS", 20)))
    ctx = RxContext(0, bytes(range(1, 17)), max_frame=9216)
    cases = {"a": (int(os.environ.get("AB_FRAMES_A", 1 << 20)), 1500, 576),
             "b": (int(os.environ.get("AB_FRAMES_B", 1 << 17)), 9000, 1500)}
    for case in os.environ.get("AB_CASES", "a,b").split(","):
        n, length, mtu = cases[case]
        frames = make_frames(n, length, dev)
        kw = dict(stride=length, fixed_len=length)
        plan = ctx.ip_fragment_device(frames, n, mtu, 0, **kw)
        torch.cuda.synchronize()
        nfrag = int(plan["totals"][0].item())
        fr = ctx.ip_fragment_device(frames, n, mtu, nfrag, **kw)
        torch.cuda.synchronize()
        assert int(fr["totals"][1].item()) == nfrag and nfrag % n == 0
        keep = {k: fr[k] for k in ("out", "out_len", "out_src", "first", "count", "status", "totals",
                                   "scratch")}
        frag_ms = timed(lambda: ctx.ip_fragment_device(frames, n, mtu, nfrag,
                                                       out_stride=fr["out_stride"], **keep, **kw), reps)
        # the fragments, shuffled within windows of WINDOW datagrams
        per = nfrag // n
        w = WINDOW * per
        g = torch.Generator(device="cpu").manual_seed(7)
        idx = torch.arange(nfrag, dtype=torch.int64)
        nw = nfrag // w
        keys = torch.rand(nw * w, generator=g).view(nw, w).argsort(dim=1)
        idx[:nw * w] = (keys + torch.arange(nw).view(-1, 1) * w).view(-1)
        idx = idx.to(dev)
        d_off = idx * fr["out_stride"]
        d_len = fr["out_len"][:nfrag][idx].contiguous()
        side = torch.zeros((nfrag, 16), dtype=torch.uint8, device=dev)
        recs = ctx.batch_device(fr["out"], nfrag, off=d_off, lens=d_len, max_len=18 + mtu,
                                frag_out=side)
        stride = (length + 15) & ~15
        r = ctx.ip_reass_device(fr["out"], nfrag, recs, side, nfrag, n, stride, report_cap=n,
                                off=d_off, lens=d_len)
        torch.cuda.synchronize()
        hdr = r["hdr"].cpu().numpy().view(REASS_HDR_DTYPE)[0]
        assert int(hdr["written"]) == int(hdr["dgrams"]) == n, hdr
        # every slot is its frame again (slot order = order of the first fragments)
        slot_src = fr["out_src"][:nfrag][idx][r["report"].view(torch.int32).view(-1, 4)[:n, 0].long()]
        probe = torch.arange(0, n, max(1, n // 997), device=dev)
        assert torch.equal(r["out"][probe, :length],
                           frames[:n * length].view(n, length)[slot_src[probe].long()])
        rk = {k: r[k] for k in ("out", "out_len", "report", "dgram", "fstatus", "hdr", "scratch")}
        full = lambda: ctx.ip_reass_device(fr["out"], nfrag, recs, side, nfrag, n, stride,
                                           report_cap=n, off=d_off, lens=d_len, **rk)
        count = lambda: ctx.ip_reass_device(fr["out"], nfrag, recs, side, nfrag, 0, stride,
                                            report_cap=0, off=d_off, lens=d_len, **rk)
        ms, count_ms = timed(full, reps), timed(count, reps)
        rd = int((d_len.to(torch.int64) & 0xFFFF).sum().item()) + (48 + 16 + 10) * nfrag
        wr = n * stride + (2 + 16) * n + 5 * nfrag
        nt = nfrag // 64
        rb, wb = (64 * rd // nfrag + 15) & ~15, max(16, (64 * wr // nfrag + 15) & ~15)
        sol_out = torch.empty(nt * wb, dtype=torch.uint8, device=dev)
        src = fr["out"].view(-1)
        sol = mix_ms(src, rb, min(nt, src.numel() // rb), sol_out, wb, reps=reps)
        print(json.dumps({
            "case": case, "datagrams": n, "fragments": nfrag, "mtu": mtu,
            "ms": round(ms, 4), "count_ms": round(count_ms, 4), "emit_ms": round(ms - count_ms, 4),
            "read_bytes": rd, "write_bytes": wr, "gbs": round((rd + wr) / ms / 1e6, 1),
            "sol_ms": round(sol, 4), "sol_rb": rb, "sol_wb": wb, "sol_frac": round(sol / ms, 3),
            "frag_ms": round(frag_ms, 4), "ratio_to_frag": round(ms / frag_ms, 3)}), flush=True)
        del frames, fr, keep, r, rk, recs, side, sol_out, full, count, plan, src
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
