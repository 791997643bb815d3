"""ctypes front-end of libpptkrx.so (include/pptk_rx.h) for tests and bench.

The product is the C-ABI library; this module only marshals torch/numpy
buffers into it.  There is no Python or CPU fallback: if the library is
missing, importing this module raises.
"""
import collections
import ctypes
import os

import numpy as np

from .records import REC32_DTYPE, REC_DTYPE

LIB_PATH = os.environ.get("PPTK_RX_LIB") or os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "libpptkrx.so")   # env: A/B builds


class RxOpts(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int), ("key", ctypes.c_uint8 * 16),
                ("iphash_bits4", ctypes.c_uint8), ("iphash_bits6", ctypes.c_uint8),
                ("gather_threads", ctypes.c_uint16), ("iphash_size", ctypes.c_uint32),
                ("max_batch", ctypes.c_uint32), ("max_frame", ctypes.c_uint32),
                ("comm_timeout_ms", ctypes.c_uint32)]


class RxDevBatch(ctypes.Structure):
    _fields_ = [("d_frames", ctypes.c_void_p), ("d_off", ctypes.c_void_p),
                ("d_len", ctypes.c_void_p), ("d_perm", ctypes.c_void_p),
                ("stride", ctypes.c_uint64), ("fixed_len", ctypes.c_uint32),
                ("max_len", ctypes.c_uint32), ("n", ctypes.c_uint64),
                ("d_recs", ctypes.c_void_p), ("d_hash", ctypes.c_void_p),
                ("d_recs32", ctypes.c_void_p), ("d_frag", ctypes.c_void_p),
                ("d_key", ctypes.c_void_p)]


class RxRingSpec(ctypes.Structure):
    """struct pptk_rx_ring_spec (include/pptk_rx.h "Device rings")."""
    _fields_ = [("frame_bytes", ctypes.c_uint64), ("nrec", ctypes.c_uint64),
                ("rec_bytes", ctypes.c_uint32), ("probe_len", ctypes.c_uint32),
                ("frame_cands", ctypes.c_uint32), ("rec_cands", ctypes.c_uint32),
                ("reps", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("budget_bytes", ctypes.c_uint64), ("reserved", ctypes.c_uint64)]


class RxGatherSpec(ctypes.Structure):
    """struct pptk_rx_gather_spec (include/pptk_rx.h)."""
    _fields_ = [("per_rank", ctypes.c_uint64), ("nranks", ctypes.c_int32),
                ("rank", ctypes.c_int32), ("cands", ctypes.c_uint32), ("reps", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("budget_bytes", ctypes.c_uint64)]


class RxGatherC(ctypes.Structure):
    """struct pptk_rx_gather."""
    _fields_ = [("d_out", ctypes.c_void_p * 2), ("per_rank", ctypes.c_uint64),
                ("nranks", ctypes.c_int32), ("rank", ctypes.c_int32), ("device", ctypes.c_int32),
                ("cands", ctypes.c_uint32), ("chosen", ctypes.c_int32),
                ("chosen_ms", ctypes.c_float), ("first_ms", ctypes.c_float),
                ("settle_ms", ctypes.c_uint32), ("freed_bytes", ctypes.c_uint64),
                ("cand_ms", ctypes.c_float * 16)]


assert ctypes.sizeof(RxGatherSpec) == 40 and ctypes.sizeof(RxGatherC) == 128


class RxRingC(ctypes.Structure):
    """struct pptk_rx_ring."""
    _fields_ = [("d_frames", ctypes.c_void_p), ("d_recs", ctypes.c_void_p),
                ("frame_bytes", ctypes.c_uint64), ("nrec", ctypes.c_uint64),
                ("rec_bytes", ctypes.c_uint32), ("device", ctypes.c_int32),
                ("frame_cands", ctypes.c_uint32), ("rec_cands", ctypes.c_uint32),
                ("chosen_frames", ctypes.c_int32), ("chosen_recs", ctypes.c_int32),
                ("chosen_ms", ctypes.c_float), ("first_ms", ctypes.c_float),
                ("probe_frames", ctypes.c_uint64), ("freed_bytes", ctypes.c_uint64),
                ("settle_ms", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


RING_SETTLE = 0x1
RING_PROBE_HASH = 0x2


class _RingOwner:
    """Frees a pptk_rx_ring when the last tensor over it is gone."""

    def __init__(self, L, ring):
        self.L, self.ring = L, ring

    def __del__(self):
        try:
            if self.ring is not None:
                self.L.pptk_rx_ring_free(ctypes.byref(self.ring))
        except Exception:
            pass
        self.ring = None


class _DevMem:
    """A device range as a __cuda_array_interface__ object: torch.as_tensor
    wraps it without copying and keeps it (and so the ring) alive."""

    def __init__(self, owner, ptr, nbytes):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1",
                                         "data": (ptr, False), "version": 3, "strides": None}


class _GatherOwner:
    """Frees a pptk_rx_gather when the last tensor over it is gone."""

    def __init__(self, L, g):
        self.L, self.g = L, g

    def __del__(self):
        try:
            if self.g is not None:
                self.L.pptk_rx_gather_free(ctypes.byref(self.g))
        except Exception:
            pass
        self.g = None


class DeviceGather:
    """Library-placed gather buffers (pptk_rx_gather_alloc): .out[0], .out[1]
    (torch int64, nranks * per_rank each) and the probe .report; freed once
    no tensor over them is referenced."""

    def __init__(self, ctx, g):
        torch = _torch()
        dev = torch.device("cuda", ctx.device)
        own = _GatherOwner(ctx._L, g)
        nb = g.nranks * g.per_rank * 8
        self.out = [torch.as_tensor(_DevMem(own, g.d_out[k], nb), device=dev).view(torch.int64)
                    for k in range(2)]
        self.report = {"candidates": g.cands, "chosen": g.chosen,
                       "chosen_ms": round(g.chosen_ms, 4), "first_ms": round(g.first_ms, 4),
                       "freed_bytes": g.freed_bytes, "settle_ms": g.settle_ms,
                       "candidate_ms": [round(x, 4) for x in g.cand_ms[:g.cands]],
                       "alloc": "pptk_rx_gather_alloc"}


class DeviceRing:
    """Library-owned placed device rings (pptk_rx_ring_alloc): .frames (torch
    uint8, frame_bytes + 64), .recs (torch uint8 (nrec, rec_bytes)) and the
    probe .report.  The rings are freed (pptk_rx_ring_free) once neither
    tensor (nor a view of one) is referenced any more."""

    def __init__(self, ctx, ring):
        torch = _torch()
        dev = torch.device("cuda", ctx.device)
        own = _RingOwner(ctx._L, ring)
        self.frames = torch.as_tensor(_DevMem(own, ring.d_frames, ring.frame_bytes + 64),
                                      device=dev)
        self.recs = torch.as_tensor(_DevMem(own, ring.d_recs, ring.nrec * ring.rec_bytes),
                                    device=dev).view(ring.nrec, ring.rec_bytes)
        self.report = {k: getattr(ring, k) for k in (
            "frame_cands", "rec_cands", "chosen_frames", "chosen_recs", "settle_ms",
            "probe_frames", "freed_bytes")}
        self.report["chosen_ms"] = round(ring.chosen_ms, 4)
        self.report["first_ms"] = round(ring.first_ms, 4)


class LdpPacket(ctypes.Structure):
    """struct ldp_packet (include/ldp_packet.h; reference ldp/ldp.h:98-108)."""
    _fields_ = [("data", ctypes.c_void_p), ("sz", ctypes.c_uint32),
                ("ancillary64", ctypes.c_uint64)]


class Dispatch(ctypes.Structure):
    """struct pptk_dispatch (include/pptk_rx.h "Egress dispatch"): the
    arguments of pptk_tx_dispatch_device / _host; the pointers are addresses."""
    _fields_ = [("n", ctypes.c_uint64), ("port", ctypes.c_void_p), ("idx", ctypes.c_void_p),
                ("flow_port", ctypes.c_void_p), ("flows", ctypes.c_uint64),
                ("subject", ctypes.c_void_p), ("in_port", ctypes.c_void_p),
                ("in_port_all", ctypes.c_uint32), ("nports", ctypes.c_uint32),
                ("miss_code", ctypes.c_uint8), ("pad0", ctypes.c_uint8 * 7),
                ("off", ctypes.c_void_p), ("len", ctypes.c_void_p), ("stride", ctypes.c_uint64),
                ("fixed_len", ctypes.c_uint32), ("pad1", ctypes.c_uint32),
                ("list", ctypes.c_void_p), ("out_off", ctypes.c_void_p),
                ("out_len", ctypes.c_void_p), ("cap", ctypes.c_uint64),
                ("ports", ctypes.c_void_p), ("hdr", ctypes.c_void_p)]


class Gather(ctypes.Structure):
    """struct pptk_gather (include/pptk_rx.h "Egress gather"): the arguments of
    pptk_tx_gather_device / _host; the pointers are addresses."""
    _fields_ = [("frames", ctypes.c_void_p), ("off", ctypes.c_void_p), ("len", ctypes.c_void_p),
                ("stride", ctypes.c_uint64), ("fixed_len", ctypes.c_uint32),
                ("pad0", ctypes.c_uint32), ("n", ctypes.c_uint64), ("list", ctypes.c_void_p),
                ("max_entries", ctypes.c_uint64), ("d_entries", ctypes.c_void_p),
                ("runs", ctypes.c_void_p), ("nports", ctypes.c_uint32),
                ("pad1", ctypes.c_uint32), ("out", ctypes.c_void_p),
                ("out_cap", ctypes.c_uint64), ("pk_off", ctypes.c_void_p),
                ("pk_len", ctypes.c_void_p), ("ports", ctypes.c_void_p),
                ("hdr", ctypes.c_void_p)]


assert ctypes.sizeof(LdpPacket) == 24
assert ctypes.sizeof(Dispatch) == 152
assert ctypes.sizeof(Gather) == 136
assert ctypes.sizeof(RxOpts) == 40

# Every C function this module binds: name -> (restype, argtypes), as its
# prototype in include/*.h states (tests/test_capi.py compares the two).
# Pointers to device memory, opaque handles and byte buffers are vp; lib()
# sets both attributes on every function, so none is left with ctypes'
# defaults (under which a uint64_t argument is cut to an int).
P = ctypes.POINTER
vp, ci, sz, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_float
u16, u32, u64 = ctypes.c_uint16, ctypes.c_uint32, ctypes.c_uint64
_batch, _cksum = (ci, (vp, vp, ci, vp)), (u16, (vp, u16, vp, u16))
_SIGNATURES = {
    # contexts, host batches, zero-copy rings
    "pptk_rx_opts_default": (None, (P(RxOpts),)),
    "pptk_rx_ctx_create": (ci, (P(vp), P(RxOpts))),
    "pptk_rx_ctx_destroy": (None, (vp,)),
    "pptk_rx_batch": _batch,
    "pptk_rx_batch32": _batch,
    "pptk_rx_batch_submit": _batch,
    "pptk_rx_batch_submit32": _batch,
    "pptk_rx_batch_complete": (ci, (vp,)),
    "pptk_rx_batch_pending": (ci, (vp,)),
    "pptk_rx_register_ring": (ci, (vp, vp, sz)),
    "pptk_rx_unregister_ring": (ci, (vp, vp)),
    # device batches and length binning
    "pptk_rx_batch_device": (ci, (vp, P(RxDevBatch), vp)),
    "pptk_rx_bin_scratch_bytes": (sz, (u64,)),
    "pptk_rx_bin_device": (ci, (vp, vp, u64, vp, vp, vp)),
    "pptk_rx_batch_device_mixed": (ci, (vp, P(RxDevBatch), vp, vp, vp)),
    # rate limiter
    "pptk_rx_permit_scratch_bytes": (sz, (u64, u32)),
    "pptk_rx_permit_device": (ci, (vp, vp, vp, u64, ci, vp, vp, vp, vp, vp)),
    "pptk_rx_permit_keys_device": (ci, (vp, vp, u64, ci, vp, vp, vp, vp, vp)),
    "pptk_rx_permit_status": (ci, (vp, vp, vp)),
    "pptk_rx_tokens_refill_device": (ci, (vp, vp, u32, u32, u32, u32, vp)),
    # tx checksums and header edits
    "pptk_tx_cksum_device": (ci, (vp, vp, vp, vp, u64, u32, u64, u32, vp)),
    "pptk_tx_set_side_buffer": (ci, (vp, vp, u64)),
    "pptk_tx_rewrite_device": (ci, (vp, vp, vp, vp, u64, u32, u64, vp, u64, vp, vp)),
    "pptk_tcp_mss_clamp_device": (ci, (vp, vp, vp, vp, u64, u32, u64, u16, u32, vp, vp)),
    "pptk_tcp_seq_translate_device": (ci, (vp, vp, vp, vp, u64, u32, u64, vp, u64, vp, vp, vp)),
    "pptk_tcp_seq_translate_hdr": (u32, (vp, u32, vp)),
    # IPv4 fragmentation
    "pptk_ip_fragment_scratch_bytes": (sz, (u64,)),
    "pptk_ip_fragment_device": (ci, (vp, vp, vp, vp, u64, u32, u64, u32, vp, u64, u64)
                                + (vp,) * 8),
    "pptk_ip_fragment_host": (ci, (vp, u32, u32, vp, u64, u32, vp, vp)),
    # IPv4 reassembly
    "pptk_ip_reass_scratch_bytes": (sz, (u64, u64)),
    "pptk_ip_reass_device": (ci, (vp, vp, vp, vp, u64, u32, u64, vp, vp, u64, vp, u64, u64, vp, vp,
                                  u64, vp, vp, vp, vp, sz, vp)),
    "pptk_ip_reass_host": (ci, (vp, vp, vp, u64, u32, u64, vp, vp, u64, vp, u64, u64, vp, vp, u64,
                                vp, vp, vp)),
    "pptk_ip_reass_shape": (None, (P(u32), P(u32))),
    # GRE tunnel
    "pptk_tunnel_encap_device": (ci, (vp, vp, vp, vp, u64, u32, u64, vp, u64, vp, u32, vp, u64,
                                      vp, vp, vp)),
    "pptk_tunnel_decap_device": (ci, (vp, vp, vp, vp, u64, u32, u64, vp, vp, vp, vp)),
    "pptk_tunnel_encap_host": (u32, (vp, u32, vp, u32, vp, u64, vp)),
    "pptk_tunnel_decap_host": (u32, (vp, u32, vp, vp)),
    # flow table
    "pptk_flow_table_create": (ci, (vp, u32, P(vp))),
    "pptk_flow_table_destroy": (None, (vp,)),
    "pptk_flow_key_from_rec": (None, (vp, vp)),
    "pptk_flow_key_hash": (u64, (vp, vp)),
    "pptk_flow_table_insert": (ci, (vp, vp, u64, u32)),
    "pptk_flow_table_update": (ci, (vp, vp, u64, u32)),
    "pptk_flow_table_delete": (ci, (vp, vp, u64)),
    "pptk_flow_table_find": (ci, (vp, vp, u64, P(u32))),
    "pptk_flow_table_insert_recs": (ci, (vp, vp, u64, vp, vp)),
    "pptk_flow_table_clear": (None, (vp,)),
    "pptk_flow_table_stats": (None, (vp, P(u32), P(u32), P(u32))),
    "pptk_flow_table_sync": (ci, (vp, vp, P(u64))),
    "pptk_flow_lookup_device": (ci, (vp, vp, vp, u64, vp, vp, vp, vp)),
    "pptk_flow_lookup_host": (ci, (vp, vp, u64, vp, vp, vp)),
    # flow state
    "pptk_flow_account_device": (ci, (vp, vp, vp, u32, u64, vp, u64, vp, u64, vp)),
    "pptk_flow_account_host": (ci, (vp, vp, u32, u64, vp, u64, vp, u64)),
    "pptk_flow_stats_reset_device": (ci, (vp, vp, u64, vp, u64, u64, vp)),
    "pptk_flow_account_shape": (None, (P(u32), P(u32))),
    "pptk_flow_table_expire": (ci, (vp, vp, u64, u64, u64, vp, u32)),
    "pptk_tx_rewrite_flow_device": (ci, (vp, vp, vp, vp, u64, u32, u64, vp, u64, vp, vp, vp)),
    # flow learning
    "pptk_flow_learn_scratch_bytes": (sz, (u64, u64)),
    "pptk_flow_learn_device": (ci, (vp, vp, vp, u64, u64, vp, vp, vp, u64, vp, vp, sz, vp)),
    "pptk_flow_learn_host": (ci, (vp, vp, u64, u64, vp, vp, vp, u64, vp)),
    "pptk_flow_learn_shape": (None, (P(u32), P(u32))),
    # egress dispatch
    "pptk_tx_dispatch_scratch_bytes": (sz, (u64, u32)),
    "pptk_tx_dispatch_device": (ci, (vp, P(Dispatch), vp, sz, vp)),
    "pptk_tx_dispatch_host": (ci, (P(Dispatch),)),
    "pptk_tx_dispatch_shape": (None, (P(u32), P(u32))),
    # egress gather
    "pptk_tx_gather_scratch_bytes": (sz, (u64, u32)),
    "pptk_tx_gather_device": (ci, (vp, P(Gather), vp, sz, vp)),
    "pptk_tx_gather_host": (ci, (P(Gather),)),
    "pptk_tx_gather_shape": (None, (P(u32), P(u32))),
    # tuning
    "pptk_rx_set_tuning": (ci, (vp, ci, ci)),
    "pptk_rx_variant_count": (ci, ()),
    "pptk_rx_last_variant": (ci, (vp,)),
    "pptk_rx_autotune": (ci, (vp, P(RxDevBatch), ci, vp)),
    # multi-GPU (RCCL)
    "pptk_rx_device_count": (ci, ()),
    "pptk_rx_comm_uid": (ci, (vp,)),
    "pptk_rx_comm_create": (ci, (vp, ci, ci, vp)),
    "pptk_rx_comm_create_all": (ci, (P(vp), ci)),
    "pptk_rx_comm_destroy": (ci, (vp,)),
    "pptk_rx_comm_abort": (ci, (vp,)),
    "pptk_rx_comm_sync": (ci, (vp, vp, u32)),
    "pptk_rx_comm_info": (ci, (vp, P(ci), P(ci))),
    "pptk_rx_shard_range": (None, (u64, ci, ci, P(u64), P(u64), P(u64))),
    "pptk_rx_allgather_hash": (ci, (vp, vp, u64, vp, vp)),
    "pptk_rx_stream_split": (ci, (vp, ci, P(vp), P(vp))),
    "pptk_rx_stream_destroy": (ci, (vp,)),
    # buffer placement, device rings, gather buffers
    "pptk_rx_place_buffers": (ci, (vp, P(RxDevBatch), P(vp), ci, P(vp), ci, ci, P(ci), P(ci),
                                   P(f32), vp)),
    "pptk_rx_place_records": (ci, (vp, P(RxDevBatch), P(vp), ci, ci, P(ci), P(f32), vp)),
    "pptk_rx_ring_alloc": (ci, (vp, P(RxRingSpec), P(RxRingC), vp)),
    "pptk_rx_ring_free": (ci, (P(RxRingC),)),
    "pptk_rx_gather_alloc": (ci, (vp, P(RxDevBatch), P(RxGatherSpec), P(RxGatherC), vp)),
    "pptk_rx_gather_free": (ci, (P(RxGatherC),)),
    "pptk_rx_version": (ctypes.c_char_p, ()),
    "pptk_rx_abi": (ci, ()),
    # kept per-packet APIs (ipcksum.h, hashseed.h, iphdr.h)
    "ip_cksum_feed": (None, (P(u32), vp, sz)),
    "ip_hdr_cksum_calc": (u16, (vp, u16)),
    "tcp_cksum_calc": _cksum,
    "udp_cksum_calc": _cksum,
    "tcp6_cksum_calc": _cksum,
    "udp6_cksum_calc": _cksum,
    "hash_seed_init": (None, ()),
    "tcp_parse_options": (None, (vp, vp)),
    "tcp_find_sack_ts_headers": (None, (vp, vp)),
    "tcp_find_sack_header": (vp, (vp, P(sz), P(ci))),
}
EXPORTS = tuple(_SIGNATURES)

# Kernel variants, in the order of enum RxVariant (pptk_amd/csrc/rx_internal.h).
VARIANTS = ("T4S1", "T4S2", "T16S2", "T16S6", "T32S3", "T64S2", "T16S7L", "T32S4L",
            "T32S3D7", "T16S6D1", "T8S2", "T16S4", "L4", "M6")
RX_L4 = VARIANTS.index("L4")

_libs = {}
ABI = 6   # include/pptk_rx.h PPTK_RX_ABI


def lib(path=None):
    """Load libpptkrx.so (or the A/B build at `path`) once; raise if it is
    missing (no fallback) or lacks a function of EXPORTS."""
    path = path or LIB_PATH
    if path not in _libs:
        if not os.path.exists(path):
            raise ImportError(f"{path} not built: run `make` or __graft_entry__.build()")
        L = ctypes.CDLL(path)
        missing = [f for f in _SIGNATURES if not hasattr(L, f)]
        if missing:
            raise ImportError(f"{path} lacks {', '.join(missing)}")
        for f, (restype, argtypes) in _SIGNATURES.items():
            fn = getattr(L, f)
            fn.restype, fn.argtypes = restype, argtypes
        if L.pptk_rx_abi() != ABI:   # the struct layouts above are PPTK_RX_ABI's
            raise ImportError(f"{path}: struct layout revision {L.pptk_rx_abi()}, "
                              f"this binding expects {ABI}")
        _libs[path] = L
    return _libs[path]


def _torch():
    """torch, imported at its first use: importing this module does not."""
    import torch
    return torch


def _dp(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _check(rc, name, counts=False):
    """Raise the -errno return `rc` of C function `name` as OSError; with
    `counts` a positive return is the call's result, otherwise an error too."""
    if rc < 0 or (rc and not counts):
        raise OSError(-rc, f"{name} failed ({rc})")
    return rc


def _stream(stream, device):
    """The hipStream_t of `stream`, a torch stream or None = the current one
    of `device`, as a C argument."""
    if stream is None:
        stream = _torch().cuda.current_stream(device)
    return ctypes.c_void_p(stream.cuda_stream)


def _empty(t, shape, dtype, device):
    """`t`, or where it is None an uninitialised torch tensor of `shape` and
    the dtype of that name on `device`."""
    if t is None:
        torch = _torch()
        t = torch.empty(shape, dtype=getattr(torch, dtype), device=device)
    return t


def _ptr(t):
    return None if t is None else t.data_ptr()


def _dev_batch(frames, n, off=None, lens=None, stride=0, fixed_len=0, max_len=0, perm=None,
               recs=None, compact=False, hash_out=None, frag_out=None, key_out=None):
    """struct pptk_rx_dev_batch over torch CUDA tensors (None = a null
    pointer); recs goes into d_recs32 with compact, into d_recs without."""
    r = _ptr(recs)
    return RxDevBatch(_ptr(frames), _ptr(off), _ptr(lens), _ptr(perm), stride, fixed_len,
                      max_len, n, None if compact else r, _ptr(hash_out),
                      r if compact else None, _ptr(frag_out), _ptr(key_out))


def _one_struct(x, arg, struct, nbytes):
    """One C struct as a uint8 array, from a NumPy entry or its bytes."""
    b = np.frombuffer(x.tobytes() if hasattr(x, "tobytes") else bytes(x), np.uint8)
    if b.size != nbytes:
        raise ValueError(f"{arg} must be one struct {struct} ({nbytes} bytes)")
    return b


class RxContext:
    """One pptk_rx_ctx (one per rx thread in a C application)."""

    def __init__(self, device=0, key=bytes(16), iphash_bits4=0, iphash_bits6=0,
                 iphash_size=1, max_batch=8192, max_frame=9216, gather_threads=1,
                 lib_path=None, comm_timeout_ms=0):
        self._L = L = lib(lib_path)
        o = RxOpts()
        L.pptk_rx_opts_default(ctypes.byref(o))
        o.device = device
        for i, b in enumerate(bytes(key)):
            o.key[i] = b
        o.iphash_bits4, o.iphash_bits6, o.iphash_size = iphash_bits4, iphash_bits6, iphash_size
        o.max_batch, o.max_frame, o.gather_threads = max_batch, max_frame, gather_threads
        if comm_timeout_ms:
            o.comm_timeout_ms = comm_timeout_ms
        self._ctx = ctypes.c_void_p()
        self._inflight = collections.deque()   # (pkts, out) of submitted host batches
        _check(L.pptk_rx_ctx_create(ctypes.byref(self._ctx), ctypes.byref(o)),
               "pptk_rx_ctx_create")
        self.device = device

    def set_tuning(self, variant=-1, flags=-1):
        """Force kernel variant / memory-policy flags (speed only; -1 = auto)."""
        _check(self._L.pptk_rx_set_tuning(self._ctx, variant, flags),
               f"pptk_rx_set_tuning({variant}, {flags})")

    def last_variant(self):
        """Kernel variant of the last device batch (-1: none yet)."""
        return self._L.pptk_rx_last_variant(self._ctx)

    def close(self):
        if self._ctx:
            self.stream_join()
            self._L.pptk_rx_ctx_destroy(self._ctx)   # (waits for outstanding submissions)
            self._ctx = ctypes.c_void_p()
            self._inflight.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def batch_device(self, frames, n, off=None, lens=None, stride=0, fixed_len=0,
                     perm=None, recs=None, hash_out=None, max_len=0, stream=None,
                     compact=False, frag_out=None, key_out=None):
        """Asynchronous device batch on `stream` (torch stream or None = current).
        frames/off/lens/perm/recs/hash_out are torch CUDA tensors; compact:
        32-byte struct pptk_rx_rec32 records (recs is (n, 32) bytes);
        frag_out: (n, 16) uint8 tensor of struct pptk_rx_frag side records;
        key_out: (n,) int32 tensor of dense rate-limiter keys (d_key)."""
        recs = _empty(recs, (n, 32 if compact else 64), "uint8", frames.device)
        b = _dev_batch(frames, n, off, lens, stride, fixed_len, max_len, perm, recs, compact,
                       hash_out, frag_out, key_out)
        _check(self._L.pptk_rx_batch_device(self._ctx, ctypes.byref(b),
                                            _stream(stream, frames.device)),
               "pptk_rx_batch_device")
        return recs

    def autotune(self, frames, n, off=None, lens=None, stride=0, fixed_len=0, max_len=0,
                 recs=None, compact=False, reps=5, stream=None):
        """pptk_rx_autotune on this batch layout (synchronous): later device
        batches of the same shape use the fastest interchangeable kernel
        variant; returns its name (VARIANTS)."""
        recs = _empty(recs, (n, 32 if compact else 64), "uint8", frames.device)
        b = _dev_batch(frames, n, off, lens, stride, fixed_len, max_len, None, recs, compact)
        _check(self._L.pptk_rx_autotune(self._ctx, ctypes.byref(b), reps,
                                        _stream(stream, frames.device)), "pptk_rx_autotune")
        return self.tuned_variant(frames, n, off, lens, stride, fixed_len, max_len, compact)

    def place_records(self, frames, n, cands, off=None, lens=None, stride=0, fixed_len=0,
                      max_len=0, compact=False, reps=3, stream=None):
        """pptk_rx_place_records: run the batch into each candidate record
        buffer (torch uint8 CUDA tensors of n x 64 or n x 32 bytes) and
        return (index of the fastest, per-candidate median ms)."""
        arr = (ctypes.c_void_p * max(1, len(cands)))(*[t.data_ptr() for t in cands])
        b = _dev_batch(frames, n, off, lens, stride, fixed_len, max_len, None,
                       cands[0] if cands else None, compact)
        best = ctypes.c_int(-1)
        ms = (ctypes.c_float * max(1, len(cands)))()
        _check(self._L.pptk_rx_place_records(self._ctx, ctypes.byref(b), arr, len(cands), reps,
                                             ctypes.byref(best), ms,
                                             _stream(stream, frames.device)),
               "pptk_rx_place_records")
        return best.value, [round(x, 4) for x in ms[:len(cands)]]

    def place_buffers(self, frame_cands, n, rec_cands, off=None, lens=None, stride=0,
                      fixed_len=0, max_len=0, compact=False, reps=3, stream=None):
        """pptk_rx_place_buffers: the batch (the same bytes in every frame
        candidate) on every (frames, records) pair; returns (frame index,
        record index, median ms per pair, frames-major)."""
        nf, nr = len(frame_cands), len(rec_cands)
        fa = (ctypes.c_void_p * max(1, nf))(*[t.data_ptr() for t in frame_cands])
        ra = (ctypes.c_void_p * max(1, nr))(*[t.data_ptr() for t in rec_cands])
        b = _dev_batch(frame_cands[0] if nf else None, n, off, lens, stride, fixed_len, max_len,
                       None, rec_cands[0] if nr else None, compact)
        bf, br = ctypes.c_int(-1), ctypes.c_int(-1)
        ms = (ctypes.c_float * max(1, nf * nr))()
        dev = frame_cands[0].device if nf else _torch().device("cuda", self.device)
        _check(self._L.pptk_rx_place_buffers(self._ctx, ctypes.byref(b), fa, nf, ra, nr, reps,
                                             ctypes.byref(bf), ctypes.byref(br), ms,
                                             _stream(stream, dev)), "pptk_rx_place_buffers")
        return bf.value, br.value, [round(x, 4) for x in ms[:nf * nr]]

    def ring_alloc(self, frame_bytes, nrec, rec_bytes=64, probe_len=0, frame_cands=0,
                   rec_cands=0, reps=0, settle=False, stream=None, budget_bytes=0,
                   probe_hash=False):
        """pptk_rx_ring_alloc: placed device frame and record rings (a
        DeviceRing; its .report carries the probe).  probe_hash: the probe
        batches also write dense flow hashes (PPTK_RX_RING_PROBE_HASH)."""
        spec = RxRingSpec(frame_bytes, nrec, rec_bytes, probe_len, frame_cands, rec_cands, reps,
                          (RING_SETTLE if settle else 0) | (RING_PROBE_HASH if probe_hash else 0),
                          budget_bytes, 0)
        ring = RxRingC()
        _check(self._L.pptk_rx_ring_alloc(self._ctx, ctypes.byref(spec), ctypes.byref(ring),
                                          _stream(stream, self.device)), "pptk_rx_ring_alloc")
        return DeviceRing(self, ring)

    def gather_alloc(self, frames, n, per_rank, nranks, rank, off=None, lens=None, stride=0,
                     fixed_len=0, max_len=0, recs=None, compact=False, cands=0, reps=0,
                     settle=False, budget_bytes=0, stream=None):
        """pptk_rx_gather_alloc: this rank's two gather buffers, placed by a
        probe that runs the batch (frames/recs as for batch_device) with its
        hashes into each candidate; a DeviceGather."""
        recs = _empty(recs, (n, 32 if compact else 64), "uint8", frames.device)
        b = _dev_batch(frames, n, off, lens, stride, fixed_len, max_len, None, recs, compact)
        spec = RxGatherSpec(per_rank, nranks, rank, cands, reps, RING_SETTLE if settle else 0, 0,
                            budget_bytes)
        g = RxGatherC()
        _check(self._L.pptk_rx_gather_alloc(self._ctx, ctypes.byref(b), ctypes.byref(spec),
                                            ctypes.byref(g), _stream(stream, frames.device)),
               "pptk_rx_gather_alloc")
        return DeviceGather(self, g)

    def tuned_variant(self, frames, n, off=None, lens=None, stride=0, fixed_len=0, max_len=0,
                      compact=False):
        """Name of the variant a device batch of this shape launches now
        (runs one batch of it: the variant is reported by the library)."""
        self.batch_device(frames, n, off=off, lens=lens, stride=stride, fixed_len=fixed_len,
                          max_len=max_len, compact=compact)
        _torch().cuda.synchronize(frames.device)
        return VARIANTS[self._L.pptk_rx_last_variant(self._ctx)]

    def batch_device_mixed(self, frames, n, off, lens, recs=None, hash_out=None, max_len=0,
                           perm=None, scratch=None, stream=None, frag_out=None):
        """Mixed-size batch (pptk_rx_batch_device_mixed, asynchronous): batch
        order, or device binning + one launch per length group when the batch
        mixes jumbo frames with shorter ones.  perm: optional device buffer
        that receives the processing order; scratch: optional preallocated."""
        recs = _empty(recs, (n, 64), "uint8", frames.device)
        if scratch is None:
            scratch = _empty(None, self._L.pptk_rx_bin_scratch_bytes(n), "uint8", frames.device)
        b = _dev_batch(frames, n, off, lens, max_len=max_len, recs=recs, hash_out=hash_out,
                       frag_out=frag_out)
        _check(self._L.pptk_rx_batch_device_mixed(self._ctx, ctypes.byref(b), _dp(perm),
                                                  _dp(scratch), _stream(stream, frames.device)),
               "pptk_rx_batch_device_mixed")
        return recs

    def permit_device(self, recs, family, tokens, subject=None, compact=False, verdict=None,
                      scratch=None, stream=None):
        """Batched ip(v6)_permitted over device records (torch uint8 (n, 64)
        or (n, 32) with compact); tokens: torch int32 (iphash_size) updated
        in place; returns the uint8 verdicts (1 permit, 0 deny, 2 n/a)."""
        n = recs.shape[0]
        verdict = _empty(verdict, n, "uint8", recs.device)
        if scratch is None:
            scratch = _empty(None, self._L.pptk_rx_permit_scratch_bytes(n, tokens.numel()),
                             "uint8", recs.device)
        _check(self._L.pptk_rx_permit_device(self._ctx, None if compact else _dp(recs),
                                             _dp(recs) if compact else None, n, family,
                                             _dp(subject), _dp(tokens), _dp(verdict),
                                             _dp(scratch), _stream(stream, recs.device)),
               "pptk_rx_permit_device")
        return verdict

    def permit_keys_device(self, keys, family, tokens, subject=None, verdict=None, scratch=None,
                           stream=None):
        """pptk_rx_permit_keys_device: the rate limiter from the dense keys
        (torch int32 (n,)) a batch wrote through key_out."""
        n = keys.numel()
        verdict = _empty(verdict, n, "uint8", keys.device)
        if scratch is None:
            scratch = _empty(None, self._L.pptk_rx_permit_scratch_bytes(n, tokens.numel()),
                             "uint8", keys.device)
        _check(self._L.pptk_rx_permit_keys_device(self._ctx, _dp(keys), n, family, _dp(subject),
                                                  _dp(tokens), _dp(verdict), _dp(scratch),
                                                  _stream(stream, keys.device)),
               "pptk_rx_permit_keys_device")
        return verdict

    def permit_status(self, scratch, stream=None):
        """pptk_rx_permit_status: 0, or -ETIMEDOUT if a permit_keys_device
        call on `scratch` since the last query aborted (synchronises the
        stream)."""
        return self._L.pptk_rx_permit_status(self._ctx, _dp(scratch),
                                             _stream(stream, scratch.device))

    def tokens_refill_device(self, tokens, start, end, add, initial, stream=None):
        _check(self._L.pptk_rx_tokens_refill_device(self._ctx, _dp(tokens), start, end, add,
                                                    initial, _stream(stream, tokens.device)),
               "pptk_rx_tokens_refill_device")

    def tx_cksum_device(self, frames, n, off=None, lens=None, stride=0, fixed_len=0, max_len=0,
                        stream=None):
        """Tx side: set the checksums of the frames in `frames` (torch uint8
        CUDA tensor) in place, asynchronously."""
        _check(self._L.pptk_tx_cksum_device(self._ctx, _dp(frames), _dp(off), _dp(lens), stride,
                                            fixed_len, n, max_len,
                                            _stream(stream, frames.device)),
               "pptk_tx_cksum_device")

    def tx_set_side_buffer(self, buf):
        """pptk_tx_set_side_buffer: `buf` (a CUDA tensor of >= 8 bytes per
        frame, kept alive by the caller) as the two-pass tx side array, or
        None for the context's own."""
        nbytes = 0 if buf is None else buf.numel() * buf.element_size()
        _check(self._L.pptk_tx_set_side_buffer(self._ctx, _dp(buf), nbytes // 8),
               "pptk_tx_set_side_buffer")
        self._tx_side = buf

    def tx_rewrite_device(self, frames, n, rw, off=None, lens=None, stride=0, fixed_len=0,
                          status=None, stream=None):
        """Header rewrite with incremental checksum updates, in place and
        asynchronously.  rw: torch uint8 CUDA tensor of 1 or n struct
        pptk_rewrite entries (16 bytes each, records.REWRITE_DTYPE);
        status: optional torch uint8 CUDA tensor of n PPTK_RW_ST_* bytes."""
        count = rw.numel() // 16
        _check(self._L.pptk_tx_rewrite_device(self._ctx, _dp(frames), _dp(off), _dp(lens), stride,
                                              fixed_len, n, _dp(rw), count, _dp(status),
                                              _stream(stream, frames.device)),
               "pptk_tx_rewrite_device")

    def tx_rewrite_flow_device(self, frames, n, rw, idx=None, off=None, lens=None, stride=0,
                               fixed_len=0, status=None, stream=None):
        """pptk_tx_rewrite_flow_device: tx_rewrite_device with rw a table of
        struct pptk_rewrite entries indexed by idx (torch int32 CUDA tensor of
        n entries, the idx of flow_lookup_device; an index at or past the
        table, -1 = FLOW_NONE among them, leaves the frame alone with status
        records.RW_ST_NOFLOW).  idx=None is tx_rewrite_device itself."""
        count = rw.numel() * rw.element_size() // 16
        _check(self._L.pptk_tx_rewrite_flow_device(self._ctx, _dp(frames), _dp(off), _dp(lens),
                                                   stride, fixed_len, n, _dp(rw), count,
                                                   _dp(idx), _dp(status),
                                                   _stream(stream, frames.device)),
               "pptk_tx_rewrite_flow_device")

    def mss_clamp_device(self, frames, n, mss, syn_only=False, off=None, lens=None, stride=0,
                         fixed_len=0, status=None, stream=None):
        """TCP MSS clamping with incremental checksum update, in place and
        asynchronously; status: optional torch uint8 CUDA tensor of n
        PPTK_MSS_ST_* bytes."""
        _check(self._L.pptk_tcp_mss_clamp_device(self._ctx, _dp(frames), _dp(off), _dp(lens),
                                                 stride, fixed_len, n, mss,
                                                 1 if syn_only else 0, _dp(status),
                                                 _stream(stream, frames.device)),
               "pptk_tcp_mss_clamp_device")

    def seq_translate_device(self, frames, n, xl, idx=None, off=None, lens=None, stride=0,
                             fixed_len=0, status=None, stream=None):
        """TCP sequence-space translation (pptk_tcp_seq_translate_device), in
        place and asynchronously.  xl: torch uint8 CUDA tensor of struct
        pptk_seqxlate entries (24 bytes each, records.seqxlate_dtype): 1 or n
        of them, or a flow table indexed by idx (torch int32 CUDA tensor of n
        entries, -1 = 0xffffffff = no flow); status: optional torch uint8
        CUDA tensor of n PPTK_SEQ_ST_* bytes."""
        count = xl.numel() * xl.element_size() // 24
        _check(self._L.pptk_tcp_seq_translate_device(self._ctx, _dp(frames), _dp(off), _dp(lens),
                                                     stride, fixed_len, n, _dp(xl), count,
                                                     _dp(idx), _dp(status),
                                                     _stream(stream, frames.device)),
               "pptk_tcp_seq_translate_device")

    def ip_fragment_device(self, frames, n, mtu, out_cap, off=None, lens=None, stride=0,
                           fixed_len=0, out=None, out_stride=0, out_len=None, out_src=None,
                           first=None, count=None, status=None, totals=None, scratch=None,
                           stream=None):
        """IPv4 fragmentation to `mtu` (pptk_ip_fragment_device), asynchronous.
        Allocates what is not given -- out ((out_cap, out_stride) uint8,
        out_stride = round_up(18 + mtu, 16) unless given), out_len (int16),
        out_src / first / count (int32), status (uint8), totals (2 x int64),
        scratch -- and returns them as a dict.  Rows [0, totals[1]) of out
        hold the fragments; the views are the C arrays' bits (out_len is
        uint16 in C)."""
        dev = frames.device
        out_stride = out_stride or (18 + mtu + 15) & ~15
        out = _empty(out, (out_cap, out_stride), "uint8", dev)
        out_len = _empty(out_len, out_cap, "int16", dev)
        out_src = _empty(out_src, out_cap, "int32", dev)
        first = _empty(first, n, "int32", dev)
        count = _empty(count, n, "int32", dev)
        status = _empty(status, n, "uint8", dev)
        totals = _empty(totals, 2, "int64", dev)
        if scratch is None:
            scratch = _empty(None, self._L.pptk_ip_fragment_scratch_bytes(n), "uint8", dev)
        _check(self._L.pptk_ip_fragment_device(self._ctx, _dp(frames), _dp(off), _dp(lens),
                                               stride, fixed_len, n, mtu, _dp(out), out_stride,
                                               out_cap, _dp(out_len), _dp(out_src), _dp(first),
                                               _dp(count), _dp(status), _dp(totals),
                                               _dp(scratch), _stream(stream, dev)),
               "pptk_ip_fragment_device")
        return dict(out=out, out_stride=out_stride, out_len=out_len, out_src=out_src, first=first,
                    count=count, status=status, totals=totals, scratch=scratch)

    def ip_reass_device(self, frames, n, recs, frag, max_candidates, out_cap, out_stride,
                        report_cap=None, off=None, lens=None, stride=0, fixed_len=0, out=None,
                        out_len=None, report=None, dgram=None, fstatus=None, hdr=None,
                        scratch=None, stream=None):
        """Batch-local IPv4 reassembly (pptk_ip_reass_device), asynchronous.
        recs / frag: the uint8 CUDA tensors of 64-byte records and 16-byte
        fragment side records batch_device wrote for the same frames.
        Allocates what is not given -- out ((out_cap, out_stride) uint8),
        out_len (int16, the C array's uint16 bits), report (uint8, report_cap
        entries of records.REASS_DGRAM_DTYPE; report_cap = n unless given),
        dgram (int32, n), fstatus (uint8, n), hdr (int64, the six words of
        records.REASS_HDR_DTYPE) and the scratch -- and returns them as a
        dict.  Download hdr, then hdr.written slots and hdr.reported
        entries."""
        dev = frames.device
        report_cap = n if report_cap is None else report_cap
        out = _empty(out, (max(out_cap, 1), out_stride), "uint8", dev)
        out_len = _empty(out_len, max(out_cap, 1), "int16", dev)
        report = _empty(report, max(report_cap, 1) * 16, "uint8", dev)
        dgram = _empty(dgram, max(n, 1), "int32", dev)
        fstatus = _empty(fstatus, max(n, 1), "uint8", dev)
        hdr = _empty(hdr, 6, "int64", dev)
        need = self._L.pptk_ip_reass_scratch_bytes(n, max_candidates)
        scratch = _empty(scratch, max(need, 256), "uint8", dev)
        _check(self._L.pptk_ip_reass_device(self._ctx, _dp(frames), _dp(off), _dp(lens), stride,
                                            fixed_len, n, _dp(recs), _dp(frag), max_candidates,
                                            _dp(out), out_stride, out_cap, _dp(out_len),
                                            _dp(report), report_cap, _dp(dgram), _dp(fstatus),
                                            _dp(hdr), _dp(scratch),
                                            scratch.numel() * scratch.element_size(),
                                            _stream(stream, dev)), "pptk_ip_reass_device")
        return dict(out=out, out_stride=out_stride, out_len=out_len, report=report, dgram=dgram,
                    fstatus=fstatus, hdr=hdr, scratch=scratch)

    def ip_reass_host(self, *args, **kw):
        """pptk_ip_reass_host (the module's ip_reass_host) with this context's library."""
        return ip_reass_host(*args, lib_path=self._L._name, **kw)

    def ip_reass_scratch_bytes(self, n, max_candidates):
        return self._L.pptk_ip_reass_scratch_bytes(n, max_candidates)

    def ip_reass_shape(self):
        return ip_reass_shape(lib_path=self._L._name)

    def tunnel_encap_device(self, frames, n, tun, idx=None, id_base=0, off=None, lens=None,
                            stride=0, fixed_len=0, out=None, out_stride=0, out_len=None,
                            status=None, stream=None):
        """GRE encapsulation (pptk_tunnel_encap_device), asynchronous: slot i
        = 38-byte outer header + frame i.  tun: struct pptk_tunnel entries
        (records.TUNNEL_DTYPE) -- 1 or n of them, or a table indexed by idx
        (torch int32 CUDA tensor of n entries, -1 = 0xffffffff = no tunnel)
        -- as a NumPy array, which is checked (EINVAL for a non-zero
        `reserved` or an unknown flag bit) and uploaded, or as a torch CUDA
        tensor, which is passed as it is.  Allocates what is not given -- out
        ((n, out_stride) uint8; out_stride = round_up(38 + fixed_len, 16)
        unless given, and required with lens), out_len (int16), status (uint8) --
        and returns them as a dict; out_len holds the C array's uint16 bits."""
        from .records import TUN_DF, TUN_HDR_LEN, TUN_ID_SEQ, TUNNEL_DTYPE
        dev = frames.device
        if isinstance(tun, np.ndarray):
            t = np.ascontiguousarray(tun, dtype=TUNNEL_DTYPE).reshape(-1)
            if np.any(t["reserved"]) or np.any(t["flags"] & ~np.uint32(TUN_DF | TUN_ID_SEQ)):
                raise OSError(22, "struct pptk_tunnel: reserved must be 0, flags DF | ID_SEQ")
            tun = _torch().from_numpy(t.view(np.uint8).copy()).to(dev)
        count = tun.numel() * tun.element_size() // 32
        if not out_stride:
            if lens is not None:   # (the lengths are device data: n x 64 KB would be the only safe guess)
                raise ValueError("tunnel_encap_device: out_stride is required with lens")
            out_stride = (TUN_HDR_LEN + fixed_len + 15) & ~15
        out = _empty(out, (n, out_stride), "uint8", dev)
        out_len = _empty(out_len, n, "int16", dev)
        status = _empty(status, n, "uint8", dev)
        _check(self._L.pptk_tunnel_encap_device(self._ctx, _dp(frames), _dp(off), _dp(lens),
                                                stride, fixed_len, n, _dp(tun), count, _dp(idx),
                                                id_base, _dp(out), out_stride, _dp(out_len),
                                                _dp(status), _stream(stream, dev)),
               "pptk_tunnel_encap_device")
        return dict(out=out, out_stride=out_stride, out_len=out_len, status=status, tun=tun)

    def tunnel_decap_device(self, frames, n, off=None, lens=None, stride=0, fixed_len=0,
                            in_off=None, in_len=None, status=None, stream=None):
        """GRE decapsulation (pptk_tunnel_decap_device), asynchronous and
        zero-copy: descriptors of the inner frames inside `frames`.
        Allocates what is not given -- in_off (int64), in_len (int16), status
        (uint8) -- and returns them as a dict; in_off / in_len go into
        batch_device as off / lens."""
        dev = frames.device
        in_off = _empty(in_off, n, "int64", dev)
        in_len = _empty(in_len, n, "int16", dev)
        status = _empty(status, n, "uint8", dev)
        _check(self._L.pptk_tunnel_decap_device(self._ctx, _dp(frames), _dp(off), _dp(lens),
                                                stride, fixed_len, n, _dp(in_off), _dp(in_len),
                                                _dp(status), _stream(stream, dev)),
               "pptk_tunnel_decap_device")
        return dict(in_off=in_off, in_len=in_len, status=status)

    def flow_table(self, slots):
        """A flow table of `slots` slots mirrored on this context's device."""
        return FlowTable(slots, ctx=self)

    def flow_lookup_device(self, table, recs, subject=None, idx=None, status=None, stream=None):
        """pptk_flow_lookup_device, asynchronous: recs is the uint8 CUDA
        tensor of n 64-byte records batch_device returned, table a synced
        FlowTable of this context; subject: optional uint8 CUDA tensor of n
        entries.  Allocates what is not given and returns (idx, status): idx
        int32 (the C array's uint32 bits, -1 = FLOW_NONE = no flow), ready to
        be the idx= of seq_translate_device / tunnel_encap_device; status
        uint8 FLOW_ST_* bits."""
        dev = recs.device
        n = recs.numel() * recs.element_size() // 64
        idx = _empty(idx, n, "int32", dev)
        status = _empty(status, n, "uint8", dev)
        _check(self._L.pptk_flow_lookup_device(self._ctx, table._t, _dp(recs), n, _dp(subject),
                                               _dp(idx), _dp(status), _stream(stream, dev)),
               "pptk_flow_lookup_device")
        return idx, status

    def flow_account_device(self, idx, stats, now, lens=None, fixed_len=0, unmatched=None,
                            n=None, stream=None):
        """pptk_flow_account_device, asynchronous: adds the n frames of idx
        (torch int32 CUDA tensor, the idx of flow_lookup_device) to stats, a
        CUDA tensor of struct pptk_flow_stats entries (32 bytes each,
        records.FLOW_STATS_DTYPE; entry v belongs to flow value v), with
        their lengths lens (int16 CUDA tensor, the C array's uint16 bits) or
        fixed_len, and stamps the entries with `now`.  Frames whose index is
        at or past the array go to unmatched (one entry, optional).  The
        tensors accumulate: the caller zeroes them once."""
        n = idx.numel() if n is None else n
        count = stats.numel() * stats.element_size() // 32
        _check(self._L.pptk_flow_account_device(self._ctx, _dp(idx), _dp(lens), fixed_len, n,
                                                _dp(stats), count, _dp(unmatched), now,
                                                _stream(stream, stats.device)),
               "pptk_flow_account_device")

    def flow_stats_reset_device(self, stats, values, now, stream=None):
        """pptk_flow_stats_reset_device, asynchronous: stats[v] = {0, 0, now}
        for every v of values (torch int32 CUDA tensor) inside the array."""
        count = stats.numel() * stats.element_size() // 32
        _check(self._L.pptk_flow_stats_reset_device(self._ctx, _dp(stats), count, _dp(values),
                                                    values.numel(), now,
                                                    _stream(stream, stats.device)),
               "pptk_flow_stats_reset_device")

    def flow_learn_device(self, recs, status, max_candidates, cap, new_recs=None, first=None,
                          packets=None, hdr=None, scratch=None, n=None, stream=None):
        """pptk_flow_learn_device, asynchronous: the report of the new flows
        among the n frames of recs (the uint8 CUDA tensor of 64-byte records)
        by status (uint8 CUDA tensor, the status of flow_lookup_device).
        Allocates what is not given -- new_recs (uint8, cap * 64 bytes), first
        and packets (int32, cap entries; pass False for a null pointer), hdr
        (int64, the four words of records.FLOW_LEARN_HDR_DTYPE) and the
        scratch (uint8, flow_learn_scratch_bytes(n, max_candidates)) -- and
        returns dict(hdr, new_recs, first, packets, scratch).  Download hdr,
        then the first hdr.written entries of the arrays."""
        dev = recs.device
        n = recs.numel() * recs.element_size() // 64 if n is None else n
        if cap:
            new_recs = _empty(new_recs, cap * 64, "uint8", dev)
        first = None if first is False else _empty(first, max(cap, 1), "int32", dev)
        packets = None if packets is False else _empty(packets, max(cap, 1), "int32", dev)
        hdr = _empty(hdr, 4, "int64", dev)
        need = self._L.pptk_flow_learn_scratch_bytes(n, max_candidates)
        scratch = _empty(scratch, max(need, 256), "uint8", dev)
        _check(self._L.pptk_flow_learn_device(self._ctx, _dp(recs), _dp(status), n,
                                              max_candidates, _dp(new_recs), _dp(first),
                                              _dp(packets), cap, _dp(hdr), _dp(scratch),
                                              scratch.numel() * scratch.element_size(),
                                              _stream(stream, dev)), "pptk_flow_learn_device")
        return dict(hdr=hdr, new_recs=new_recs, first=first, packets=packets, scratch=scratch)

    def tx_dispatch_device(self, n, nports, port=None, idx=None, flow_port=None, miss_code=None,
                           subject=None, in_port=None, in_port_all=None, off=None, lens=None,
                           stride=0, fixed_len=0, cap=None, out_list=None, out_off=None,
                           out_len=None, ports=None, hdr=None, scratch=None, stream=None):
        """pptk_tx_dispatch_device, asynchronous: the per-port tx lists of n
        frames by their code -- port (uint8 CUDA tensor), or idx (int32, the
        index of flow_lookup_device) with flow_port (uint8, one code per flow
        value) and miss_code (default records.PORT_DROP).  subject and in_port
        are uint8 tensors or None; in_port_all defaults to "none".  Allocates
        what is not given -- out_list (int32), out_off (int64) and out_len
        (int16) of cap entries (cap defaults to n; pass False for a null
        out_off / out_len), ports (int64, 4 words per port:
        records.DISPATCH_PORT_DTYPE), hdr (int64, records.DISPATCH_HDR_DTYPE)
        and the scratch (uint8, tx_dispatch_scratch_bytes(n, nports)) -- and
        returns dict(hdr, ports, list, out_off, out_len, scratch).  Download
        ports, then each port's entries [start, start + count) below
        hdr.written."""
        from .records import PORT_DROP, PORT_MAX
        dev = (port if port is not None else idx).device
        cap = n if cap is None else cap
        if cap:
            out_list = _empty(out_list, cap, "int32", dev)
        out_off = None if out_off is False else _empty(out_off, max(cap, 1), "int64", dev)
        out_len = None if out_len is False else _empty(out_len, max(cap, 1), "int16", dev)
        ports = _empty(ports, 4 * nports, "int64", dev)
        hdr = _empty(hdr, 8, "int64", dev)
        need = self._L.pptk_tx_dispatch_scratch_bytes(n, nports)
        scratch = _empty(scratch, max(need, 256), "uint8", dev)
        d = Dispatch(n=n, port=_ptr(port), idx=_ptr(idx), flow_port=_ptr(flow_port),
                     flows=0 if flow_port is None else flow_port.numel(), subject=_ptr(subject),
                     in_port=_ptr(in_port),
                     in_port_all=PORT_MAX if in_port_all is None else in_port_all, nports=nports,
                     miss_code=PORT_DROP if miss_code is None else miss_code, off=_ptr(off),
                     len=_ptr(lens), stride=stride, fixed_len=fixed_len, list=_ptr(out_list),
                     out_off=_ptr(out_off), out_len=_ptr(out_len), cap=cap, ports=_ptr(ports),
                     hdr=_ptr(hdr))
        _check(self._L.pptk_tx_dispatch_device(self._ctx, ctypes.byref(d), _dp(scratch),
                                               scratch.numel() * scratch.element_size(),
                                               _stream(stream, dev)), "pptk_tx_dispatch_device")
        return dict(hdr=hdr, ports=ports, list=out_list, out_off=out_off, out_len=out_len,
                    scratch=scratch)

    def tx_gather_device(self, frames, n, max_entries, out_cap, nports=1, off=None, lens=None,
                         stride=0, fixed_len=0, entries=None, d_entries=None, runs=None,
                         out=None, pk_off=None, pk_len=None, ports=None, hdr=None, scratch=None,
                         stream=None):
        """pptk_tx_gather_device, asynchronous: the frames that the max_entries
        entries of `entries` (int32 CUDA tensor, the list of tx_dispatch_device;
        None: entry g is frame g) name, packed into one 256-byte aligned
        region of `out` per port, every frame in a slot of whole 16-byte
        chunks.  frames / off / lens / stride / fixed_len describe the n
        source frames as for every batch op.  runs is the ports tensor of
        tx_dispatch_device (None with nports 1: one region), d_entries a
        device word that cuts max_entries (an int64 tensor, or an address
        such as that of the dispatch header's `written`).  Allocates what is
        not given -- out (uint8, out_cap bytes; none for out_cap 0), pk_off
        (int64) and pk_len (int16) of max_entries entries (pass False for a
        null pointer), ports (int64, 4 words per port:
        records.GATHER_PORT_DTYPE), hdr (int64, records.GATHER_HDR_DTYPE) and
        the scratch (uint8, tx_gather_scratch_bytes(max_entries, nports)) --
        and returns dict(hdr, ports, out, pk_off, pk_len, scratch).  Download
        ports, then each port's out[start, start + bytes)."""
        dev = frames.device
        if out_cap:
            out = _empty(out, out_cap, "uint8", dev)
        pk_off = None if pk_off is False else _empty(pk_off, max(max_entries, 1), "int64", dev)
        pk_len = None if pk_len is False else _empty(pk_len, max(max_entries, 1), "int16", dev)
        ports = _empty(ports, 4 * nports, "int64", dev)
        hdr = _empty(hdr, 8, "int64", dev)
        need = self._L.pptk_tx_gather_scratch_bytes(max_entries, nports)
        scratch = _empty(scratch, max(need, 256), "uint8", dev)
        g = Gather(frames=_ptr(frames), off=_ptr(off), len=_ptr(lens), stride=stride,
                   fixed_len=fixed_len, n=n, list=_ptr(entries), max_entries=max_entries,
                   d_entries=d_entries if isinstance(d_entries, int) else _ptr(d_entries),
                   runs=_ptr(runs), nports=nports, out=_ptr(out) if out_cap else None,
                   out_cap=out_cap, pk_off=_ptr(pk_off), pk_len=_ptr(pk_len), ports=_ptr(ports),
                   hdr=_ptr(hdr))
        _check(self._L.pptk_tx_gather_device(self._ctx, ctypes.byref(g), _dp(scratch),
                                             scratch.numel() * scratch.element_size(),
                                             _stream(stream, dev)), "pptk_tx_gather_device")
        return dict(hdr=hdr, ports=ports, out=out, pk_off=pk_off, pk_len=pk_len, scratch=scratch)

    @staticmethod
    def tx_gather_host(*args, **kw):
        """pptk_tx_gather_host (the module's tx_gather_host)."""
        return tx_gather_host(*args, **kw)

    @staticmethod
    def tx_gather_scratch_bytes(max_entries, nports):
        """pptk_tx_gather_scratch_bytes (the module's tx_gather_scratch_bytes)."""
        return tx_gather_scratch_bytes(max_entries, nports)

    @staticmethod
    def tx_gather_shape():
        """pptk_tx_gather_shape (the module's tx_gather_shape)."""
        return tx_gather_shape()

    # ---- multi-GPU (RCCL) -------------------------------------------------
    def comm_create(self, nranks, rank, uid):
        """Join communicator `uid` (bytes from comm_uid()) as rank/nranks."""
        _check(self._L.pptk_rx_comm_create(self._ctx, nranks, rank, bytes(uid)),
               f"pptk_rx_comm_create({nranks}, {rank})")

    def comm_destroy(self):
        _check(self._L.pptk_rx_comm_destroy(self._ctx), "pptk_rx_comm_destroy")

    def comm_abort(self):
        """pptk_rx_comm_abort: cancel the communicator (any thread)."""
        _check(self._L.pptk_rx_comm_abort(self._ctx), "pptk_rx_comm_abort")

    def comm_sync(self, stream=None, timeout_ms=0):
        """pptk_rx_comm_sync: bounded wait for `stream` (torch stream, None =
        current) with RCCL error checks; returns 0 or the negative errno
        (-ETIMEDOUT / -EIO / -ECANCELED: the communicator is then dead)."""
        return self._L.pptk_rx_comm_sync(self._ctx, _stream(stream, self.device), timeout_ms)

    def comm_info(self):
        """(nranks, rank) of the context's communicator, or None."""
        nr, r = ctypes.c_int(), ctypes.c_int()
        rc = self._L.pptk_rx_comm_info(self._ctx, ctypes.byref(nr), ctypes.byref(r))
        return None if rc != 0 else (nr.value, r.value)

    def allgather_hash(self, d_hash, n, d_out, stream=None):
        """pptk_rx_allgather_hash: n u64 per rank from d_hash into d_out
        (torch int64 CUDA tensors), asynchronous on `stream`."""
        _check(self._L.pptk_rx_allgather_hash(self._ctx, _dp(d_hash), n, _dp(d_out),
                                              _stream(stream, d_out.device)),
               "pptk_rx_allgather_hash")

    def stream_split(self, coll_cus):
        """pptk_rx_stream_split: (rx stream, collective stream) as torch
        streams on this context's device, the collective's holding coll_cus
        CUs (a multiple of 32 on an MI355X) and the batches' the rest; the
        context sizes its grids for the rest until stream_join().  Call it
        before creating the communicator (its channel cap follows coll_cus).
        The HIP streams belong to the context and are destroyed with it."""
        torch = _torch()
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        _check(self._L.pptk_rx_stream_split(self._ctx, coll_cus, ctypes.byref(a),
                                            ctypes.byref(b)), f"pptk_rx_stream_split({coll_cus})")
        dev = torch.device("cuda", self.device)
        return (torch.cuda.ExternalStream(a.value, device=dev),
                torch.cuda.ExternalStream(b.value, device=dev))

    def stream_join(self):
        """Undo stream_split: the whole chip for this context's grids again
        (the split's streams stay the context's until close())."""
        self._L.pptk_rx_stream_split(self._ctx, 0, None, None)

    def bin_device(self, lens, n, stream=None):
        """Stable permutation of 0..n-1 by length class (torch uint32 tensor)."""
        perm = _empty(None, n, "int32", lens.device)
        scratch = _empty(None, self._L.pptk_rx_bin_scratch_bytes(n), "uint8", lens.device)
        _check(self._L.pptk_rx_bin_device(self._ctx, _dp(lens), n, _dp(perm), _dp(scratch),
                                          _stream(stream, lens.device)), "pptk_rx_bin_device")
        return perm

    def register_ring(self, buf):
        """Register numpy buffer `buf` as a zero-copy rx ring."""
        _check(self._L.pptk_rx_register_ring(self._ctx, ctypes.c_void_p(buf.ctypes.data),
                                             buf.nbytes), "pptk_rx_register_ring")

    def unregister_ring(self, buf):
        _check(self._L.pptk_rx_unregister_ring(self._ctx, ctypes.c_void_p(buf.ctypes.data)),
               "pptk_rx_unregister_ring")

    def batch_host(self, pkts, out=None, compact=False):
        """pptk_rx_batch (compact: pptk_rx_batch32, 32-byte records) over a
        ctypes array of LdpPacket; returns records (into `out`, a REC_DTYPE /
        REC32_DTYPE array of len(pkts), when given: an rx loop reuses its
        record array, so its pages are not faulted in per call)."""
        n = len(pkts)
        dt = REC32_DTYPE if compact else REC_DTYPE
        if out is not None:
            assert out.dtype == dt and out.shape == (n,) and out.flags["C_CONTIGUOUS"]
            recs = out
        else:
            recs = np.zeros(n, dtype=dt)
        fn = self._L.pptk_rx_batch32 if compact else self._L.pptk_rx_batch
        _check(fn(self._ctx, ctypes.cast(pkts, ctypes.c_void_p), n,
                  ctypes.c_void_p(recs.ctypes.data)), fn.__name__)
        return recs

    def submit_host(self, pkts, out):
        """pptk_rx_batch_submit (pptk_rx_batch_submit32 when `out` is a
        REC32_DTYPE array): enqueue one batch (len(pkts) <= max_batch);
        `pkts`, the frames they point at and `out` (len(pkts) records) must
        stay alive and untouched until complete_host() has returned this
        batch.  Raises OSError(EBUSY) with PPTK_RX_MAX_INFLIGHT batches
        outstanding."""
        n = len(pkts)
        compact = out.dtype == REC32_DTYPE
        assert (compact or out.dtype == REC_DTYPE) and out.shape == (n,) and out.flags["C_CONTIGUOUS"]
        fn = self._L.pptk_rx_batch_submit32 if compact else self._L.pptk_rx_batch_submit
        _check(fn(self._ctx, ctypes.cast(pkts, ctypes.c_void_p), n,
                  ctypes.c_void_p(out.ctypes.data)), fn.__name__)
        # the library holds pointers into both until the batch completes:
        # keep the Python objects alive until then (FIFO, as completions)
        self._inflight.append((pkts, out))

    def complete_host(self):
        """pptk_rx_batch_complete: wait for the oldest outstanding batch;
        returns its frame count."""
        n = _check(self._L.pptk_rx_batch_complete(self._ctx), "pptk_rx_batch_complete", True)
        self._inflight.popleft()
        return n

    def pending_host(self):
        return self._L.pptk_rx_batch_pending(self._ctx)


def _flow_key(key):
    """One struct pptk_flow_key as a 40-byte uint8 array, from a
    records.FLOW_KEY_DTYPE entry or its bytes."""
    return _one_struct(key, "key", "pptk_flow_key", 40)


def flow_key_hash(key16, key, lib_path=None):
    """pptk_flow_key_hash: the flow hash the receive transform gives the
    tuple `key` (a records.FLOW_KEY_DTYPE entry) under the SipHash key."""
    key16 = bytes(key16)
    if len(key16) != 16:
        raise ValueError("key16 must be 16 bytes")
    k = _flow_key(key)   # (kept alive across the call)
    return lib(lib_path).pptk_flow_key_hash(key16, k.ctypes.data)


def flow_key_from_rec(rec, lib_path=None):
    """pptk_flow_key_from_rec: the records.FLOW_KEY_DTYPE entry of one record
    (a records.REC_DTYPE entry or its 64 bytes)."""
    from .records import FLOW_KEY_DTYPE
    r = _one_struct(rec, "rec", "pptk_rx_rec", 64)
    k = np.full(1, 0xEE, np.uint8).repeat(40)
    lib(lib_path).pptk_flow_key_from_rec(r.ctypes.data, k.ctypes.data)
    return k.view(FLOW_KEY_DTYPE)[0]


class FlowTable:
    """One pptk_flow_table: FlowTable(slots) is host-only, RxContext.flow_table
    (slots) is mirrored on the context's device (sync, flow_lookup_device).
    Keys are records.FLOW_KEY_DTYPE entries (or their 40 bytes); the errno
    returns of the C calls are raised as OSError, except where a method's
    docstring says it returns them."""

    def __init__(self, slots, ctx=None, lib_path=None):
        self._L = L = ctx._L if ctx is not None else lib(lib_path)
        self._t = ctypes.c_void_p()
        self._ctx = ctx   # (keeps the context alive as long as the table)
        _check(L.pptk_flow_table_create(ctx._ctx if ctx is not None else None, slots,
                                        ctypes.byref(self._t)),
               f"pptk_flow_table_create({slots})")

    def close(self):
        if self._t:
            self._L.pptk_flow_table_destroy(self._t)
            self._t = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def insert_rc(self, key, flow_hash, value):
        """pptk_flow_table_insert's return code (0, -EEXIST, -ENOSPC, -EINVAL)."""
        k = _flow_key(key)   # (kept alive across the call)
        return self._L.pptk_flow_table_insert(self._t, k.ctypes.data, flow_hash, value)

    def update_rc(self, key, flow_hash, value):
        k = _flow_key(key)
        return self._L.pptk_flow_table_update(self._t, k.ctypes.data, flow_hash, value)

    def delete_rc(self, key, flow_hash):
        k = _flow_key(key)
        return self._L.pptk_flow_table_delete(self._t, k.ctypes.data, flow_hash)

    def insert(self, key, flow_hash, value):
        _check(self.insert_rc(key, flow_hash, value), "pptk_flow_table_insert")

    def update(self, key, flow_hash, value):
        _check(self.update_rc(key, flow_hash, value), "pptk_flow_table_update")

    def delete(self, key, flow_hash):
        _check(self.delete_rc(key, flow_hash), "pptk_flow_table_delete")

    def find(self, key, flow_hash):
        """The key's value, or None if it is absent."""
        v = ctypes.c_uint32(0)
        k = _flow_key(key)
        rc = self._L.pptk_flow_table_find(self._t, k.ctypes.data, flow_hash, ctypes.byref(v))
        if rc == -2:
            return None
        _check(rc, "pptk_flow_table_find")
        return v.value

    def insert_recs(self, recs, values):
        """pptk_flow_table_insert_recs over a NumPy array of records
        (records.REC_DTYPE, or its bytes): (number inserted, int32 results)."""
        r = np.ascontiguousarray(recs).view(np.uint8).reshape(-1)
        n = r.size // 64
        v = np.ascontiguousarray(values, dtype=np.uint32).reshape(-1)
        if r.size != n * 64 or v.size != n:
            raise ValueError("insert_recs: n 64-byte records and n values")
        res = np.zeros(max(n, 1), np.int32)
        rc = _check(self._L.pptk_flow_table_insert_recs(self._t, r.ctypes.data, n, v.ctypes.data,
                                                        res.ctypes.data),
                    "pptk_flow_table_insert_recs", True)
        return rc, res[:n]

    def clear(self):
        self._L.pptk_flow_table_clear(self._t)

    def stats(self):
        """dict(slots, count, probe_limit)."""
        a, b, c = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        self._L.pptk_flow_table_stats(self._t, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        return dict(slots=a.value, count=b.value, probe_limit=c.value)

    def sync(self, stream=None):
        """pptk_flow_table_sync on `stream` (torch stream or None = current):
        the bytes it uploaded."""
        s = None if self._ctx is None else _stream(stream, self._ctx.device)
        up = ctypes.c_uint64(0)
        _check(self._L.pptk_flow_table_sync(self._t, s, ctypes.byref(up)),
               "pptk_flow_table_sync")
        return up.value

    def expire(self, stats, now, idle, cap=None):
        """pptk_flow_table_expire: deletes up to cap (default: all) flows whose
        value v lies inside stats -- a NumPy array of records.FLOW_STATS_DTYPE,
        the downloaded copy -- with stats[v].last_seen + idle < now, and
        returns their values (uint32).  Call again while it returns cap
        values; sync() uploads the change."""
        st = _flow_stats(stats)
        cap = self.stats()["count"] if cap is None else cap
        out = np.zeros(max(cap, 1), np.uint32)
        rc = _check(self._L.pptk_flow_table_expire(self._t, st.ctypes.data, st.size, now, idle,
                                                   out.ctypes.data, cap),
                    "pptk_flow_table_expire", True)
        return out[:rc]

    def lookup_host(self, recs, subject=None):
        """pptk_flow_lookup_host over a NumPy array of records: (idx uint32,
        status uint8)."""
        r = np.ascontiguousarray(recs).view(np.uint8).reshape(-1)
        n = r.size // 64
        idx = np.zeros(max(n, 1), np.uint32)
        st = np.zeros(max(n, 1), np.uint8)
        sub = None
        if subject is not None:
            sub = np.ascontiguousarray(subject, dtype=np.uint8).reshape(-1)
            if sub.size != n:
                raise ValueError("lookup_host: one subject byte per record")
        _check(self._L.pptk_flow_lookup_host(self._t, r.ctypes.data, n,
                                             None if sub is None else sub.ctypes.data,
                                             idx.ctypes.data, st.ctypes.data),
               "pptk_flow_lookup_host")
        return idx[:n], st[:n]


def _flow_stats(stats):
    """A NumPy array of records.FLOW_STATS_DTYPE as the C calls need it: a
    32-byte aligned one-dimensional array (the caller's own where it is one)."""
    from .records import FLOW_STATS_DTYPE
    if not (isinstance(stats, np.ndarray) and stats.dtype == FLOW_STATS_DTYPE and stats.ndim == 1
            and stats.flags.c_contiguous):
        raise ValueError("stats must be a 1-d contiguous array of records.FLOW_STATS_DTYPE")
    if stats.ctypes.data & 31:
        raise ValueError("stats must be 32-byte aligned (rx.flow_stats_array allocates one)")
    return stats


def flow_stats_array(count):
    """A zeroed, 32-byte aligned array of `count` records.FLOW_STATS_DTYPE entries."""
    from .records import FLOW_STATS_DTYPE
    raw = np.zeros(count * 32 + 32, np.uint8)
    skip = -raw.ctypes.data & 31
    return raw[skip:skip + count * 32].view(FLOW_STATS_DTYPE)


def flow_account_host(idx, stats, now, lens=None, fixed_len=0, unmatched=None, lib_path=None):
    """pptk_flow_account_host, the CPU statement of flow_account_device, in
    place: idx uint32, lens uint16 or None (then fixed_len), stats and
    unmatched (one entry, optional) aligned arrays of records.FLOW_STATS_DTYPE
    (flow_stats_array)."""
    i = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
    ln = None if lens is None else np.ascontiguousarray(lens, dtype=np.uint16).reshape(-1)
    if ln is not None and ln.size != i.size:
        raise ValueError("flow_account_host: one length per index")
    st = _flow_stats(stats)
    um = None if unmatched is None else _flow_stats(unmatched)
    _check(lib(lib_path).pptk_flow_account_host(
        i.ctypes.data, None if ln is None else ln.ctypes.data, fixed_len, i.size, st.ctypes.data,
        st.size, None if um is None else um.ctypes.data, now), "pptk_flow_account_host")


def flow_account_shape(lib_path=None):
    """pptk_flow_account_shape: (segment_frames, lds_slots) of the library's
    accounting kernel; lds_slots is 0 for a direct build."""
    s, k = ctypes.c_uint32(), ctypes.c_uint32()
    lib(lib_path).pptk_flow_account_shape(ctypes.byref(s), ctypes.byref(k))
    return s.value, k.value


def _aligned_bytes(nbytes, align=64):
    """A zeroed uint8 array of nbytes whose address is a multiple of align."""
    raw = np.zeros(nbytes + align, np.uint8)
    skip = -raw.ctypes.data & (align - 1)
    return raw[skip:skip + nbytes]


def flow_learn_host(recs, status, max_candidates, cap, lib_path=None):
    """pptk_flow_learn_host, the CPU statement of flow_learn_device: recs a
    NumPy array of records (records.REC_DTYPE, or its bytes), status the uint8
    array of the lookup.  Returns (hdr, new_recs, first, packets): hdr one
    records.FLOW_LEARN_HDR_DTYPE entry, the arrays cut to hdr.written entries
    (records.REC_DTYPE, uint32, uint32)."""
    from .records import FLOW_LEARN_HDR_DTYPE, REC_DTYPE
    r = np.ascontiguousarray(recs).view(np.uint8).reshape(-1)
    n = r.size // 64
    st = np.ascontiguousarray(status, dtype=np.uint8).reshape(-1)
    if r.size != n * 64 or st.size != n:
        raise ValueError("flow_learn_host: n 64-byte records and n status bytes")
    if r.ctypes.data & 15:
        a = _aligned_bytes(r.size)
        a[:] = r
        r = a
    out = _aligned_bytes(max(cap, 1) * 64)
    first = np.zeros(max(cap, 1), np.uint32)
    packets = np.zeros(max(cap, 1), np.uint32)
    hdr = np.zeros(1, FLOW_LEARN_HDR_DTYPE)
    _check(lib(lib_path).pptk_flow_learn_host(
        r.ctypes.data, st.ctypes.data, n, max_candidates, out.ctypes.data if cap else None,
        first.ctypes.data, packets.ctypes.data, cap, hdr.ctypes.data), "pptk_flow_learn_host")
    w = int(hdr["written"][0])
    return hdr[0], out[:w * 64].view(REC_DTYPE), first[:w], packets[:w]


def flow_learn_scratch_bytes(n, max_candidates, lib_path=None):
    """pptk_flow_learn_scratch_bytes: the device scratch a learn call over n
    frames with this max_candidates needs (0 for n = 0)."""
    return lib(lib_path).pptk_flow_learn_scratch_bytes(n, max_candidates)


def flow_learn_shape(lib_path=None):
    """pptk_flow_learn_shape: (block_frames, scan_width) of the library's
    learning kernels."""
    b, w = ctypes.c_uint32(), ctypes.c_uint32()
    lib(lib_path).pptk_flow_learn_shape(ctypes.byref(b), ctypes.byref(w))
    return b.value, w.value


def tx_dispatch_host(nports, port=None, idx=None, flow_port=None, miss_code=None, subject=None,
                     in_port=None, in_port_all=None, off=None, lens=None, stride=0, fixed_len=0,
                     cap=None, lib_path=None):
    """pptk_tx_dispatch_host, the CPU statement of tx_dispatch_device, over
    NumPy arrays: port (uint8) or idx (uint32) with flow_port (uint8) and
    miss_code (default records.PORT_DROP); subject, in_port (uint8), off
    (uint64) and lens (uint16) are arrays or None; cap defaults to n.  Returns
    (hdr, ports, list, out_off, out_len): hdr one records.DISPATCH_HDR_DTYPE
    entry, ports nports records.DISPATCH_PORT_DTYPE entries, the three arrays
    cut to hdr.written entries (uint32, uint64, uint16)."""
    from .records import DISPATCH_HDR_DTYPE, DISPATCH_PORT_DTYPE, PORT_DROP, PORT_MAX

    def arr(x, dtype):
        return None if x is None else np.ascontiguousarray(x, dtype=dtype).reshape(-1)

    port, idx, flow_port = arr(port, np.uint8), arr(idx, np.uint32), arr(flow_port, np.uint8)
    subject, in_port = arr(subject, np.uint8), arr(in_port, np.uint8)
    off, lens = arr(off, np.uint64), arr(lens, np.uint16)
    if (port is None) == (idx is None):
        raise ValueError("tx_dispatch_host: exactly one of port / idx")
    n = len(port if port is not None else idx)
    if any(x is not None and len(x) != n for x in (subject, in_port, off, lens)):
        raise ValueError("tx_dispatch_host: subject, in_port, off and lens have n entries")
    cap = n if cap is None else cap
    out = (np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint64),
           np.zeros(max(cap, 1), np.uint16))
    ports, hdr = np.zeros(max(nports, 1), DISPATCH_PORT_DTYPE), np.zeros(1, DISPATCH_HDR_DTYPE)

    def p(x):
        return None if x is None else x.ctypes.data

    d = Dispatch(n=n, port=p(port), idx=p(idx), flow_port=p(flow_port),
                 flows=0 if flow_port is None else len(flow_port), subject=p(subject),
                 in_port=p(in_port), in_port_all=PORT_MAX if in_port_all is None else in_port_all,
                 nports=nports, miss_code=PORT_DROP if miss_code is None else miss_code,
                 off=p(off), len=p(lens), stride=stride, fixed_len=fixed_len,
                 list=p(out[0]) if cap else None, out_off=p(out[1]), out_len=p(out[2]), cap=cap,
                 ports=p(ports), hdr=p(hdr))
    _check(lib(lib_path).pptk_tx_dispatch_host(ctypes.byref(d)), "pptk_tx_dispatch_host")
    w = int(hdr["written"][0])
    return hdr[0], ports[:nports], out[0][:w], out[1][:w], out[2][:w]


def tx_dispatch_scratch_bytes(n, nports, lib_path=None):
    """pptk_tx_dispatch_scratch_bytes: the device scratch a dispatch of n
    frames to nports ports needs (0 for n = 0)."""
    return lib(lib_path).pptk_tx_dispatch_scratch_bytes(n, nports)


def tx_dispatch_shape(lib_path=None):
    """pptk_tx_dispatch_shape: (block_frames, scan_width) of the library's
    dispatch kernels."""
    b, w = ctypes.c_uint32(), ctypes.c_uint32()
    lib(lib_path).pptk_tx_dispatch_shape(ctypes.byref(b), ctypes.byref(w))
    return b.value, w.value


def tx_gather_host(frames, n, out_cap, nports=1, off=None, lens=None, stride=0, fixed_len=0,
                   entries=None, max_entries=None, d_entries=None, runs=None, lib_path=None):
    """pptk_tx_gather_host, the CPU statement of tx_gather_device, over NumPy
    arrays: frames (uint8) with off (uint64) / lens (uint16) or stride /
    fixed_len, n frames; entries (uint32) or None (entry g is frame g,
    max_entries defaults to n); d_entries an int that cuts max_entries or
    None; runs nports records.DISPATCH_PORT_DTYPE entries or None.  Returns
    (hdr, ports, out, pk_off, pk_len): hdr one records.GATHER_HDR_DTYPE entry,
    ports nports records.GATHER_PORT_DTYPE entries, out the out_cap bytes
    (zero where the call wrote nothing), pk_off / pk_len cut to hdr.entries."""
    from .records import DISPATCH_PORT_DTYPE, GATHER_HDR_DTYPE, GATHER_PORT_DTYPE

    def arr(x, dtype):
        return None if x is None else np.ascontiguousarray(x, dtype=dtype).reshape(-1)

    frames, off, lens = arr(frames, np.uint8), arr(off, np.uint64), arr(lens, np.uint16)
    entries = arr(entries, np.uint32)
    if any(x is not None and len(x) != n for x in (off, lens)):
        raise ValueError("tx_gather_host: off and lens have n entries")
    if max_entries is None:
        max_entries = n if entries is None else len(entries)
    if entries is not None and len(entries) < max_entries:
        raise ValueError("tx_gather_host: entries has max_entries entries")
    if runs is not None:
        runs = np.ascontiguousarray(runs, dtype=DISPATCH_PORT_DTYPE).reshape(-1)
        if len(runs) != nports:
            raise ValueError("tx_gather_host: runs has nports entries")
    out = np.zeros(max(out_cap, 1) + 255, np.uint8)
    shift = -out.ctypes.data % 256
    pk_off, pk_len = np.zeros(max(max_entries, 1), np.uint64), np.zeros(max(max_entries, 1), np.uint16)
    ports, hdr = np.zeros(max(nports, 1), GATHER_PORT_DTYPE), np.zeros(1, GATHER_HDR_DTYPE)
    word = None if d_entries is None else np.array([d_entries], np.uint64)

    def p(x):
        return None if x is None else x.ctypes.data

    g = Gather(frames=p(frames), off=p(off), len=p(lens), stride=stride, fixed_len=fixed_len, n=n,
               list=p(entries), max_entries=max_entries, d_entries=p(word), runs=p(runs),
               nports=nports, out=out.ctypes.data + shift if out_cap else None, out_cap=out_cap,
               pk_off=p(pk_off), pk_len=p(pk_len), ports=p(ports), hdr=p(hdr))
    _check(lib(lib_path).pptk_tx_gather_host(ctypes.byref(g)), "pptk_tx_gather_host")
    e = int(hdr["entries"][0])
    return hdr[0], ports[:nports], out[shift:shift + out_cap], pk_off[:e], pk_len[:e]


def tx_gather_scratch_bytes(max_entries, nports, lib_path=None):
    """pptk_tx_gather_scratch_bytes: the device scratch a gather of up to
    max_entries entries into nports regions needs (0 for max_entries = 0)."""
    return lib(lib_path).pptk_tx_gather_scratch_bytes(max_entries, nports)


def tx_gather_shape(lib_path=None):
    """pptk_tx_gather_shape: (block_entries, scan_width) of the library's
    gather kernels."""
    b, w = ctypes.c_uint32(), ctypes.c_uint32()
    lib(lib_path).pptk_tx_gather_shape(ctypes.byref(b), ctypes.byref(w))
    return b.value, w.value


def ip_fragment_host(frame, mtu, out_cap, out_stride=0, lib_path=None):
    """pptk_ip_fragment_host on one frame (bytes): (count, status, out,
    out_len) with out an (out_cap, out_stride) uint8 array pre-filled with
    0xEE whose rows [0, count) hold the fragments unless status has NOROOM."""
    out_stride = out_stride or (18 + mtu + 15) & ~15
    out = np.full((max(out_cap, 1), out_stride), 0xEE, np.uint8)
    out_len = np.zeros(max(out_cap, 1), np.uint16)
    status = ctypes.c_uint8(0)
    rc = _check(lib(lib_path).pptk_ip_fragment_host(
        bytes(frame), len(frame), mtu, out.ctypes.data, out_stride, out_cap, out_len.ctypes.data,
        ctypes.byref(status)), "pptk_ip_fragment_host", True)
    return rc, status.value, out[:out_cap], out_len[:out_cap]


def ip_reass_host(buf, recs, frag, max_candidates, out_cap, out_stride, report_cap=None, off=None,
                  lens=None, stride=0, fixed_len=0, n=None, fill=0xEE, lib_path=None):
    """pptk_ip_reass_host, the CPU statement of ip_reass_device, over NumPy
    arrays: buf the frame bytes, recs / frag the records (records.REC_DTYPE /
    FRAG_DTYPE or their bytes), off (uint64) / lens (uint16) or stride /
    fixed_len the layout.  Every output array is pre-filled with `fill` so a
    caller can see what was not touched.  Returns dict(hdr, out, out_len,
    report, dgram, fstatus): hdr one records.REASS_HDR_DTYPE entry, out
    (out_cap, out_stride) uint8, report report_cap REASS_DGRAM_DTYPE
    entries (report_cap = n unless given)."""
    from .records import REASS_DGRAM_DTYPE, REASS_HDR_DTYPE
    b = np.ascontiguousarray(buf, dtype=np.uint8)
    r = np.ascontiguousarray(recs).view(np.uint8).reshape(-1)
    f = np.ascontiguousarray(frag).view(np.uint8).reshape(-1)
    if n is None:
        n = r.size // 64
    if r.size < n * 64 or f.size < n * 16:
        raise ValueError("ip_reass_host: n 64-byte records and n 16-byte side records")
    report_cap = n if report_cap is None else report_cap
    o = None if off is None else np.ascontiguousarray(off, dtype=np.uint64)
    ln = None if lens is None else np.ascontiguousarray(lens, dtype=np.uint16)
    out = _aligned_bytes(max(out_cap, 1) * out_stride)
    out[:] = fill
    out_len = np.full(max(out_cap, 1), fill * 0x0101, np.uint16)
    report = np.full(max(report_cap, 1) * 16, fill, np.uint8)
    dgram = np.full(max(n, 1), fill * 0x01010101, np.uint32)
    fstatus = np.full(max(n, 1), fill, np.uint8)
    hdr = np.zeros(1, REASS_HDR_DTYPE)

    def p(a):
        return None if a is None else a.ctypes.data

    _check(lib(lib_path).pptk_ip_reass_host(
        p(b), p(o), p(ln), stride, fixed_len, n, p(r), p(f), max_candidates,
        p(out) if out_cap else None, out_stride, out_cap, p(out_len) if out_cap else None,
        p(report) if report_cap else None, report_cap, p(dgram), p(fstatus), p(hdr)),
        "pptk_ip_reass_host")
    return dict(hdr=hdr[0], out=out[:out_cap * out_stride].reshape(out_cap, out_stride),
                out_len=out_len[:out_cap], report=report[:report_cap * 16].view(REASS_DGRAM_DTYPE),
                dgram=dgram[:n], fstatus=fstatus[:n])


def ip_reass_scratch_bytes(n, max_candidates, lib_path=None):
    """pptk_ip_reass_scratch_bytes: the device scratch a reassembly call over
    n frames with this max_candidates needs (0 for n = 0)."""
    return lib(lib_path).pptk_ip_reass_scratch_bytes(n, max_candidates)


def ip_reass_shape(lib_path=None):
    """pptk_ip_reass_shape: (max_frags, block_frames) of the library's
    reassembly kernels."""
    m, b = ctypes.c_uint32(), ctypes.c_uint32()
    lib(lib_path).pptk_ip_reass_shape(ctypes.byref(m), ctypes.byref(b))
    return m.value, b.value


def tunnel_encap_host(frame, tun, seq=0, out_cap=None, lib_path=None):
    """pptk_tunnel_encap_host on one frame (bytes) with one struct
    pptk_tunnel (a records.TUNNEL_DTYPE entry or its 32 bytes): (status, out,
    out_len) with out an out_cap-byte uint8 array (round_up(38 + len, 16)
    unless given) pre-filled with 0xEE."""
    t = _one_struct(tun, "tun", "pptk_tunnel", 32)
    frame = bytes(frame)
    if out_cap is None:
        out_cap = (38 + len(frame) + 15) & ~15
    out = np.full(max(out_cap, 1), 0xEE, np.uint8)
    out_len = ctypes.c_uint16(0xEEEE)
    st = lib(lib_path).pptk_tunnel_encap_host(frame, len(frame), t.ctypes.data, seq,
                                              out.ctypes.data, out_cap, ctypes.byref(out_len))
    return st, out[:out_cap], out_len.value


def tunnel_decap_host(frame, lib_path=None):
    """pptk_tunnel_decap_host on one frame (bytes): (status, in_off, in_len),
    the inner frame being frame[in_off:in_off + in_len] when status has OK."""
    frame = bytes(frame)
    in_off, in_len = ctypes.c_uint32(0xEEEEEEEE), ctypes.c_uint16(0xEEEE)
    st = lib(lib_path).pptk_tunnel_decap_host(frame, len(frame), ctypes.byref(in_off),
                                              ctypes.byref(in_len))
    return st, in_off.value, in_len.value


def tcp_seq_translate_hdr(segment_bytes, xl, lib_path=None):
    """pptk_tcp_seq_translate_hdr on one TCP segment (bytes, the TCP header
    first) with the translation xl (one records.seqxlate_dtype entry, or its
    24 bytes): (status, the segment's bytes afterwards)."""
    x = _one_struct(xl, "xl", "pptk_seqxlate", 24)
    # a buffer of exactly len(segment) bytes (at least one, to have an address)
    seg = np.frombuffer(bytes(segment_bytes), np.uint8).copy()
    buf = seg if seg.size else np.zeros(1, np.uint8)
    st = lib(lib_path).pptk_tcp_seq_translate_hdr(buf.ctypes.data, seg.size, x.ctypes.data)
    return st, seg.tobytes()


def comm_uid(lib_path=None):
    """A new RCCL communicator id (128 bytes), made on one rank."""
    buf = ctypes.create_string_buffer(128)
    _check(lib(lib_path).pptk_rx_comm_uid(buf), "pptk_rx_comm_uid")
    return buf.raw


def comm_create_all(ctxs):
    """One communicator over the contexts (one per GPU) of this process."""
    arr = (ctypes.c_void_p * len(ctxs))(*[c._ctx.value for c in ctxs])
    _check(ctxs[0]._L.pptk_rx_comm_create_all(arr, len(ctxs)), "pptk_rx_comm_create_all")


def shard_range(n, nranks, rank, lib_path=None):
    """(first, count, per_rank) of the equal-shard policy (pptk_rx_shard_range)."""
    f, c, p = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    lib(lib_path).pptk_rx_shard_range(n, nranks, rank, ctypes.byref(f), ctypes.byref(c),
                                      ctypes.byref(p))
    return f.value, c.value, p.value


LDP_PACKET_DTYPE = np.dtype([("data", "<u8"), ("sz", "<u4"), ("pad", "<u4"),
                             ("ancillary64", "<u8")])


def ldp_packets(buf, off, lens):
    """Build an LdpPacket array pointing into numpy buffer `buf` (kept alive
    by the caller), as ldp_in_nextpkts() would hand out."""
    n = len(off)
    a = np.zeros(n, dtype=LDP_PACKET_DTYPE)
    a["data"] = buf.ctypes.data + np.asarray(off, dtype=np.uint64)
    a["sz"] = np.asarray(lens, dtype=np.uint32)
    a["ancillary64"] = np.arange(n, dtype=np.uint64)
    arr = (LdpPacket * n).from_buffer(a)
    arr._keep = a
    return arr
