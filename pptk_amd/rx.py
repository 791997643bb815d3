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
        import torch
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
        import torch
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


assert ctypes.sizeof(LdpPacket) == 24
assert ctypes.sizeof(RxOpts) == 40

EXPORTS = ("pptk_rx_opts_default", "pptk_rx_ctx_create", "pptk_rx_ctx_destroy",
           "pptk_rx_batch", "pptk_rx_batch32", "pptk_rx_batch_submit", "pptk_rx_batch_submit32",
           "pptk_rx_batch_complete",
           "pptk_rx_batch_pending", "pptk_rx_batch_device", "pptk_rx_bin_scratch_bytes",
           "pptk_rx_bin_device", "pptk_rx_batch_device_mixed", "pptk_rx_version", "pptk_rx_set_tuning",
           "pptk_rx_variant_count", "pptk_rx_last_variant", "pptk_rx_register_ring", "pptk_rx_unregister_ring",
           "pptk_rx_permit_scratch_bytes", "pptk_rx_permit_device", "pptk_rx_permit_keys_device",
           "pptk_rx_permit_status", "pptk_rx_tokens_refill_device", "pptk_tx_cksum_device", "pptk_tx_set_side_buffer",
           "pptk_tx_rewrite_device",
           "pptk_tcp_mss_clamp_device", "pptk_tcp_seq_translate_device",
           "pptk_tcp_seq_translate_hdr", "pptk_ip_fragment_scratch_bytes",
           "pptk_ip_fragment_device", "pptk_ip_fragment_host",
           "pptk_tunnel_encap_device", "pptk_tunnel_decap_device",
           "pptk_tunnel_encap_host", "pptk_tunnel_decap_host",
           "pptk_flow_table_create", "pptk_flow_table_destroy", "pptk_flow_key_from_rec",
           "pptk_flow_key_hash", "pptk_flow_table_insert", "pptk_flow_table_update",
           "pptk_flow_table_delete", "pptk_flow_table_find", "pptk_flow_table_insert_recs",
           "pptk_flow_table_clear", "pptk_flow_table_stats", "pptk_flow_table_sync",
           "pptk_flow_lookup_device", "pptk_flow_lookup_host",
           "pptk_flow_account_device", "pptk_flow_account_host", "pptk_flow_stats_reset_device",
           "pptk_flow_account_shape", "pptk_flow_table_expire", "pptk_tx_rewrite_flow_device",
           "pptk_flow_learn_scratch_bytes", "pptk_flow_learn_device", "pptk_flow_learn_host",
           "pptk_flow_learn_shape",
           "pptk_rx_autotune", "pptk_rx_place_records",
           "pptk_rx_place_buffers", "pptk_rx_ring_alloc", "pptk_rx_ring_free",
           "pptk_rx_gather_alloc", "pptk_rx_gather_free",
           # multi-GPU (RCCL)
           "pptk_rx_device_count", "pptk_rx_comm_uid", "pptk_rx_comm_create",
           "pptk_rx_comm_create_all", "pptk_rx_comm_destroy", "pptk_rx_comm_info",
           "pptk_rx_comm_abort", "pptk_rx_comm_sync",
           "pptk_rx_shard_range", "pptk_rx_allgather_hash", "pptk_rx_stream_split",
           "pptk_rx_stream_destroy", "pptk_rx_abi",
           # kept per-packet APIs (ipcksum.h, hashseed.h)
           "ip_cksum_feed", "ip_hdr_cksum_calc", "tcp_cksum_calc", "udp_cksum_calc",
           "tcp6_cksum_calc", "udp6_cksum_calc", "hash_seed_init",
           "tcp_parse_options", "tcp_find_sack_ts_headers", "tcp_find_sack_header")

# Kernel variants, in the order of enum RxVariant (pptk_amd/csrc/rx_internal.h).
VARIANTS = ("T4S1", "T4S2", "T16S2", "T16S6", "T32S3", "T64S2", "T16S7L", "T32S4L",
            "T32S3D7", "T16S6D1", "T8S2", "T16S4", "L4", "M6")
RX_L4 = VARIANTS.index("L4")

_libs = {}
ABI = 6   # include/pptk_rx.h PPTK_RX_ABI


def lib(path=None):
    """Load libpptkrx.so (or the A/B build at `path`) once; raise if it is
    missing (no fallback)."""
    path = path or LIB_PATH
    if path not in _libs:
        if not os.path.exists(path):
            raise ImportError(f"{path} not built: run `make` or __graft_entry__.build()")
        L = ctypes.CDLL(path)
        vp = ctypes.c_void_p
        # the struct layouts below are PPTK_RX_ABI's (older A/B builds lack
        # the symbol and are taken as they are)
        if hasattr(L, "pptk_rx_abi") and L.pptk_rx_abi() != ABI:
            raise ImportError(f"{path}: struct layout revision {L.pptk_rx_abi()}, "
                              f"this binding expects {ABI}")
        L.pptk_rx_opts_default.argtypes = [ctypes.POINTER(RxOpts)]
        L.pptk_rx_opts_default.restype = None
        L.pptk_rx_ctx_create.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(RxOpts)]
        L.pptk_rx_ctx_create.restype = ctypes.c_int
        L.pptk_rx_ctx_destroy.argtypes = [vp]
        L.pptk_rx_ctx_destroy.restype = None
        L.pptk_rx_batch.argtypes = [vp, vp, ctypes.c_int, vp]
        L.pptk_rx_batch.restype = ctypes.c_int
        if hasattr(L, "pptk_rx_batch32"):   # (absent from older A/B builds)
            for f in ("pptk_rx_batch32", "pptk_rx_batch_submit32"):
                getattr(L, f).argtypes = [vp, vp, ctypes.c_int, vp]
                getattr(L, f).restype = ctypes.c_int
        L.pptk_rx_batch_device.argtypes = [vp, ctypes.POINTER(RxDevBatch), vp]
        L.pptk_rx_batch_device.restype = ctypes.c_int
        L.pptk_rx_bin_scratch_bytes.argtypes = [ctypes.c_uint64]
        L.pptk_rx_bin_scratch_bytes.restype = ctypes.c_size_t
        L.pptk_rx_bin_device.argtypes = [vp, vp, ctypes.c_uint64, vp, vp, vp]
        L.pptk_rx_bin_device.restype = ctypes.c_int
        if hasattr(L, "pptk_tx_cksum_device"):         # absent from older A/B builds
            L.pptk_tx_cksum_device.argtypes = [vp, vp, vp, vp, ctypes.c_uint64, ctypes.c_uint32,
                                               ctypes.c_uint64, ctypes.c_uint32, vp]
            L.pptk_tx_cksum_device.restype = ctypes.c_int
        if hasattr(L, "pptk_tx_set_side_buffer"):      # absent from older A/B builds
            L.pptk_tx_set_side_buffer.argtypes = [vp, vp, ctypes.c_uint64]
            L.pptk_tx_set_side_buffer.restype = ctypes.c_int
        if hasattr(L, "pptk_tx_rewrite_device"):       # absent from older A/B builds
            L.pptk_tx_rewrite_device.argtypes = [vp, vp, vp, vp, ctypes.c_uint64, ctypes.c_uint32,
                                                 ctypes.c_uint64, vp, ctypes.c_uint64, vp, vp]
            L.pptk_tx_rewrite_device.restype = ctypes.c_int
        if hasattr(L, "pptk_rx_autotune"):             # absent from older A/B builds
            L.pptk_rx_autotune.argtypes = [vp, ctypes.POINTER(RxDevBatch), ctypes.c_int, vp]
            L.pptk_rx_autotune.restype = ctypes.c_int
        if hasattr(L, "pptk_rx_place_records"):        # absent from older A/B builds
            L.pptk_rx_place_records.argtypes = [vp, ctypes.POINTER(RxDevBatch), ctypes.POINTER(vp),
                                                ctypes.c_int, ctypes.c_int,
                                                ctypes.POINTER(ctypes.c_int),
                                                ctypes.POINTER(ctypes.c_float), vp]
            L.pptk_rx_place_records.restype = ctypes.c_int
        if hasattr(L, "pptk_rx_place_buffers"):        # absent from older A/B builds
            L.pptk_rx_place_buffers.argtypes = [vp, ctypes.POINTER(RxDevBatch), ctypes.POINTER(vp),
                                                ctypes.c_int, ctypes.POINTER(vp), ctypes.c_int,
                                                ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                                ctypes.POINTER(ctypes.c_int),
                                                ctypes.POINTER(ctypes.c_float), vp]
            L.pptk_rx_place_buffers.restype = ctypes.c_int
        if hasattr(L, "pptk_rx_ring_alloc"):           # absent from older A/B builds
            L.pptk_rx_ring_alloc.argtypes = [vp, ctypes.POINTER(RxRingSpec),
                                             ctypes.POINTER(RxRingC), vp]
            L.pptk_rx_ring_alloc.restype = ctypes.c_int
            L.pptk_rx_ring_free.argtypes = [ctypes.POINTER(RxRingC)]
            L.pptk_rx_ring_free.restype = ctypes.c_int
        if hasattr(L, "pptk_rx_gather_alloc"):         # absent from older A/B builds
            L.pptk_rx_gather_alloc.argtypes = [vp, ctypes.POINTER(RxDevBatch),
                                               ctypes.POINTER(RxGatherSpec),
                                               ctypes.POINTER(RxGatherC), vp]
            L.pptk_rx_gather_alloc.restype = ctypes.c_int
            L.pptk_rx_gather_free.argtypes = [ctypes.POINTER(RxGatherC)]
            L.pptk_rx_gather_free.restype = ctypes.c_int
        if hasattr(L, "pptk_tcp_mss_clamp_device"):    # absent from older A/B builds
            L.pptk_tcp_mss_clamp_device.argtypes = [vp, vp, vp, vp, ctypes.c_uint64,
                                                    ctypes.c_uint32, ctypes.c_uint64,
                                                    ctypes.c_uint16, ctypes.c_uint32, vp, vp]
            L.pptk_tcp_mss_clamp_device.restype = ctypes.c_int
        if hasattr(L, "pptk_tcp_seq_translate_device"):   # absent from older A/B builds
            L.pptk_tcp_seq_translate_device.argtypes = [vp, vp, vp, vp, ctypes.c_uint64,
                                                        ctypes.c_uint32, ctypes.c_uint64, vp,
                                                        ctypes.c_uint64, vp, vp, vp]
            L.pptk_tcp_seq_translate_device.restype = ctypes.c_int
            L.pptk_tcp_seq_translate_hdr.argtypes = [vp, ctypes.c_uint32, vp]
            L.pptk_tcp_seq_translate_hdr.restype = ctypes.c_uint32
        if hasattr(L, "pptk_ip_fragment_device"):      # absent from older A/B builds
            L.pptk_ip_fragment_scratch_bytes.argtypes = [ctypes.c_uint64]
            L.pptk_ip_fragment_scratch_bytes.restype = ctypes.c_size_t
            L.pptk_ip_fragment_device.argtypes = [vp, vp, vp, vp, ctypes.c_uint64,
                                                  ctypes.c_uint32, ctypes.c_uint64,
                                                  ctypes.c_uint32, vp, ctypes.c_uint64,
                                                  ctypes.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp]
            L.pptk_ip_fragment_device.restype = ctypes.c_int
            L.pptk_ip_fragment_host.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, vp,
                                                ctypes.c_uint64, ctypes.c_uint32, vp, vp]
            L.pptk_ip_fragment_host.restype = ctypes.c_int
        if hasattr(L, "pptk_tunnel_encap_device"):     # absent from older A/B builds
            L.pptk_tunnel_encap_device.argtypes = [vp, vp, vp, vp, ctypes.c_uint64,
                                                   ctypes.c_uint32, ctypes.c_uint64, vp,
                                                   ctypes.c_uint64, vp, ctypes.c_uint32, vp,
                                                   ctypes.c_uint64, vp, vp, vp]
            L.pptk_tunnel_encap_device.restype = ctypes.c_int
            L.pptk_tunnel_decap_device.argtypes = [vp, vp, vp, vp, ctypes.c_uint64,
                                                   ctypes.c_uint32, ctypes.c_uint64, vp, vp, vp,
                                                   vp]
            L.pptk_tunnel_decap_device.restype = ctypes.c_int
            L.pptk_tunnel_encap_host.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_uint32, vp,
                                                 ctypes.c_uint64, vp]
            L.pptk_tunnel_encap_host.restype = ctypes.c_uint32
            L.pptk_tunnel_decap_host.argtypes = [vp, ctypes.c_uint32, vp, vp]
            L.pptk_tunnel_decap_host.restype = ctypes.c_uint32
        if hasattr(L, "pptk_flow_table_create"):       # absent from older A/B builds
            u32, u64 = ctypes.c_uint32, ctypes.c_uint64
            L.pptk_flow_table_create.argtypes = [vp, u32, ctypes.POINTER(vp)]
            L.pptk_flow_table_create.restype = ctypes.c_int
            L.pptk_flow_table_destroy.argtypes = [vp]
            L.pptk_flow_table_destroy.restype = None
            L.pptk_flow_key_from_rec.argtypes = [vp, vp]
            L.pptk_flow_key_from_rec.restype = None
            L.pptk_flow_key_hash.argtypes = [vp, vp]
            L.pptk_flow_key_hash.restype = u64
            for f in ("pptk_flow_table_insert", "pptk_flow_table_update"):
                getattr(L, f).argtypes = [vp, vp, u64, u32]
                getattr(L, f).restype = ctypes.c_int
            L.pptk_flow_table_delete.argtypes = [vp, vp, u64]
            L.pptk_flow_table_delete.restype = ctypes.c_int
            L.pptk_flow_table_find.argtypes = [vp, vp, u64, ctypes.POINTER(u32)]
            L.pptk_flow_table_find.restype = ctypes.c_int
            L.pptk_flow_table_insert_recs.argtypes = [vp, vp, u64, vp, vp]
            L.pptk_flow_table_insert_recs.restype = ctypes.c_int
            L.pptk_flow_table_clear.argtypes = [vp]
            L.pptk_flow_table_clear.restype = None
            L.pptk_flow_table_stats.argtypes = [vp] + [ctypes.POINTER(u32)] * 3
            L.pptk_flow_table_stats.restype = None
            L.pptk_flow_table_sync.argtypes = [vp, vp, ctypes.POINTER(u64)]
            L.pptk_flow_table_sync.restype = ctypes.c_int
            L.pptk_flow_lookup_device.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp]
            L.pptk_flow_lookup_device.restype = ctypes.c_int
            L.pptk_flow_lookup_host.argtypes = [vp, vp, u64, vp, vp, vp]
            L.pptk_flow_lookup_host.restype = ctypes.c_int
        if hasattr(L, "pptk_flow_account_device"):     # absent from older A/B builds
            u32, u64 = ctypes.c_uint32, ctypes.c_uint64
            L.pptk_flow_account_device.argtypes = [vp, vp, vp, u32, u64, vp, u64, vp, u64, vp]
            L.pptk_flow_account_device.restype = ctypes.c_int
            L.pptk_flow_account_host.argtypes = [vp, vp, u32, u64, vp, u64, vp, u64]
            L.pptk_flow_account_host.restype = ctypes.c_int
            L.pptk_flow_stats_reset_device.argtypes = [vp, vp, u64, vp, u64, u64, vp]
            L.pptk_flow_stats_reset_device.restype = ctypes.c_int
            L.pptk_flow_account_shape.argtypes = [ctypes.POINTER(u32), ctypes.POINTER(u32)]
            L.pptk_flow_account_shape.restype = None
            L.pptk_flow_table_expire.argtypes = [vp, vp, u64, u64, u64, vp, u32]
            L.pptk_flow_table_expire.restype = ctypes.c_int
            L.pptk_tx_rewrite_flow_device.argtypes = [vp, vp, vp, vp, u64, u32, u64, vp, u64, vp,
                                                      vp, vp]
            L.pptk_tx_rewrite_flow_device.restype = ctypes.c_int
        if hasattr(L, "pptk_flow_learn_device"):       # absent from older A/B builds
            u32, u64 = ctypes.c_uint32, ctypes.c_uint64
            L.pptk_flow_learn_scratch_bytes.argtypes = [u64, u64]
            L.pptk_flow_learn_scratch_bytes.restype = ctypes.c_size_t
            L.pptk_flow_learn_device.argtypes = [vp, vp, vp, u64, u64, vp, vp, vp, u64, vp, vp,
                                                 ctypes.c_size_t, vp]
            L.pptk_flow_learn_device.restype = ctypes.c_int
            L.pptk_flow_learn_host.argtypes = [vp, vp, u64, u64, vp, vp, vp, u64, vp]
            L.pptk_flow_learn_host.restype = ctypes.c_int
            L.pptk_flow_learn_shape.argtypes = [ctypes.POINTER(u32), ctypes.POINTER(u32)]
            L.pptk_flow_learn_shape.restype = None
        if hasattr(L, "pptk_rx_permit_device"):        # absent from older A/B builds
            L.pptk_rx_permit_scratch_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint32]
            L.pptk_rx_permit_scratch_bytes.restype = ctypes.c_size_t
            L.pptk_rx_permit_device.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.c_int, vp,
                                                vp, vp, vp, vp]
            L.pptk_rx_permit_device.restype = ctypes.c_int
        if hasattr(L, "pptk_rx_permit_keys_device"):   # absent from older A/B builds
            L.pptk_rx_permit_keys_device.argtypes = [vp, vp, ctypes.c_uint64, ctypes.c_int, vp,
                                                     vp, vp, vp, vp]
            L.pptk_rx_permit_keys_device.restype = ctypes.c_int
            L.pptk_rx_tokens_refill_device.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint32,
                                                       ctypes.c_uint32, ctypes.c_uint32, vp]
            L.pptk_rx_tokens_refill_device.restype = ctypes.c_int
        if hasattr(L, "pptk_rx_permit_status"):        # absent from older A/B builds
            L.pptk_rx_permit_status.argtypes = [vp, vp, vp]
            L.pptk_rx_permit_status.restype = ctypes.c_int
        if hasattr(L, "pptk_rx_batch_device_mixed"):   # absent from older A/B builds
            L.pptk_rx_batch_device_mixed.argtypes = [vp, ctypes.POINTER(RxDevBatch), vp, vp, vp]
            L.pptk_rx_batch_device_mixed.restype = ctypes.c_int
        if hasattr(L, "pptk_rx_allgather_hash"):       # absent from older A/B builds
            L.pptk_rx_device_count.argtypes = []
            L.pptk_rx_device_count.restype = ctypes.c_int
            L.pptk_rx_comm_uid.argtypes = [vp]
            L.pptk_rx_comm_uid.restype = ctypes.c_int
            L.pptk_rx_comm_create.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp]
            L.pptk_rx_comm_create.restype = ctypes.c_int
            L.pptk_rx_comm_create_all.argtypes = [ctypes.POINTER(vp), ctypes.c_int]
            L.pptk_rx_comm_create_all.restype = ctypes.c_int
            L.pptk_rx_comm_destroy.argtypes = [vp]
            L.pptk_rx_comm_destroy.restype = ctypes.c_int
            L.pptk_rx_comm_info.argtypes = [vp, ctypes.POINTER(ctypes.c_int),
                                            ctypes.POINTER(ctypes.c_int)]
            L.pptk_rx_comm_info.restype = ctypes.c_int
            u64p = ctypes.POINTER(ctypes.c_uint64)
            L.pptk_rx_shard_range.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                              u64p, u64p, u64p]
            L.pptk_rx_shard_range.restype = None
            L.pptk_rx_allgather_hash.argtypes = [vp, vp, ctypes.c_uint64, vp, vp]
            L.pptk_rx_allgather_hash.restype = ctypes.c_int
        if hasattr(L, "pptk_rx_comm_sync"):            # absent from older A/B builds
            L.pptk_rx_comm_abort.argtypes = [vp]
            L.pptk_rx_comm_abort.restype = ctypes.c_int
            L.pptk_rx_comm_sync.argtypes = [vp, vp, ctypes.c_uint32]
            L.pptk_rx_comm_sync.restype = ctypes.c_int
        if hasattr(L, "pptk_rx_stream_split"):         # absent from older A/B builds
            L.pptk_rx_stream_split.argtypes = [vp, ctypes.c_int, ctypes.POINTER(vp),
                                               ctypes.POINTER(vp)]
            L.pptk_rx_stream_split.restype = ctypes.c_int
            L.pptk_rx_stream_destroy.argtypes = [vp]
            L.pptk_rx_stream_destroy.restype = ctypes.c_int
        L.pptk_rx_version.restype = ctypes.c_char_p
        L.pptk_rx_set_tuning.argtypes = [vp, ctypes.c_int, ctypes.c_int]
        L.pptk_rx_set_tuning.restype = ctypes.c_int
        L.pptk_rx_variant_count.restype = ctypes.c_int
        if hasattr(L, "pptk_rx_last_variant"):   # (absent from older A/B builds)
            L.pptk_rx_last_variant.argtypes = [vp]
            L.pptk_rx_last_variant.restype = ctypes.c_int
        if hasattr(L, "pptk_rx_batch_submit"):   # (absent from older A/B builds)
            L.pptk_rx_batch_submit.argtypes = [vp, vp, ctypes.c_int, vp]
            L.pptk_rx_batch_submit.restype = ctypes.c_int
            L.pptk_rx_batch_complete.argtypes = [vp]
            L.pptk_rx_batch_complete.restype = ctypes.c_int
            L.pptk_rx_batch_pending.argtypes = [vp]
            L.pptk_rx_batch_pending.restype = ctypes.c_int
        L.pptk_rx_register_ring.argtypes = [vp, vp, ctypes.c_size_t]
        L.pptk_rx_register_ring.restype = ctypes.c_int
        L.pptk_rx_unregister_ring.argtypes = [vp, vp]
        L.pptk_rx_unregister_ring.restype = ctypes.c_int
        L.ip_hdr_cksum_calc.argtypes = [vp, ctypes.c_uint16]
        L.ip_hdr_cksum_calc.restype = ctypes.c_uint16
        for f in ("tcp_cksum_calc", "udp_cksum_calc", "tcp6_cksum_calc", "udp6_cksum_calc"):
            getattr(L, f).argtypes = [vp, ctypes.c_uint16, vp, ctypes.c_uint16]
            getattr(L, f).restype = ctypes.c_uint16
        L.ip_cksum_feed.argtypes = [ctypes.POINTER(ctypes.c_uint32), vp, ctypes.c_size_t]
        L.ip_cksum_feed.restype = None
        _libs[path] = L
    return _libs[path]


def _dp(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


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
        rc = L.pptk_rx_ctx_create(ctypes.byref(self._ctx), ctypes.byref(o))
        if rc != 0:
            raise OSError(-rc, f"pptk_rx_ctx_create failed ({rc})")
        self.device = device

    def set_tuning(self, variant=-1, flags=-1):
        """Force kernel variant / memory-policy flags (speed only; -1 = auto)."""
        rc = self._L.pptk_rx_set_tuning(self._ctx, variant, flags)
        if rc != 0:
            raise OSError(-rc, f"pptk_rx_set_tuning({variant}, {flags}) failed")

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
        import torch
        rb = 32 if compact else 64
        if recs is None:
            recs = torch.empty((n, rb), dtype=torch.uint8, device=frames.device)
        b = RxDevBatch(frames.data_ptr(), None if off is None else off.data_ptr(),
                       None if lens is None else lens.data_ptr(),
                       None if perm is None else perm.data_ptr(), stride, fixed_len,
                       max_len, n, None if compact else recs.data_ptr(),
                       None if hash_out is None else hash_out.data_ptr(),
                       recs.data_ptr() if compact else None,
                       None if frag_out is None else frag_out.data_ptr(),
                       None if key_out is None else key_out.data_ptr())
        s = stream if stream is not None else torch.cuda.current_stream(frames.device)
        rc = self._L.pptk_rx_batch_device(self._ctx, ctypes.byref(b), ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise OSError(-rc, f"pptk_rx_batch_device failed ({rc})")
        return recs

    def autotune(self, frames, n, off=None, lens=None, stride=0, fixed_len=0, max_len=0,
                 recs=None, compact=False, reps=5, stream=None):
        """pptk_rx_autotune on this batch layout (synchronous): later device
        batches of the same shape use the fastest interchangeable kernel
        variant; returns its name (VARIANTS)."""
        import torch
        rb = 32 if compact else 64
        if recs is None:
            recs = torch.empty((n, rb), dtype=torch.uint8, device=frames.device)
        b = RxDevBatch(frames.data_ptr(), None if off is None else off.data_ptr(),
                       None if lens is None else lens.data_ptr(), None, stride, fixed_len,
                       max_len, n, None if compact else recs.data_ptr(), None,
                       recs.data_ptr() if compact else None)
        s = stream if stream is not None else torch.cuda.current_stream(frames.device)
        rc = self._L.pptk_rx_autotune(self._ctx, ctypes.byref(b), reps,
                                      ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise OSError(-rc, f"pptk_rx_autotune failed ({rc})")
        return self.tuned_variant(frames, n, off, lens, stride, fixed_len, max_len, compact)

    def place_records(self, frames, n, cands, off=None, lens=None, stride=0, fixed_len=0,
                      max_len=0, compact=False, reps=3, stream=None):
        """pptk_rx_place_records: run the batch into each candidate record
        buffer (torch uint8 CUDA tensors of n x 64 or n x 32 bytes) and
        return (index of the fastest, per-candidate median ms)."""
        import torch
        arr = (ctypes.c_void_p * max(1, len(cands)))(*[t.data_ptr() for t in cands])
        c0 = cands[0].data_ptr() if cands else None
        b = RxDevBatch(frames.data_ptr(), None if off is None else off.data_ptr(),
                       None if lens is None else lens.data_ptr(), None, stride, fixed_len,
                       max_len, n, None if compact else c0, None, c0 if compact else None)
        best = ctypes.c_int(-1)
        ms = (ctypes.c_float * max(1, len(cands)))()
        s = stream if stream is not None else torch.cuda.current_stream(frames.device)
        rc = self._L.pptk_rx_place_records(self._ctx, ctypes.byref(b), arr, len(cands), reps,
                                           ctypes.byref(best), ms, ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise OSError(-rc, f"pptk_rx_place_records failed ({rc})")
        return best.value, [round(x, 4) for x in ms[:len(cands)]]

    def place_buffers(self, frame_cands, n, rec_cands, off=None, lens=None, stride=0,
                      fixed_len=0, max_len=0, compact=False, reps=3, stream=None):
        """pptk_rx_place_buffers: the batch (the same bytes in every frame
        candidate) on every (frames, records) pair; returns (frame index,
        record index, median ms per pair, frames-major)."""
        import torch
        nf, nr = len(frame_cands), len(rec_cands)
        fa = (ctypes.c_void_p * max(1, nf))(*[t.data_ptr() for t in frame_cands])
        ra = (ctypes.c_void_p * max(1, nr))(*[t.data_ptr() for t in rec_cands])
        f0 = frame_cands[0].data_ptr() if nf else None
        r0 = rec_cands[0].data_ptr() if nr else None
        b = RxDevBatch(f0, None if off is None else off.data_ptr(),
                       None if lens is None else lens.data_ptr(), None, stride, fixed_len,
                       max_len, n, None if compact else r0, None, r0 if compact else None)
        bf, br = ctypes.c_int(-1), ctypes.c_int(-1)
        ms = (ctypes.c_float * max(1, nf * nr))()
        dev = frame_cands[0].device if nf else torch.device("cuda", self.device)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        rc = self._L.pptk_rx_place_buffers(self._ctx, ctypes.byref(b), fa, nf, ra, nr, reps,
                                           ctypes.byref(bf), ctypes.byref(br), ms,
                                           ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise OSError(-rc, f"pptk_rx_place_buffers failed ({rc})")
        return bf.value, br.value, [round(x, 4) for x in ms[:nf * nr]]

    def ring_alloc(self, frame_bytes, nrec, rec_bytes=64, probe_len=0, frame_cands=0,
                   rec_cands=0, reps=0, settle=False, stream=None, budget_bytes=0,
                   probe_hash=False):
        """pptk_rx_ring_alloc: placed device frame and record rings (a
        DeviceRing; its .report carries the probe).  probe_hash: the probe
        batches also write dense flow hashes (PPTK_RX_RING_PROBE_HASH)."""
        import torch
        spec = RxRingSpec(frame_bytes, nrec, rec_bytes, probe_len, frame_cands, rec_cands, reps,
                          (RING_SETTLE if settle else 0) | (RING_PROBE_HASH if probe_hash else 0),
                          budget_bytes, 0)
        ring = RxRingC()
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        rc = self._L.pptk_rx_ring_alloc(self._ctx, ctypes.byref(spec), ctypes.byref(ring),
                                        ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise OSError(-rc, f"pptk_rx_ring_alloc failed ({rc})")
        return DeviceRing(self, ring)

    def gather_alloc(self, frames, n, per_rank, nranks, rank, off=None, lens=None, stride=0,
                     fixed_len=0, max_len=0, recs=None, compact=False, cands=0, reps=0,
                     settle=False, budget_bytes=0, stream=None):
        """pptk_rx_gather_alloc: this rank's two gather buffers, placed by a
        probe that runs the batch (frames/recs as for batch_device) with its
        hashes into each candidate; a DeviceGather."""
        import torch
        rb = 32 if compact else 64
        if recs is None:
            recs = torch.empty((n, rb), dtype=torch.uint8, device=frames.device)
        b = RxDevBatch(frames.data_ptr(), None if off is None else off.data_ptr(),
                       None if lens is None else lens.data_ptr(), None, stride, fixed_len,
                       max_len, n, None if compact else recs.data_ptr(), None,
                       recs.data_ptr() if compact else None)
        spec = RxGatherSpec(per_rank, nranks, rank, cands, reps, RING_SETTLE if settle else 0, 0,
                            budget_bytes)
        g = RxGatherC()
        s = stream if stream is not None else torch.cuda.current_stream(frames.device)
        rc = self._L.pptk_rx_gather_alloc(self._ctx, ctypes.byref(b), ctypes.byref(spec),
                                          ctypes.byref(g), ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise OSError(-rc, f"pptk_rx_gather_alloc failed ({rc})")
        return DeviceGather(self, g)

    def tuned_variant(self, frames, n, off=None, lens=None, stride=0, fixed_len=0, max_len=0,
                      compact=False):
        """Name of the variant a device batch of this shape launches now
        (runs one batch of it: the variant is reported by the library)."""
        import torch
        self.batch_device(frames, n, off=off, lens=lens, stride=stride, fixed_len=fixed_len,
                          max_len=max_len, compact=compact)
        torch.cuda.synchronize(frames.device)
        return VARIANTS[self._L.pptk_rx_last_variant(self._ctx)]

    def batch_device_mixed(self, frames, n, off, lens, recs=None, hash_out=None, max_len=0,
                           perm=None, scratch=None, stream=None, frag_out=None):
        """Mixed-size batch (pptk_rx_batch_device_mixed, asynchronous): batch
        order, or device binning + one launch per length group when the batch
        mixes jumbo frames with shorter ones.  perm: optional device buffer
        that receives the processing order; scratch: optional preallocated."""
        import torch
        if recs is None:
            recs = torch.empty((n, 64), dtype=torch.uint8, device=frames.device)
        if scratch is None:
            scratch = torch.empty(self._L.pptk_rx_bin_scratch_bytes(n), dtype=torch.uint8,
                                  device=frames.device)
        b = RxDevBatch(frames.data_ptr(), off.data_ptr(), lens.data_ptr(), None, 0, 0,
                       max_len, n, recs.data_ptr(),
                       None if hash_out is None else hash_out.data_ptr(), None,
                       None if frag_out is None else frag_out.data_ptr())
        s = stream if stream is not None else torch.cuda.current_stream(frames.device)
        rc = self._L.pptk_rx_batch_device_mixed(self._ctx, ctypes.byref(b), _dp(perm),
                                                _dp(scratch), ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise OSError(-rc, f"pptk_rx_batch_device_mixed failed ({rc})")
        return recs

    def permit_device(self, recs, family, tokens, subject=None, compact=False, verdict=None,
                      scratch=None, stream=None):
        """Batched ip(v6)_permitted over device records (torch uint8 (n, 64)
        or (n, 32) with compact); tokens: torch int32 (iphash_size) updated
        in place; returns the uint8 verdicts (1 permit, 0 deny, 2 n/a)."""
        import torch
        n = recs.shape[0]
        if verdict is None:
            verdict = torch.empty(n, dtype=torch.uint8, device=recs.device)
        if scratch is None:
            scratch = torch.empty(self._L.pptk_rx_permit_scratch_bytes(n, tokens.numel()),
                                  dtype=torch.uint8, device=recs.device)
        s = stream if stream is not None else torch.cuda.current_stream(recs.device)
        rc = self._L.pptk_rx_permit_device(self._ctx, None if compact else _dp(recs),
                                           _dp(recs) if compact else None, n, family,
                                           _dp(subject), _dp(tokens), _dp(verdict),
                                           _dp(scratch), ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise OSError(-rc, f"pptk_rx_permit_device failed ({rc})")
        return verdict

    def permit_keys_device(self, keys, family, tokens, subject=None, verdict=None, scratch=None,
                           stream=None):
        """pptk_rx_permit_keys_device: the rate limiter from the dense keys
        (torch int32 (n,)) a batch wrote through key_out."""
        import torch
        n = keys.numel()
        if verdict is None:
            verdict = torch.empty(n, dtype=torch.uint8, device=keys.device)
        if scratch is None:
            scratch = torch.empty(self._L.pptk_rx_permit_scratch_bytes(n, tokens.numel()),
                                  dtype=torch.uint8, device=keys.device)
        s = stream if stream is not None else torch.cuda.current_stream(keys.device)
        rc = self._L.pptk_rx_permit_keys_device(self._ctx, _dp(keys), n, family, _dp(subject),
                                                _dp(tokens), _dp(verdict), _dp(scratch),
                                                ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise OSError(-rc, f"pptk_rx_permit_keys_device failed ({rc})")
        return verdict

    def permit_status(self, scratch, stream=None):
        """pptk_rx_permit_status: 0, or -ETIMEDOUT if a permit_keys_device
        call on `scratch` since the last query aborted (synchronises the
        stream)."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(scratch.device)
        return self._L.pptk_rx_permit_status(self._ctx, _dp(scratch), ctypes.c_void_p(s.cuda_stream))

    def tokens_refill_device(self, tokens, start, end, add, initial, stream=None):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(tokens.device)
        rc = self._L.pptk_rx_tokens_refill_device(self._ctx, _dp(tokens), start, end, add,
                                                  initial, ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise OSError(-rc, f"pptk_rx_tokens_refill_device failed ({rc})")

    def tx_cksum_device(self, frames, n, off=None, lens=None, stride=0, fixed_len=0, max_len=0,
                        stream=None):
        """Tx side: set the checksums of the frames in `frames` (torch uint8
        CUDA tensor) in place, asynchronously."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(frames.device)
        rc = self._L.pptk_tx_cksum_device(self._ctx, _dp(frames), _dp(off), _dp(lens), stride,
                                          fixed_len, n, max_len, ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise OSError(-rc, f"pptk_tx_cksum_device failed ({rc})")

    def tx_set_side_buffer(self, buf):
        """pptk_tx_set_side_buffer: `buf` (a CUDA tensor of >= 8 bytes per
        frame, kept alive by the caller) as the two-pass tx side array, or
        None for the context's own."""
        nbytes = 0 if buf is None else buf.numel() * buf.element_size()
        rc = self._L.pptk_tx_set_side_buffer(self._ctx, _dp(buf), nbytes // 8)
        if rc != 0:
            raise OSError(-rc, f"pptk_tx_set_side_buffer failed ({rc})")
        self._tx_side = buf

    def tx_rewrite_device(self, frames, n, rw, off=None, lens=None, stride=0, fixed_len=0,
                          status=None, stream=None):
        """Header rewrite with incremental checksum updates, in place and
        asynchronously.  rw: torch uint8 CUDA tensor of 1 or n struct
        pptk_rewrite entries (16 bytes each, records.REWRITE_DTYPE);
        status: optional torch uint8 CUDA tensor of n PPTK_RW_ST_* bytes."""
        import torch
        count = rw.numel() // 16
        s = stream if stream is not None else torch.cuda.current_stream(frames.device)
        rc = self._L.pptk_tx_rewrite_device(self._ctx, _dp(frames), _dp(off), _dp(lens), stride,
                                            fixed_len, n, _dp(rw), count, _dp(status),
                                            ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise OSError(-rc, f"pptk_tx_rewrite_device failed ({rc})")

    def tx_rewrite_flow_device(self, frames, n, rw, idx=None, off=None, lens=None, stride=0,
                               fixed_len=0, status=None, stream=None):
        """pptk_tx_rewrite_flow_device: tx_rewrite_device with rw a table of
        struct pptk_rewrite entries indexed by idx (torch int32 CUDA tensor of
        n entries, the idx of flow_lookup_device; an index at or past the
        table, -1 = FLOW_NONE among them, leaves the frame alone with status
        records.RW_ST_NOFLOW).  idx=None is tx_rewrite_device itself."""
        import torch
        if not hasattr(self._L, "pptk_tx_rewrite_flow_device"):
            raise OSError(38, "this libpptkrx.so lacks pptk_tx_rewrite_flow_device")
        count = rw.numel() * rw.element_size() // 16
        s = stream if stream is not None else torch.cuda.current_stream(frames.device)
        rc = self._L.pptk_tx_rewrite_flow_device(self._ctx, _dp(frames), _dp(off), _dp(lens),
                                                 stride, fixed_len, n, _dp(rw), count, _dp(idx),
                                                 _dp(status), ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise OSError(-rc, f"pptk_tx_rewrite_flow_device failed ({rc})")

    def mss_clamp_device(self, frames, n, mss, syn_only=False, off=None, lens=None, stride=0,
                         fixed_len=0, status=None, stream=None):
        """TCP MSS clamping with incremental checksum update, in place and
        asynchronously; status: optional torch uint8 CUDA tensor of n
        PPTK_MSS_ST_* bytes."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(frames.device)
        rc = self._L.pptk_tcp_mss_clamp_device(self._ctx, _dp(frames), _dp(off), _dp(lens),
                                               stride, fixed_len, n, mss, 1 if syn_only else 0,
                                               _dp(status), ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise OSError(-rc, f"pptk_tcp_mss_clamp_device failed ({rc})")

    def seq_translate_device(self, frames, n, xl, idx=None, off=None, lens=None, stride=0,
                             fixed_len=0, status=None, stream=None):
        """TCP sequence-space translation (pptk_tcp_seq_translate_device), in
        place and asynchronously.  xl: torch uint8 CUDA tensor of struct
        pptk_seqxlate entries (24 bytes each, records.seqxlate_dtype): 1 or n
        of them, or a flow table indexed by idx (torch int32 CUDA tensor of n
        entries, -1 = 0xffffffff = no flow); status: optional torch uint8
        CUDA tensor of n PPTK_SEQ_ST_* bytes."""
        import torch
        if not hasattr(self._L, "pptk_tcp_seq_translate_device"):
            raise OSError(38, "this libpptkrx.so lacks pptk_tcp_seq_translate_device")
        count = xl.numel() * xl.element_size() // 24
        s = stream if stream is not None else torch.cuda.current_stream(frames.device)
        rc = self._L.pptk_tcp_seq_translate_device(self._ctx, _dp(frames), _dp(off), _dp(lens),
                                                   stride, fixed_len, n, _dp(xl), count,
                                                   _dp(idx), _dp(status),
                                                   ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise OSError(-rc, f"pptk_tcp_seq_translate_device failed ({rc})")

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
        import torch
        dev = frames.device
        out_stride = out_stride or (18 + mtu + 15) & ~15
        if out is None:
            out = torch.empty((out_cap, out_stride), dtype=torch.uint8, device=dev)
        if out_len is None:
            out_len = torch.empty(out_cap, dtype=torch.int16, device=dev)
        if out_src is None:
            out_src = torch.empty(out_cap, dtype=torch.int32, device=dev)
        if first is None:
            first = torch.empty(n, dtype=torch.int32, device=dev)
        if count is None:
            count = torch.empty(n, dtype=torch.int32, device=dev)
        if status is None:
            status = torch.empty(n, dtype=torch.uint8, device=dev)
        if totals is None:
            totals = torch.empty(2, dtype=torch.int64, device=dev)
        if scratch is None:
            scratch = torch.empty(self._L.pptk_ip_fragment_scratch_bytes(n), dtype=torch.uint8,
                                  device=dev)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        rc = self._L.pptk_ip_fragment_device(self._ctx, _dp(frames), _dp(off), _dp(lens), stride,
                                             fixed_len, n, mtu, _dp(out), out_stride, out_cap,
                                             _dp(out_len), _dp(out_src), _dp(first), _dp(count),
                                             _dp(status), _dp(totals), _dp(scratch),
                                             ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise OSError(-rc, f"pptk_ip_fragment_device failed ({rc})")
        return dict(out=out, out_stride=out_stride, out_len=out_len, out_src=out_src, first=first,
                    count=count, status=status, totals=totals, scratch=scratch)

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
        import torch
        from .records import TUN_DF, TUN_HDR_LEN, TUN_ID_SEQ, TUNNEL_DTYPE
        if not hasattr(self._L, "pptk_tunnel_encap_device"):
            raise OSError(38, "this libpptkrx.so lacks pptk_tunnel_encap_device")
        dev = frames.device
        if isinstance(tun, np.ndarray):
            t = np.ascontiguousarray(tun, dtype=TUNNEL_DTYPE).reshape(-1)
            if np.any(t["reserved"]) or np.any(t["flags"] & ~np.uint32(TUN_DF | TUN_ID_SEQ)):
                raise OSError(22, "struct pptk_tunnel: reserved must be 0, flags DF | ID_SEQ")
            tun = torch.from_numpy(t.view(np.uint8).copy()).to(dev)
        count = tun.numel() * tun.element_size() // 32
        if not out_stride:
            if lens is not None:   # (the lengths are device data: n x 64 KB would be the only safe guess)
                raise ValueError("tunnel_encap_device: out_stride is required with lens")
            out_stride = (TUN_HDR_LEN + fixed_len + 15) & ~15
        if out is None:
            out = torch.empty((n, out_stride), dtype=torch.uint8, device=dev)
        if out_len is None:
            out_len = torch.empty(n, dtype=torch.int16, device=dev)
        if status is None:
            status = torch.empty(n, dtype=torch.uint8, device=dev)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        rc = self._L.pptk_tunnel_encap_device(self._ctx, _dp(frames), _dp(off), _dp(lens), stride,
                                              fixed_len, n, _dp(tun), count, _dp(idx), id_base,
                                              _dp(out), out_stride, _dp(out_len), _dp(status),
                                              ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise OSError(-rc, f"pptk_tunnel_encap_device failed ({rc})")
        return dict(out=out, out_stride=out_stride, out_len=out_len, status=status, tun=tun)

    def tunnel_decap_device(self, frames, n, off=None, lens=None, stride=0, fixed_len=0,
                            in_off=None, in_len=None, status=None, stream=None):
        """GRE decapsulation (pptk_tunnel_decap_device), asynchronous and
        zero-copy: descriptors of the inner frames inside `frames`.
        Allocates what is not given -- in_off (int64), in_len (int16), status
        (uint8) -- and returns them as a dict; in_off / in_len go into
        batch_device as off / lens."""
        import torch
        if not hasattr(self._L, "pptk_tunnel_decap_device"):
            raise OSError(38, "this libpptkrx.so lacks pptk_tunnel_decap_device")
        dev = frames.device
        if in_off is None:
            in_off = torch.empty(n, dtype=torch.int64, device=dev)
        if in_len is None:
            in_len = torch.empty(n, dtype=torch.int16, device=dev)
        if status is None:
            status = torch.empty(n, dtype=torch.uint8, device=dev)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        rc = self._L.pptk_tunnel_decap_device(self._ctx, _dp(frames), _dp(off), _dp(lens), stride,
                                              fixed_len, n, _dp(in_off), _dp(in_len), _dp(status),
                                              ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise OSError(-rc, f"pptk_tunnel_decap_device failed ({rc})")
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
        import torch
        if not hasattr(self._L, "pptk_flow_lookup_device"):
            raise OSError(38, "this libpptkrx.so lacks pptk_flow_lookup_device")
        dev = recs.device
        n = recs.numel() * recs.element_size() // 64
        if idx is None:
            idx = torch.empty(n, dtype=torch.int32, device=dev)
        if status is None:
            status = torch.empty(n, dtype=torch.uint8, device=dev)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        rc = self._L.pptk_flow_lookup_device(self._ctx, table._t, _dp(recs), n, _dp(subject),
                                             _dp(idx), _dp(status),
                                             ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise OSError(-rc, f"pptk_flow_lookup_device failed ({rc})")
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
        import torch
        if not hasattr(self._L, "pptk_flow_account_device"):
            raise OSError(38, "this libpptkrx.so lacks pptk_flow_account_device")
        n = idx.numel() if n is None else n
        count = stats.numel() * stats.element_size() // 32
        s = stream if stream is not None else torch.cuda.current_stream(stats.device)
        rc = self._L.pptk_flow_account_device(self._ctx, _dp(idx), _dp(lens), fixed_len, n,
                                              _dp(stats), count, _dp(unmatched), now,
                                              ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise OSError(-rc, f"pptk_flow_account_device failed ({rc})")

    def flow_stats_reset_device(self, stats, values, now, stream=None):
        """pptk_flow_stats_reset_device, asynchronous: stats[v] = {0, 0, now}
        for every v of values (torch int32 CUDA tensor) inside the array."""
        import torch
        if not hasattr(self._L, "pptk_flow_stats_reset_device"):
            raise OSError(38, "this libpptkrx.so lacks pptk_flow_stats_reset_device")
        count = stats.numel() * stats.element_size() // 32
        s = stream if stream is not None else torch.cuda.current_stream(stats.device)
        rc = self._L.pptk_flow_stats_reset_device(self._ctx, _dp(stats), count, _dp(values),
                                                  values.numel(), now,
                                                  ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise OSError(-rc, f"pptk_flow_stats_reset_device failed ({rc})")

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
        import torch
        if not hasattr(self._L, "pptk_flow_learn_device"):
            raise OSError(38, "this libpptkrx.so lacks pptk_flow_learn_device")
        dev = recs.device
        n = recs.numel() * recs.element_size() // 64 if n is None else n
        if new_recs is None and cap:
            new_recs = torch.empty(cap * 64, dtype=torch.uint8, device=dev)
        if first is None:
            first = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        if packets is None:
            packets = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        first = None if first is False else first
        packets = None if packets is False else packets
        if hdr is None:
            hdr = torch.empty(4, dtype=torch.int64, device=dev)
        need = self._L.pptk_flow_learn_scratch_bytes(n, max_candidates)
        if scratch is None:
            scratch = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        rc = self._L.pptk_flow_learn_device(self._ctx, _dp(recs), _dp(status), n, max_candidates,
                                            _dp(new_recs), _dp(first), _dp(packets), cap,
                                            _dp(hdr), _dp(scratch),
                                            scratch.numel() * scratch.element_size(),
                                            ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise OSError(-rc, f"pptk_flow_learn_device failed ({rc})")
        return dict(hdr=hdr, new_recs=new_recs, first=first, packets=packets, scratch=scratch)

    # ---- multi-GPU (RCCL) -------------------------------------------------
    def comm_create(self, nranks, rank, uid):
        """Join communicator `uid` (bytes from comm_uid()) as rank/nranks."""
        rc = self._L.pptk_rx_comm_create(self._ctx, nranks, rank, bytes(uid))
        if rc != 0:
            raise OSError(-rc, f"pptk_rx_comm_create({nranks}, {rank}) failed ({rc})")

    def comm_destroy(self):
        rc = self._L.pptk_rx_comm_destroy(self._ctx)
        if rc != 0:
            raise OSError(-rc, f"pptk_rx_comm_destroy failed ({rc})")

    def comm_abort(self):
        """pptk_rx_comm_abort: cancel the communicator (any thread)."""
        rc = self._L.pptk_rx_comm_abort(self._ctx)
        if rc != 0:
            raise OSError(-rc, f"pptk_rx_comm_abort failed ({rc})")

    def comm_sync(self, stream=None, timeout_ms=0):
        """pptk_rx_comm_sync: bounded wait for `stream` (torch stream, None =
        current) with RCCL error checks; returns 0 or the negative errno
        (-ETIMEDOUT / -EIO / -ECANCELED: the communicator is then dead)."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        return self._L.pptk_rx_comm_sync(self._ctx, ctypes.c_void_p(s.cuda_stream), timeout_ms)

    def comm_info(self):
        """(nranks, rank) of the context's communicator, or None."""
        nr, r = ctypes.c_int(), ctypes.c_int()
        rc = self._L.pptk_rx_comm_info(self._ctx, ctypes.byref(nr), ctypes.byref(r))
        return None if rc != 0 else (nr.value, r.value)

    def allgather_hash(self, d_hash, n, d_out, stream=None):
        """pptk_rx_allgather_hash: n u64 per rank from d_hash into d_out
        (torch int64 CUDA tensors), asynchronous on `stream`."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(d_out.device)
        rc = self._L.pptk_rx_allgather_hash(self._ctx, _dp(d_hash), n, _dp(d_out),
                                            ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise OSError(-rc, f"pptk_rx_allgather_hash failed ({rc})")

    def stream_split(self, coll_cus):
        """pptk_rx_stream_split: (rx stream, collective stream) as torch
        streams on this context's device, the collective's holding coll_cus
        CUs (a multiple of 32 on an MI355X) and the batches' the rest; the
        context sizes its grids for the rest until stream_join().  Call it
        before creating the communicator (its channel cap follows coll_cus).
        The HIP streams belong to the context and are destroyed with it."""
        import torch
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        rc = self._L.pptk_rx_stream_split(self._ctx, coll_cus, ctypes.byref(a), ctypes.byref(b))
        if rc != 0:
            raise OSError(-rc, f"pptk_rx_stream_split({coll_cus}) failed ({rc})")
        dev = torch.device("cuda", self.device)
        return (torch.cuda.ExternalStream(a.value, device=dev),
                torch.cuda.ExternalStream(b.value, device=dev))

    def stream_join(self):
        """Undo stream_split: the whole chip for this context's grids again
        (the split's streams stay the context's until close())."""
        if not hasattr(self._L, "pptk_rx_stream_split"):
            return
        self._L.pptk_rx_stream_split(self._ctx, 0, None, None)

    def bin_device(self, lens, n, stream=None):
        """Stable permutation of 0..n-1 by length class (torch uint32 tensor)."""
        import torch
        perm = torch.empty(n, dtype=torch.int32, device=lens.device)
        scratch = torch.empty(self._L.pptk_rx_bin_scratch_bytes(n), dtype=torch.uint8,
                              device=lens.device)
        s = stream if stream is not None else torch.cuda.current_stream(lens.device)
        rc = self._L.pptk_rx_bin_device(self._ctx, _dp(lens), n, _dp(perm), _dp(scratch),
                                      ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise OSError(-rc, f"pptk_rx_bin_device failed ({rc})")
        return perm

    def register_ring(self, buf):
        """Register numpy buffer `buf` as a zero-copy rx ring."""
        rc = self._L.pptk_rx_register_ring(self._ctx, ctypes.c_void_p(buf.ctypes.data), buf.nbytes)
        if rc != 0:
            raise OSError(-rc, "pptk_rx_register_ring failed")

    def unregister_ring(self, buf):
        rc = self._L.pptk_rx_unregister_ring(self._ctx, ctypes.c_void_p(buf.ctypes.data))
        if rc != 0:
            raise OSError(-rc, "pptk_rx_unregister_ring failed")

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
        rc = fn(self._ctx, ctypes.cast(pkts, ctypes.c_void_p), n, ctypes.c_void_p(recs.ctypes.data))
        if rc != 0:
            raise OSError(-rc, f"pptk_rx_batch{'32' if compact else ''} failed ({rc})")
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
        rc = fn(self._ctx, ctypes.cast(pkts, ctypes.c_void_p), n, ctypes.c_void_p(out.ctypes.data))
        if rc != 0:
            raise OSError(-rc, f"pptk_rx_batch_submit failed ({rc})")
        # the library holds pointers into both until the batch completes:
        # keep the Python objects alive until then (FIFO, as completions)
        self._inflight.append((pkts, out))

    def complete_host(self):
        """pptk_rx_batch_complete: wait for the oldest outstanding batch;
        returns its frame count."""
        rc = self._L.pptk_rx_batch_complete(self._ctx)
        if rc < 0:
            raise OSError(-rc, f"pptk_rx_batch_complete failed ({rc})")
        self._inflight.popleft()
        return rc

    def pending_host(self):
        return self._L.pptk_rx_batch_pending(self._ctx)


def _flow_key(key):
    """One struct pptk_flow_key as a 40-byte uint8 array, from a
    records.FLOW_KEY_DTYPE entry or its bytes."""
    k = np.frombuffer(key.tobytes() if hasattr(key, "tobytes") else bytes(key), np.uint8)
    if k.size != 40:
        raise ValueError("key must be one struct pptk_flow_key (40 bytes)")
    return k


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
    r = np.frombuffer(rec.tobytes() if hasattr(rec, "tobytes") else bytes(rec), np.uint8)
    if r.size != 64:
        raise ValueError("rec must be one struct pptk_rx_rec (64 bytes)")
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
        if not hasattr(L, "pptk_flow_table_create"):
            raise OSError(38, "this libpptkrx.so lacks pptk_flow_table_create")
        self._t = ctypes.c_void_p()
        self._ctx = ctx   # (keeps the context alive as long as the table)
        rc = L.pptk_flow_table_create(ctx._ctx if ctx is not None else None, slots,
                                      ctypes.byref(self._t))
        if rc != 0:
            raise OSError(-rc, f"pptk_flow_table_create({slots}) failed ({rc})")

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
        rc = self.insert_rc(key, flow_hash, value)
        if rc != 0:
            raise OSError(-rc, f"pptk_flow_table_insert failed ({rc})")

    def update(self, key, flow_hash, value):
        rc = self.update_rc(key, flow_hash, value)
        if rc != 0:
            raise OSError(-rc, f"pptk_flow_table_update failed ({rc})")

    def delete(self, key, flow_hash):
        rc = self.delete_rc(key, flow_hash)
        if rc != 0:
            raise OSError(-rc, f"pptk_flow_table_delete failed ({rc})")

    def find(self, key, flow_hash):
        """The key's value, or None if it is absent."""
        v = ctypes.c_uint32(0)
        k = _flow_key(key)
        rc = self._L.pptk_flow_table_find(self._t, k.ctypes.data, flow_hash, ctypes.byref(v))
        if rc == -2:
            return None
        if rc != 0:
            raise OSError(-rc, f"pptk_flow_table_find failed ({rc})")
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
        rc = self._L.pptk_flow_table_insert_recs(self._t, r.ctypes.data, n, v.ctypes.data,
                                                 res.ctypes.data)
        if rc < 0:
            raise OSError(-rc, f"pptk_flow_table_insert_recs failed ({rc})")
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
        if self._ctx is None:
            s = None
        else:
            import torch
            s = stream if stream is not None else torch.cuda.current_stream(self._ctx.device)
            s = ctypes.c_void_p(s.cuda_stream)
        up = ctypes.c_uint64(0)
        rc = self._L.pptk_flow_table_sync(self._t, s, ctypes.byref(up))
        if rc != 0:
            raise OSError(-rc, f"pptk_flow_table_sync failed ({rc})")
        return up.value

    def expire(self, stats, now, idle, cap=None):
        """pptk_flow_table_expire: deletes up to cap (default: all) flows whose
        value v lies inside stats -- a NumPy array of records.FLOW_STATS_DTYPE,
        the downloaded copy -- with stats[v].last_seen + idle < now, and
        returns their values (uint32).  Call again while it returns cap
        values; sync() uploads the change."""
        if not hasattr(self._L, "pptk_flow_table_expire"):
            raise OSError(38, "this libpptkrx.so lacks pptk_flow_table_expire")
        st = _flow_stats(stats)
        cap = self.stats()["count"] if cap is None else cap
        out = np.zeros(max(cap, 1), np.uint32)
        rc = self._L.pptk_flow_table_expire(self._t, st.ctypes.data, st.size, now, idle,
                                            out.ctypes.data, cap)
        if rc < 0:
            raise OSError(-rc, f"pptk_flow_table_expire failed ({rc})")
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
        rc = self._L.pptk_flow_lookup_host(self._t, r.ctypes.data, n,
                                           None if sub is None else sub.ctypes.data,
                                           idx.ctypes.data, st.ctypes.data)
        if rc != 0:
            raise OSError(-rc, f"pptk_flow_lookup_host failed ({rc})")
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
    L = lib(lib_path)
    if not hasattr(L, "pptk_flow_account_host"):
        raise OSError(38, "this libpptkrx.so lacks pptk_flow_account_host")
    i = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
    ln = None if lens is None else np.ascontiguousarray(lens, dtype=np.uint16).reshape(-1)
    if ln is not None and ln.size != i.size:
        raise ValueError("flow_account_host: one length per index")
    st = _flow_stats(stats)
    um = None if unmatched is None else _flow_stats(unmatched)
    rc = L.pptk_flow_account_host(i.ctypes.data, None if ln is None else ln.ctypes.data, fixed_len,
                                  i.size, st.ctypes.data, st.size,
                                  None if um is None else um.ctypes.data, now)
    if rc != 0:
        raise OSError(-rc, f"pptk_flow_account_host failed ({rc})")


def flow_account_shape(lib_path=None):
    """pptk_flow_account_shape: (segment_frames, lds_slots) of the library's
    accounting kernel; lds_slots is 0 for a direct build."""
    L = lib(lib_path)
    if not hasattr(L, "pptk_flow_account_shape"):
        raise OSError(38, "this libpptkrx.so lacks pptk_flow_account_shape")
    s, k = ctypes.c_uint32(), ctypes.c_uint32()
    L.pptk_flow_account_shape(ctypes.byref(s), ctypes.byref(k))
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
    L = lib(lib_path)
    if not hasattr(L, "pptk_flow_learn_host"):
        raise OSError(38, "this libpptkrx.so lacks pptk_flow_learn_host")
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
    rc = L.pptk_flow_learn_host(r.ctypes.data, st.ctypes.data, n, max_candidates,
                                out.ctypes.data if cap else None, first.ctypes.data,
                                packets.ctypes.data, cap, hdr.ctypes.data)
    if rc != 0:
        raise OSError(-rc, f"pptk_flow_learn_host failed ({rc})")
    w = int(hdr["written"][0])
    return hdr[0], out[:w * 64].view(REC_DTYPE), first[:w], packets[:w]


def flow_learn_scratch_bytes(n, max_candidates, lib_path=None):
    """pptk_flow_learn_scratch_bytes: the device scratch a learn call over n
    frames with this max_candidates needs (0 for n = 0)."""
    L = lib(lib_path)
    if not hasattr(L, "pptk_flow_learn_scratch_bytes"):
        raise OSError(38, "this libpptkrx.so lacks pptk_flow_learn_scratch_bytes")
    return L.pptk_flow_learn_scratch_bytes(n, max_candidates)


def flow_learn_shape(lib_path=None):
    """pptk_flow_learn_shape: (block_frames, scan_width) of the library's
    learning kernels."""
    L = lib(lib_path)
    if not hasattr(L, "pptk_flow_learn_shape"):
        raise OSError(38, "this libpptkrx.so lacks pptk_flow_learn_shape")
    b, w = ctypes.c_uint32(), ctypes.c_uint32()
    L.pptk_flow_learn_shape(ctypes.byref(b), ctypes.byref(w))
    return b.value, w.value


def ip_fragment_host(frame, mtu, out_cap, out_stride=0, lib_path=None):
    """pptk_ip_fragment_host on one frame (bytes): (count, status, out,
    out_len) with out an (out_cap, out_stride) uint8 array pre-filled with
    0xEE whose rows [0, count) hold the fragments unless status has NOROOM."""
    L = lib(lib_path)
    out_stride = out_stride or (18 + mtu + 15) & ~15
    out = np.full((max(out_cap, 1), out_stride), 0xEE, np.uint8)
    out_len = np.zeros(max(out_cap, 1), np.uint16)
    status = ctypes.c_uint8(0)
    rc = L.pptk_ip_fragment_host(bytes(frame), len(frame), mtu, out.ctypes.data, out_stride,
                                 out_cap, out_len.ctypes.data, ctypes.byref(status))
    if rc < 0:
        raise OSError(-rc, f"pptk_ip_fragment_host failed ({rc})")
    return rc, status.value, out[:out_cap], out_len[:out_cap]


def tunnel_encap_host(frame, tun, seq=0, out_cap=None, lib_path=None):
    """pptk_tunnel_encap_host on one frame (bytes) with one struct
    pptk_tunnel (a records.TUNNEL_DTYPE entry or its 32 bytes): (status, out,
    out_len) with out an out_cap-byte uint8 array (round_up(38 + len, 16)
    unless given) pre-filled with 0xEE."""
    L = lib(lib_path)
    if not hasattr(L, "pptk_tunnel_encap_host"):
        raise OSError(38, "this libpptkrx.so lacks pptk_tunnel_encap_host")
    t = np.frombuffer(tun.tobytes() if hasattr(tun, "tobytes") else bytes(tun), np.uint8)
    if t.size != 32:
        raise ValueError("tun must be one struct pptk_tunnel (32 bytes)")
    frame = bytes(frame)
    if out_cap is None:
        out_cap = (38 + len(frame) + 15) & ~15
    out = np.full(max(out_cap, 1), 0xEE, np.uint8)
    out_len = ctypes.c_uint16(0xEEEE)
    st = L.pptk_tunnel_encap_host(frame, len(frame), t.ctypes.data, seq, out.ctypes.data, out_cap,
                                  ctypes.byref(out_len))
    return st, out[:out_cap], out_len.value


def tunnel_decap_host(frame, lib_path=None):
    """pptk_tunnel_decap_host on one frame (bytes): (status, in_off, in_len),
    the inner frame being frame[in_off:in_off + in_len] when status has OK."""
    L = lib(lib_path)
    if not hasattr(L, "pptk_tunnel_decap_host"):
        raise OSError(38, "this libpptkrx.so lacks pptk_tunnel_decap_host")
    frame = bytes(frame)
    in_off, in_len = ctypes.c_uint32(0xEEEEEEEE), ctypes.c_uint16(0xEEEE)
    st = L.pptk_tunnel_decap_host(frame, len(frame), ctypes.byref(in_off), ctypes.byref(in_len))
    return st, in_off.value, in_len.value


def tcp_seq_translate_hdr(segment_bytes, xl, lib_path=None):
    """pptk_tcp_seq_translate_hdr on one TCP segment (bytes, the TCP header
    first) with the translation xl (one records.seqxlate_dtype entry, or its
    24 bytes): (status, the segment's bytes afterwards)."""
    L = lib(lib_path)
    if not hasattr(L, "pptk_tcp_seq_translate_hdr"):
        raise OSError(38, "this libpptkrx.so lacks pptk_tcp_seq_translate_hdr")
    x = np.frombuffer(xl.tobytes() if hasattr(xl, "tobytes") else bytes(xl), np.uint8)
    if x.size != 24:
        raise ValueError("xl must be one struct pptk_seqxlate (24 bytes)")
    # a buffer of exactly len(segment) bytes (at least one, to have an address)
    seg = np.frombuffer(bytes(segment_bytes), np.uint8).copy()
    buf = seg if seg.size else np.zeros(1, np.uint8)
    st = L.pptk_tcp_seq_translate_hdr(buf.ctypes.data, seg.size, x.ctypes.data)
    return st, seg.tobytes()


def comm_uid(lib_path=None):
    """A new RCCL communicator id (128 bytes), made on one rank."""
    buf = ctypes.create_string_buffer(128)
    rc = lib(lib_path).pptk_rx_comm_uid(buf)
    if rc != 0:
        raise OSError(-rc, f"pptk_rx_comm_uid failed ({rc})")
    return buf.raw


def comm_create_all(ctxs):
    """One communicator over the contexts (one per GPU) of this process."""
    arr = (ctypes.c_void_p * len(ctxs))(*[c._ctx.value for c in ctxs])
    rc = ctxs[0]._L.pptk_rx_comm_create_all(arr, len(ctxs))
    if rc != 0:
        raise OSError(-rc, f"pptk_rx_comm_create_all failed ({rc})")


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
