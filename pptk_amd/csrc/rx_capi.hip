// rx_capi.hip -- the C-ABI shim of libpptkrx.so (include/pptk_rx.h).
//
// The context (one per rx thread) and the device-batch API: the device-
// resident batch entry points with their choice of variant, grid and memory
// policy, autotune, the tx and header ops, the rate limiter, length binning
// and the stream split.  The host-buffer batch pipeline, whose state the
// context owns, is rx_host.hip.  Error convention: 0 or -errno, never abort
// on packet content.
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <new>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/hashseed.h"
#include "rx_internal.h"

using namespace pptk;

struct pptk_rx_ctx {
  int device = 0;
  pptk_rx_opts opts{};
  RxKArgs tmpl{};      // key/iphash part of the kernel arguments
  void *d_zero = nullptr;  // 64 zeroed device bytes (RxKArgs::zero)
  // two-pass tx side arrays (8 B per frame): per call from this stream-
  // ordered pool (allocated and freed on the call's stream, so concurrent
  // tx calls on different streams never share one), or the caller's buffer
  hipMemPool_t txpool = nullptr;
  std::mutex txpool_mu;   // tx calls of one context may run on several threads
  uint64_t *d_txuser = nullptr;   // pptk_tx_set_side_buffer
  uint64_t txuser_n = 0;
  int ncu = 256;
  int coll_cus = 0;   // pptk_rx_stream_split: CUs the grids leave to the collective now
  // pptk_rx_stream_split's two streams, owned by the context: created by the
  // first split (or a split to another CU count before any communicator),
  // kept across pptk_rx_stream_split(0), destroyed by pptk_rx_ctx_destroy
  // after the communicator; split_cus = the collective stream's CUs
  hipStream_t split_rx = nullptr, split_coll = nullptr;
  int split_cus = 0;
  int bpc[RX_NVARIANTS] = {};
  int forced_variant = -1;
  int forced_flags = -1;   // the receive transform's memory policy, -1 automatic
  bool permit_passes = false;   // PPTK_RX_TUNE_PERMIT_PASSES set by pptk_rx_set_tuning
  int last_variant = -1;
  // pptk_rx_autotune's choice per automatic variant, for fixed-stride [0]
  // and offset-described [1] batches (-1: the automatic variant itself)
  int tuned[2][RX_NVARIANTS];
  HostPipe *host = nullptr;   // the host-batch pipeline's state (rx_host.hip)
  // RCCL communicator (rx_comm.hip), or null; atomic: pptk_rx_comm_abort
  // may read it from another rx thread while this one creates it
  std::atomic<void *> comm{nullptr};
};

namespace pptk {
int ctx_device(const pptk_rx_ctx *c) { return c->device; }
const pptk_rx_opts &ctx_opts(const pptk_rx_ctx *c) { return c->opts; }
HostPipe *ctx_host_pipe(const pptk_rx_ctx *c) { return c->host; }
std::atomic<void *> *ctx_comm_slot(pptk_rx_ctx *c) { return &c->comm; }
uint32_t ctx_comm_timeout_ms(const pptk_rx_ctx *c) {
  return c->opts.comm_timeout_ms ? c->opts.comm_timeout_ms : PPTK_RX_COMM_TIMEOUT_MS;
}
int ctx_coll_cap(const pptk_rx_ctx *c) { return c->split_coll ? c->split_cus : 0; }
}  // namespace pptk

// Streams pptk_rx_stream_split handed out, by owner (pptk_rx_stream_destroy
// refuses them: -EBUSY), and the ones a context destroy has since destroyed
// (a caller following the old contract -- destroy them after the context --
// gets 0 for those instead of a second hipStreamDestroy).
static std::mutex g_split_mu;
static std::unordered_map<hipStream_t, const pptk_rx_ctx *> g_split_owned;
static std::unordered_set<hipStream_t> g_split_retired;

// Destroy the context's split streams (after their work; the communicator
// that may have used the collective stream is gone or never existed).
static void drop_split_streams(pptk_rx_ctx *c) {
  hipStream_t s[2] = {c->split_rx, c->split_coll};
  {
    std::lock_guard<std::mutex> g(g_split_mu);
    for (hipStream_t x : s)
      if (x) {
        g_split_owned.erase(x);
        g_split_retired.insert(x);
      }
  }
  for (hipStream_t x : s)
    if (x) {
      (void)hipStreamSynchronize(x);
      (void)hipStreamDestroy(x);
    }
  c->split_rx = c->split_coll = nullptr;
  c->split_cus = 0;
}

static uint64_t le64(const uint8_t *p) {
  uint64_t v = 0;
  for (int i = 7; i >= 0; --i) v = (v << 8) | p[i];
  return v;
}

// The part the in-place header ops share: the checks on the batch layout
// (`op_ok` is the calling op's verdict on its own arguments), the context's
// device, the batch descriptor and the grid (one lane per frame, at most
// eight blocks per CU, grid-stride beyond).
template <class Launch>
static int hdr_op(struct pptk_rx_ctx *c, uint8_t *d_frames, const uint64_t *d_off,
                  const uint16_t *d_len, uint64_t stride, uint32_t fixed_len, uint64_t n,
                  uint8_t *d_status, bool op_ok, Launch launch) {
  if (!c || n > 0xffffffffull) return -EINVAL;
  if (n == 0) return 0;
  if (!op_ok || !frame_batch_ok(d_frames, d_off, d_len, stride, fixed_len, n)) return -EINVAL;
  DeviceScope dg(c->device);
  if (!dg.ok) return -EIO;
  const HdrBatch b = {{d_frames, d_off, d_len, stride, n, fixed_len}, d_frames, d_status};
  const uint64_t blocks = (n + 255) / 256;
  const int grid = (int)std::min<uint64_t>(blocks, (uint64_t)c->ncu * 8);
  return hip_rc(launch(b, grid));
}

extern "C" {

const char *pptk_rx_version(void) { return "pptk_amd rx 0.6 gfx950"; }

int pptk_rx_abi(void) { return PPTK_RX_ABI; }

void pptk_rx_opts_default(struct pptk_rx_opts *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->device = 0;
  if (hash_seed_inited) memcpy(o->key, hash_seed, 16);
  o->iphash_size = 1;
  o->max_batch = 8192;
  o->max_frame = 9216;
  o->comm_timeout_ms = PPTK_RX_COMM_TIMEOUT_MS;
}

int pptk_rx_ctx_create(struct pptk_rx_ctx **out, const struct pptk_rx_opts *opts) {
  if (!out || !opts) return -EINVAL;
  *out = nullptr;
  if (opts->iphash_bits4 > 32 || opts->iphash_bits6 > 128) return -EINVAL;
  if ((opts->iphash_bits4 || opts->iphash_bits6) &&
      (opts->iphash_size == 0 || (opts->iphash_size & (opts->iphash_size - 1))))
    return -EINVAL;
  if (opts->max_frame > 65535) return -EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || opts->device < 0 || opts->device >= ndev)
    return -EINVAL;
  pptk_rx_ctx *c = new (std::nothrow) pptk_rx_ctx();
  if (!c) return -ENOMEM;
  c->device = opts->device;
  c->opts = *opts;
  DeviceScope dg(c->device);
  if (!dg.ok) {
    delete c;
    return -EIO;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, c->device) == hipSuccess) c->ncu = prop.multiProcessorCount;
  for (int v = 0; v < RX_NVARIANTS; ++v) {
    c->bpc[v] = rx_variant_blocks_per_cu(v);
    c->tuned[0][v] = c->tuned[1][v] = -1;
  }
  if (hipMalloc(&c->d_zero, 64) != hipSuccess || hipMemset(c->d_zero, 0, 64) != hipSuccess ||
      !(c->host = host_pipe_create())) {
    (void)hipFree(c->d_zero);
    delete c;
    return -ENOMEM;
  }

  RxKArgs &t = c->tmpl;
  t.zero = c->d_zero;
  t.k0 = le64(opts->key);
  t.k1 = le64(opts->key + 8);
  t.bucket4 = opts->iphash_bits4 ? 1u : 0u;
  t.bucket6 = opts->iphash_bits6 ? 1u : 0u;
  t.hash_mask = opts->iphash_size ? opts->iphash_size - 1u : 0u;
  const uint32_t b4 = opts->iphash_bits4;
  t.mask4 = b4 >= 32 ? 0xffffffffu : (b4 == 0 ? 0u : ~((1u << (32 - b4)) - 1u));
  uint8_t m6[16];
  for (int b = 0; b < 16; ++b) {
    const int kept = std::min(std::max((int)opts->iphash_bits6 - 8 * b, 0), 8);
    m6[b] = (uint8_t)((0xff00u >> kept) & 0xffu);
  }
  t.mask6_0 = le64(m6);
  t.mask6_1 = le64(m6 + 8);
  *out = c;
  return 0;
}

void pptk_rx_ctx_destroy(struct pptk_rx_ctx *c) {
  if (!c) return;
  DeviceScope dg(c->device);
  comm_release(c);
  drop_split_streams(c);   // after the communicator that may have used them
  host_pipe_release(c->host);   // the slots, the worker pool
  (void)hipFree(c->d_zero);
  if (c->txpool) {   // its frees are queued on the callers' streams
    (void)hipDeviceSynchronize();
    (void)hipMemPoolDestroy(c->txpool);
  }
  host_pipe_destroy(c->host);   // the registered rings, last
  delete c;
}

static int pick_variant(uint32_t span) {
  if (span <= 64) return RX_T4S1;
  if (span <= 128) return RX_T4S2;
  if (span <= 256) return RX_T8S2;
  if (span <= 512) return RX_T16S2;
  if (span <= 1024) return RX_T16S4;
  if (span <= 1536) return RX_T16S6;
  return RX_T64S2;
}

// The result-preserving memory-policy bits (pptk_rx.h): the only ones
// pptk_rx_set_tuning and PPTK_RX_TUNE accept, so no tuning word can produce
// wrong records.
static constexpr uint32_t kTuneMask = PPTK_RX_TUNE_NT_LOADS | PPTK_RX_TUNE_NO_STAGING |
                                      PPTK_RX_TUNE_NT_STORES | PPTK_RX_TUNE_SC1_STORES |
                                      PPTK_RX_TUNE_BLOCKED | PPTK_RX_TUNE_PERMIT_PASSES;

// Memory policy (PPTK_RX_TUNE_*), from in-process A/B runs (DESIGN.md
// "Measurement log"): non-temporal record stores always (C64 0.468 -> 0.463
// ms, CMIX 3.05 -> 2.97 ms); non-temporal frame loads only for fixed-stride
// batches with the streaming variants (C1500 4.47 -> 4.25 ms; they cost 14 %
// on C64 and 10 % on offset-described CMIX).  PPTK_RX_TUNE overrides.
static long env_tune() {
  static const long tune = env_long("PPTK_RX_TUNE", -1);
  return tune;
}

static uint32_t pick_tune(const pptk_rx_ctx *c, int variant, bool gather, bool coal = false) {
  constexpr uint32_t rx_bits = kTuneMask & ~(uint32_t)PPTK_RX_TUNE_PERMIT_PASSES;
  if (c->forced_flags >= 0) return (uint32_t)c->forced_flags & rx_bits;
  // (an environment word holding only the rate limiter's bit leaves the
  // memory policy automatic, as pptk_rx_set_tuning does; any other word,
  // 0 included, forces the policy it names)
  const long tune = env_tune();
  if (tune >= 0 && tune != PPTK_RX_TUNE_PERMIT_PASSES) return (uint32_t)tune & rx_bits;
  // (the lane kernel on a packed run of 64-byte slots reads its tiles as
  // contiguous 1 KB runs, rx_kernel.hip lane_load: there non-temporal loads
  // pay, C64 0.3815 -> 0.3723 ms; on its per-frame loads they cost 22 %)
  const bool small = variant == RX_T4S1 || variant == RX_T4S2 || variant == RX_T8S2 ||
                     (variant == RX_L4 && !coal);
  return (small || gather) ? PPTK_RX_TUNE_NT_STORES
                           : (PPTK_RX_TUNE_NT_STORES | PPTK_RX_TUNE_NT_LOADS);
}

static int forced_variant(const pptk_rx_ctx *c) {
  // PPTK_RX_VARIANT: A/B override (results never change)
  static const long force = env_long("PPTK_RX_VARIANT", -1);
  if (c->forced_variant >= 0) return c->forced_variant;
  return force >= 0 && force < RX_NVARIANTS ? (int)force : -1;
}

// Blocks a launch may keep resident (the persistent grid): the variant's
// blocks per CU on every CU but the ones pptk_rx_stream_split left to the
// collective (the batches' stream cannot use them).
static uint64_t resident_blocks(const pptk_rx_ctx *c, int variant) {
  const uint64_t ncu = (uint64_t)std::max(1, c->ncu - std::min(c->coll_cus, c->ncu - 1));
  return ncu * (uint64_t)c->bpc[variant];
}

// Grid of a launch: by default persistent (every block resident, its waves
// striding over the tiles).  tpw > 0: enough blocks that each wave takes
// about tpw tiles -- more than are resident, so the dispatcher hands out
// the later blocks as earlier ones finish (tiles_per_wave).
static int grid_for(const pptk_rx_ctx *c, int variant, uint64_t n, uint32_t tpw = 0) {
  const uint64_t ntiles = (n + 63) / 64;
  const uint64_t want_blocks = (ntiles + kWavesPerBlock - 1) / kWavesPerBlock;
  if (tpw > 0) {
    const uint64_t per_block = (uint64_t)kWavesPerBlock * tpw;
    const uint64_t blocks = (ntiles + per_block - 1) / per_block;
    return (int)std::max<uint64_t>(1, std::min<uint64_t>(want_blocks,
                                                         std::max(blocks, resident_blocks(c, variant))));
  }
  return (int)std::max<uint64_t>(1, std::min<uint64_t>(want_blocks, resident_blocks(c, variant)));
}

// Tiles per wave of an oversubscribed grid (grid_for), 0 = persistent.  The
// lane kernel, and the streaming shapes on offset-described batches (tiles
// of uneven duration), run faster when the dispatcher hands out blocks of a
// few tiles per wave than when every wave owns a fixed share of the batch:
// in-process A/B (profiles/r06/grid/), C64 0.3764 -> 0.3580 ms (8 tiles)
// and 0.3972 -> 0.3615 (4), CMIX T16S6 2.5245 -> 2.4591 (8) and 2.5189 ->
// 2.4509 (4), M6 on CMIX 2.5563 -> 2.4439 and on IMIX 1.3977 -> 1.3385 (8);
// C1500 (fixed stride, T32S3) is unchanged and T16S6 on it is slower
// (4.1465 -> 4.3680), so fixed-stride streaming stays persistent, as does
// the jumbo shape T64S2 (JMIX 3.9191 -> 4.0169 with 4 tiles, equal with 8).
static uint32_t tiles_per_wave(int variant, bool gather) {
  if (variant == RX_L4) return 4;
  if (!gather) return 0;
  return variant == RX_T64S2 ? 0 : 8;
}

static uint64_t gcd64(uint64_t a, uint64_t b) {
  while (b) {
    const uint64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

static int check_batch(const pptk_rx_ctx *c, const pptk_rx_dev_batch *b) {
  if (!c || !b) return -EINVAL;
  if (b->n == 0) return 0;
  if (!b->d_recs && !b->d_recs32) return -EINVAL;
  if (b->n > 0xffffffffull) return -EINVAL;  // indices are 32-bit (d_perm)
  if (!frame_batch_ok(b->d_frames, b->d_off, b->d_len, b->stride, b->fixed_len, b->n))
    return -EINVAL;
  return 0;
}

static RxKArgs batch_args(const pptk_rx_ctx *c, const pptk_rx_dev_batch *b) {
  RxKArgs a = c->tmpl;
  a.frames = b->d_frames;
  a.off = b->d_off;
  a.len = b->d_len;
  a.perm = b->d_perm;
  a.stride = b->stride;
  a.fixed_len = b->fixed_len;
  a.n = b->n;
  a.recs = b->d_recs;
  a.recs32 = b->d_recs32;
  a.hash = b->d_hash;
  a.frag = b->d_frag;
  a.key = b->d_key;
  return a;
}

// The automatic kernel variant for a device batch: the lane kernel for
// fixed-stride 16-byte-aligned frames of at most 64 bytes, else the team
// shape sized for the longest frame plus its worst misalignment.
static int auto_variant(const pptk_rx_dev_batch *b, bool *lane_ok_out) {
  // worst misalignment of a frame start inside a 16-byte chunk
  uint32_t mmax = 15;
  if (!b->d_off) {
    const uint64_t p = (uint64_t)(uintptr_t)b->d_frames;
    const uint64_t gg = gcd64(b->stride % 16 ? b->stride % 16 : 16, 16);
    mmax = (uint32_t)((p % gg) + 16 - gg);
  }
  const uint32_t maxlen = b->d_len ? (b->max_len ? b->max_len : 65535u) : b->fixed_len;
  // the lane kernel takes fixed-stride batches of small frames that all
  // start on a 16-byte boundary (mmax == 0: aligned buffer and stride)
  // (and write no fragment side records: those come from lane_generic)
  // (an empty frame reads only the chunk holding its start, as the header
  // allows)
  const bool lane_ok = !b->d_off && !b->d_len && !b->d_perm && !b->d_frag && mmax == 0 &&
                       b->fixed_len <= 64;
  if (lane_ok_out) *lane_ok_out = lane_ok;
  return lane_ok ? RX_L4 : pick_variant(maxlen + mmax);
}

// The write-phase period of a launch (rx_kernel.hip "Global write phases"):
// ~0.75 of the time one wave takes for one 64-frame tile, estimated from the
// tile's frame bytes (fixed-stride batches: 64 strides; offset-described
// ones: 64 frames of half the max_len hint, as for lengths spread evenly up
// to it), the waves of the grid, and ~5.5 TB/s of frame stream.  Measured:
// the best periods lie at 0.6-0.9 of a tile (profiles/r05/w: C1500 30-40 us
// against 47-51 us tiles, CMIX 15-20 us against 20 us).  0 (off) for the
// small-frame shapes, permuted batches (records scatter) and tx batches.
static uint32_t phase_ticks_for(const pptk_rx_dev_batch *b, int variant, int grid) {
  if (!rx_variant_phased(variant) || b->d_perm || (!b->d_recs && !b->d_recs32)) return 0;
  const uint64_t maxlen = b->d_len ? (b->max_len ? b->max_len : 1518u) : b->fixed_len;
  // (a stride far past any frame only lengthens the estimate; capped so the
  // product below cannot overflow)
  const uint64_t tile_bytes =
      64 * (b->d_off ? std::max<uint64_t>(64, maxlen / 2)
                     : std::min<uint64_t>(std::max<uint64_t>(b->stride, 64), 1u << 20));
  const uint64_t waves = (uint64_t)grid * kWavesPerBlock;
  const uint64_t ticks = tile_bytes * waves * 3 / 4 / 55000;   // 5.5 TB/s = 55 000 B per tick
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(ticks, 100), 1000000);
}

static int launch_batch(pptk_rx_ctx *c, const pptk_rx_dev_batch *b, int variant, void *stream) {
  RxKArgs a = batch_args(c, b);
  a.tune = pick_tune(c, variant, b->d_off || b->d_len || b->d_perm,
                     variant == RX_L4 && lane_coalesced(b->stride, b->fixed_len));
  c->last_variant = variant;
  const bool gather = b->d_off || b->d_len || b->d_perm;
  const int grid = grid_for(c, variant, b->n, tiles_per_wave(variant, gather));
  // (the period follows the waves resident at once, not the whole grid)
  a.phase_ticks = phase_ticks_for(
      b, variant, (int)std::min<uint64_t>((uint64_t)grid, resident_blocks(c, variant)));
  return hip_rc(launch_rx(variant, a, grid, (hipStream_t)stream));
}

int pptk_rx_batch_device(struct pptk_rx_ctx *c, const struct pptk_rx_dev_batch *b,
                         void *stream) {
  int rc = check_batch(c, b);
  if (rc || b->n == 0) return rc;
  DeviceScope dg(c->device);
  if (!dg.ok) return -EIO;
  bool lane_ok = false;
  int variant = auto_variant(b, &lane_ok);
  const int tv = c->tuned[b->d_off || b->d_len || b->d_perm ? 1 : 0][variant];
  if (tv >= 0) variant = tv;                  // pptk_rx_autotune's choice
  const int fv = forced_variant(c);
  if (fv >= 0) variant = fv;
  if (variant == RX_L4 && !lane_ok) variant = auto_variant(b, nullptr);   // (a team shape)
  return launch_batch(c, b, variant, stream);
}

// Interchangeable shapes per automatic variant (same frame capacity, same
// results: every variant is parity-tested on every fixture).  Which is
// fastest depends on what the record writes cost (which follows the record
// buffer's placement): where they are expensive (the
// read/write-mix speed of light ~4.8 ms for C1500) T32S3D7 ran C1500 6 %
// faster than T16S6; T16S6 was chosen where the mix costs ~4.0 ms.  The
// 1536-byte class is the one measured.
static int autotune_candidates(int variant, bool gather, int cand[8]) {
  int n = 0;
  cand[n++] = variant;
  if (variant == RX_T16S6) {
    cand[n++] = RX_T32S3;
    cand[n++] = RX_T32S3D7;
    cand[n++] = RX_T16S7L;
    if (gather) cand[n++] = RX_M6;   // mixed lengths: lanes binned inside the tile
  }
  return n;
}

int pptk_rx_autotune(struct pptk_rx_ctx *c, const struct pptk_rx_dev_batch *b, int reps,
                     void *stream) {
  int rc = check_batch(c, b);
  if (rc || b->n == 0) return rc;
  if (reps < 1 || reps > 100) return -EINVAL;
  DeviceScope dg(c->device);
  if (!dg.ok) return -EIO;
  const int base = auto_variant(b, nullptr);
  const int g = b->d_off || b->d_len || b->d_perm ? 1 : 0;
  int cand[8];
  const int nc = autotune_candidates(base, g == 1, cand);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
    (void)hipEventDestroy(e0);
    return -EIO;
  }
  const hipStream_t s = (hipStream_t)stream;
  // Candidates interleaved round by round (two untimed warm-up rounds), so
  // that clock and thermal drift during the probe fall on all of them alike;
  // the fastest median wins, but a shape other than the automatic one must
  // beat it by 1 % (noise never moves the choice away from candidate 0).
  std::vector<std::vector<float>> ms((size_t)nc);
  for (int r = 0; r < reps + 2 && rc == 0; ++r) {
    for (int k = 0; k < nc && rc == 0; ++k) {
      if (hipEventRecord(e0, s) != hipSuccess) rc = -EIO;
      if (rc == 0) rc = launch_batch(c, b, cand[k], stream);
      if (rc == 0 && (hipEventRecord(e1, s) != hipSuccess ||
                      hipEventSynchronize(e1) != hipSuccess))
        rc = -EIO;
      float t = 0.f;
      if (rc == 0 && r >= 2 && hipEventElapsedTime(&t, e0, e1) == hipSuccess)
        ms[(size_t)k].push_back(t);
    }
  }
  int best = base;
  if (rc == 0 && !ms[0].empty()) {
    std::vector<float> med((size_t)nc, 1e30f);
    for (int k = 0; k < nc; ++k) {
      if (ms[(size_t)k].empty()) continue;
      std::sort(ms[(size_t)k].begin(), ms[(size_t)k].end());
      med[(size_t)k] = ms[(size_t)k][ms[(size_t)k].size() / 2];
    }
    int kb = 0;
    for (int k = 1; k < nc; ++k)
      if (med[(size_t)k] < med[(size_t)kb]) kb = k;
    if (kb != 0 && med[(size_t)kb] < 0.99f * med[0]) best = cand[kb];
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc == 0) c->tuned[g][base] = best == base ? -1 : best;
  return rc;
}

int pptk_rx_place_buffers(struct pptk_rx_ctx *c, const struct pptk_rx_dev_batch *b,
                          const uint8_t *const *fr, int nf, void *const *rc_, int nr, int reps,
                          int *best_f, int *best_r, float *ms_out, void *stream) {
  if (!c || !b || !fr || !rc_ || !best_f || !best_r || nf < 1 || nf > 16 || nr < 1 ||
      nr > 64 || nf * nr > 256 || reps < 1 || reps > 100)
    return -EINVAL;
  for (int k = 0; k < nf; ++k)
    if (!fr[k]) return -EINVAL;
  for (int k = 0; k < nr; ++k)
    if (!rc_[k]) return -EINVAL;
  pptk_rx_dev_batch t = *b;
  const bool c32 = b->d_recs32 != nullptr;
  t.d_frames = fr[0];
  t.d_recs = c32 ? nullptr : (pptk_rx_rec *)rc_[0];
  t.d_recs32 = c32 ? (pptk_rx_rec32 *)rc_[0] : nullptr;
  int rc = check_batch(c, &t);
  if (rc || b->n == 0) {
    if (rc == 0) *best_f = *best_r = 0;
    return rc;
  }
  DeviceScope dg(c->device);
  if (!dg.ok) return -EIO;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
    (void)hipEventDestroy(e0);
    return -EIO;
  }
  const hipStream_t s = (hipStream_t)stream;
  const int np = nf * nr;
  std::vector<std::vector<float>> ms((size_t)np);
  // pairs interleaved round by round, so that clock drift during the probe
  // falls on all of them alike; round 0 is the warm-up
  for (int r = 0; r <= reps && rc == 0; ++r) {
    for (int p = 0; p < np && rc == 0; ++p) {
      t.d_frames = fr[p / nr];
      if (c32) t.d_recs32 = (pptk_rx_rec32 *)rc_[p % nr];
      else t.d_recs = (pptk_rx_rec *)rc_[p % nr];
      if (hipEventRecord(e0, s) != hipSuccess) rc = -EIO;
      if (rc == 0) rc = pptk_rx_batch_device(c, &t, stream);
      if (rc == 0 && (hipEventRecord(e1, s) != hipSuccess || hipEventSynchronize(e1) != hipSuccess))
        rc = -EIO;
      float x = 0.f;
      if (rc == 0 && r > 0 && hipEventElapsedTime(&x, e0, e1) == hipSuccess)
        ms[(size_t)p].push_back(x);
    }
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc) return rc;
  int bp = 0;
  float bm = 1e30f;
  for (int p = 0; p < np; ++p) {
    std::vector<float> &v = ms[(size_t)p];
    std::sort(v.begin(), v.end());
    const float med = v.empty() ? 1e30f : v[v.size() / 2];
    if (ms_out) ms_out[p] = med;
    if (med < bm) {
      bm = med;
      bp = p;
    }
  }
  *best_f = bp / nr;
  *best_r = bp % nr;
  return 0;
}

int pptk_rx_place_records(struct pptk_rx_ctx *c, const struct pptk_rx_dev_batch *b,
                          void *const *cands, int ncand, int reps, int *best, float *ms_out,
                          void *stream) {
  if (!b || !best) return -EINVAL;
  const uint8_t *f0 = b->d_frames;
  int bf = 0;
  return pptk_rx_place_buffers(c, b, &f0, 1, cands, ncand, reps, &bf, best, ms_out, stream);
}

// Tx in two passes (fixed-stride batches): the streaming pass records each
// frame's checksum fields in a side array (8 B per frame) and a second
// kernel writes them, so that the 2-byte field writes do not land beside
// the 25 GB read stream (DESIGN.md "Secondary kernels").
int pptk_tx_cksum_device(struct pptk_rx_ctx *c, uint8_t *d_frames, const uint64_t *d_off,
                         const uint16_t *d_len, uint64_t stride, uint32_t fixed_len,
                         uint64_t n, uint32_t max_len, void *stream) {
  if (!c || n > 0xffffffffull) return -EINVAL;
  if (n == 0) return 0;
  if (!d_frames || (!d_off && stride == 0 && n > 1) || (!d_len && fixed_len > 65535))
    return -EINVAL;
  DeviceScope dg(c->device);
  if (!dg.ok) return -EIO;
  pptk_rx_dev_batch b;
  memset(&b, 0, sizeof(b));
  b.d_frames = d_frames;
  b.d_off = d_off;
  b.d_len = d_len;
  b.stride = stride;
  b.fixed_len = fixed_len;
  b.max_len = max_len;
  b.n = n;
  uint32_t mmax = 15;
  if (!d_off) {
    const uint64_t p = (uint64_t)(uintptr_t)d_frames;
    const uint64_t gg = gcd64(stride % 16 ? stride % 16 : 16, 16);
    mmax = (uint32_t)((p % gg) + 16 - gg);
  }
  const uint32_t maxlen = d_len ? (max_len ? max_len : 65535u) : fixed_len;
  int variant = pick_variant(maxlen + mmax);
  const bool two_pass = !d_off;
  if (two_pass) {
    // the streaming pass of a two-pass batch moves what the receive
    // transform moves minus most of the writes: pptk_rx_autotune's choice
    // for this shape applies (T32S3D7 5.14 ms vs T16S6 5.30 on C1500,
    // DESIGN.md "Secondary kernels")
    const int tv = c->tuned[0][variant];
    if (tv >= 0 && tv != RX_L4) variant = tv;
  }
  const int fv = forced_variant(c);
  if (fv >= 0 && fv != RX_L4) variant = fv;   // the lane kernel has no tx mode
  RxKArgs a = batch_args(c, &b);
  a.frames_w = d_frames;
  c->last_variant = variant;
  a.tune = c->forced_flags >= 0 ? (uint32_t)c->forced_flags & kTuneMask
                                : pick_tune(c, variant, d_off || d_len) &
                                      ~(uint32_t)PPTK_RX_TUNE_NT_LOADS;
  hipStream_t s = (hipStream_t)stream;
  if (two_pass) {
    // Fixed-stride batches: the streaming pass writes nothing into the
    // frames (so it may use non-temporal loads, as the receive transform
    // does); the fields go to the context's side array and a second pass
    // writes them.  Offset-described batches keep the in-place stores:
    // their streaming pass is slower with non-temporal loads, and the
    // fields stored beside it cost less than the second pass.
    if (c->forced_flags < 0)
      a.tune = pick_tune(c, variant, false);
    uint64_t *side = c->d_txuser && c->txuser_n >= n ? c->d_txuser : nullptr;
    const bool pooled = side == nullptr;
    if (pooled) {   // stream-ordered: this call's own array, freed behind it
      hipMemPool_t pool;
      {
        // created once, by whichever tx call comes first (two threads'
        // first calls may race)
        std::lock_guard<std::mutex> g(c->txpool_mu);
        if (!c->txpool) {
          hipMemPoolProps pp;
          memset(&pp, 0, sizeof(pp));
          pp.allocType = hipMemAllocationTypePinned;
          pp.location.type = hipMemLocationTypeDevice;
          pp.location.id = c->device;
          hipMemPool_t np = nullptr;
          if (hipMemPoolCreate(&np, &pp) != hipSuccess) return -ENOMEM;
          uint64_t keep = UINT64_MAX;   // keep freed blocks for the next call
          (void)hipMemPoolSetAttribute(np, hipMemPoolAttrReleaseThreshold, &keep);
          c->txpool = np;
        }
        pool = c->txpool;
      }
      if (hipMallocFromPoolAsync((void **)&side, n * 8, pool, s) != hipSuccess)
        return -ENOMEM;
    }
    a.txside = side;
    hipError_t e = launch_rx(variant, a, grid_for(c, variant, n), s);
    if (e == hipSuccess) e = launch_tx_apply(side, d_frames, d_off, stride, n, s);
    if (pooled && hipFreeAsync(side, s) != hipSuccess && e == hipSuccess) e = hipErrorUnknown;
    return hip_rc(e);
  }
  return hip_rc(launch_rx(variant, a, grid_for(c, variant, n), s));
}

int pptk_tx_set_side_buffer(struct pptk_rx_ctx *c, void *d_side, uint64_t frames) {
  if (!c || (!d_side && frames) || ((uintptr_t)d_side & 7u)) return -EINVAL;
  DeviceScope dg(c->device);
  if (!dg.ok) return -EIO;
  c->d_txuser = (uint64_t *)d_side;
  c->txuser_n = d_side ? frames : 0;
  return 0;
}

int pptk_tx_rewrite_device(struct pptk_rx_ctx *c, uint8_t *d_frames, const uint64_t *d_off,
                           const uint16_t *d_len, uint64_t stride, uint32_t fixed_len,
                           uint64_t n, const struct pptk_rewrite *d_rw, uint64_t rw_count,
                           uint8_t *d_status, void *stream) {
  return pptk_tx_rewrite_flow_device(c, d_frames, d_off, d_len, stride, fixed_len, n, d_rw,
                                     rw_count, nullptr, d_status, stream);
}

int pptk_tx_rewrite_flow_device(struct pptk_rx_ctx *c, uint8_t *d_frames, const uint64_t *d_off,
                                const uint16_t *d_len, uint64_t stride, uint32_t fixed_len,
                                uint64_t n, const struct pptk_rewrite *d_rw, uint64_t rw_count,
                                const uint32_t *d_idx, uint8_t *d_status, void *stream) {
  const bool ok = d_rw && (d_idx ? rw_count != 0 && !((uintptr_t)d_idx & 3u)
                                 : rw_count == 1 || rw_count == n);
  return hdr_op(c, d_frames, d_off, d_len, stride, fixed_len, n, d_status, ok,
                [&](const HdrBatch &b, int grid) {
                  const RewriteKArgs a = {b, d_rw, !d_idx && rw_count == 1 ? 1u : 0u, d_idx,
                                          rw_count};
                  return launch_rewrite(a, grid, (hipStream_t)stream);
                });
}

int pptk_tcp_mss_clamp_device(struct pptk_rx_ctx *c, uint8_t *d_frames, const uint64_t *d_off,
                              const uint16_t *d_len, uint64_t stride, uint32_t fixed_len,
                              uint64_t n, uint16_t mss, uint32_t flags, uint8_t *d_status,
                              void *stream) {
  const bool ok = !(flags & ~PPTK_MSS_SYN_ONLY);
  return hdr_op(c, d_frames, d_off, d_len, stride, fixed_len, n, d_status, ok,
                [&](const HdrBatch &b, int grid) {
                  const MssKArgs a = {b, mss, flags};
                  return launch_mss_clamp(a, grid, (hipStream_t)stream);
                });
}

int pptk_tcp_seq_translate_device(struct pptk_rx_ctx *c, uint8_t *d_frames, const uint64_t *d_off,
                                  const uint16_t *d_len, uint64_t stride, uint32_t fixed_len,
                                  uint64_t n, const struct pptk_seqxlate *d_xl, uint64_t xl_count,
                                  const uint32_t *d_idx, uint8_t *d_status, void *stream) {
  const bool ok = d_xl && xl_count != 0 && (d_idx || xl_count == 1 || xl_count == n);
  return hdr_op(c, d_frames, d_off, d_len, stride, fixed_len, n, d_status, ok,
                [&](const HdrBatch &b, int grid) {
                  const SeqKArgs a = {b, d_xl, xl_count, d_idx, !d_idx && xl_count == 1 ? 1u : 0u};
                  return launch_seq_translate(a, grid, (hipStream_t)stream);
                });
}

// The length groups of the mixed path, as launch_bin takes them.
static_assert(kGroups == 3, "kBinBounds lists the bounds of groups 0 and 1");
static constexpr BinBounds kBinBounds = {{kGroupMaxLen[0], kGroupMaxLen[1]}};

int pptk_rx_batch_device_mixed(struct pptk_rx_ctx *c, const struct pptk_rx_dev_batch *b,
                               uint32_t *d_perm, void *d_scratch, void *stream) {
  int rc = check_batch(c, b);
  if (rc || b->n == 0) return rc;
  if (!b->d_len || !d_scratch) return -EINVAL;
  DeviceScope dg(c->device);
  if (!dg.ok) return -EIO;
  const hipStream_t s = (hipStream_t)stream;
  if (b->max_len && b->max_len <= kGroupMaxLen[kGroups - 2]) {
    // Every frame fits the 1536-byte shape (by the hint; a wrong hint costs
    // speed, never results): no length group is worth a launch of its own
    // (DESIGN.md "Binned order"), so batch order, as pptk_rx_batch_device.
    pptk_rx_dev_batch t = *b;
    t.d_perm = nullptr;
    if ((rc = pptk_rx_batch_device(c, &t, stream)) != 0) return rc;
    return d_perm ? hip_rc(launch_iota(d_perm, b->n, s)) : 0;
  }
  uint32_t *perm = d_perm ? d_perm : bin_perm(d_scratch, kBinGrid, b->n);
  // the binning also lays the descriptors out in binned order (scratch), so
  // the group launches stream them instead of gathering them through perm
  BinDesc bd{b->d_off, b->stride, bin_desc_off(d_scratch, kBinGrid),
             bin_desc_len(d_scratch, kBinGrid, b->n)};
  hipError_t e = launch_bin(b->d_len, b->n, perm, d_scratch, s, kBinGrid, bd, kBinBounds, true);
  if (e != hipSuccess) return -EIO;
  RxKArgs a = batch_args(c, b);
  a.perm = perm;
  a.off = bd.boff;
  a.len = bd.blen;
  a.by_pos = 1;
  const uint32_t *tab = bin_table(d_scratch, kBinGrid);
  a.plan = tab + kGroups + 1;
  a.off0 = b->d_off;
  a.len0 = b->d_len;
  const uint32_t maxlen = b->max_len ? b->max_len : 65535u;
  const int fv = forced_variant(c);
  for (int g = 0; g < kGroups; ++g) {
    // the group holding max_len also takes every group above it (all empty
    // when the hint is right; a wrong hint costs speed, never results)
    const bool last = kGroupMaxLen[g] >= maxlen;
    int variant = fv >= 0 && fv != RX_L4 ? fv : kGroupVariant[g];
    // (a launch may run the whole batch when it is not binned:
    // pptk_rx_autotune's choice for its shape applies, as in batch order)
    if (fv < 0 && c->tuned[1][variant] >= 0 && c->tuned[1][variant] != RX_L4)
      variant = c->tuned[1][variant];
    a.plan_group = (uint32_t)g;
    a.range_lo = tab + g;
    a.range_hi = tab + (last ? kGroups : g + 1);
    a.tune = pick_tune(c, variant, true);
    e = launch_rx(variant, a, grid_for(c, variant, b->n), s);
    if (e != hipSuccess) return -EIO;
    if (last) break;
  }
  return 0;
}

int pptk_rx_set_tuning(struct pptk_rx_ctx *c, int variant, int flags) {
  if (!c || variant < -1 || variant >= RX_NVARIANTS || flags < -1) return -EINVAL;
  if (flags >= 0 && ((uint32_t)flags & ~kTuneMask)) return -EINVAL;
  c->forced_variant = variant;
  // the rate limiter's bit is its own switch: flags that hold nothing else
  // leave the receive transform's memory policy automatic
  const int rx = flags < 0 ? -1 : flags & ~PPTK_RX_TUNE_PERMIT_PASSES;
  c->forced_flags = flags >= 0 && rx == 0 && (flags & PPTK_RX_TUNE_PERMIT_PASSES) ? -1 : rx;
  c->permit_passes = flags >= 0 && (flags & PPTK_RX_TUNE_PERMIT_PASSES);
  return 0;
}

// CU-mask bit i names CU i / nxcc of XCC i % nxcc, and CU k of an XCC sits
// in shader engine k % 4 (tools/cumask_map.py, profiles/r05 row aj): the
// top coll_cus bits are coll_cus / nxcc CUs of every XCC, the same number
// in each of its four SEs when that is a multiple of 4.  Each workgroup goes
// to an XCC and SE in turn, so a mask that leaves one SE short of another
// overfills it and the persistent grid runs a tail (-EINVAL below).
static constexpr int kSePerXcc = 4;

int pptk_rx_stream_split(struct pptk_rx_ctx *c, int coll_cus, void **rx_stream,
                         void **coll_stream) {
  if (!c || coll_cus < 0) return -EINVAL;
  if (coll_cus == 0) {   // the whole chip for the grids again; the streams stay the context's
    if (rx_stream) *rx_stream = nullptr;
    if (coll_stream) *coll_stream = nullptr;
    c->coll_cus = 0;
    return 0;
  }
  if (!rx_stream || !coll_stream) return -EINVAL;
  *rx_stream = *coll_stream = nullptr;
  if (c->split_coll && c->split_cus == coll_cus) {   // the pair the context holds
    *rx_stream = c->split_rx;
    *coll_stream = c->split_coll;
    c->coll_cus = coll_cus;
    return 0;
  }
  // A new pair: the communicator's channel cap (ncclConfig_t.maxCTAs, fixed
  // when it is created) follows the collective stream's CUs, so that stream
  // cannot change under a communicator -- or a creation in progress.
  if (ctx_comm_slot(c)->load(std::memory_order_acquire) != nullptr) return -EBUSY;
  DeviceScope dg(c->device);
  if (!dg.ok) return -EIO;
  int nxcc = 1;
  if (hipDeviceGetAttribute(&nxcc, hipDeviceAttributeNumberOfXccs, c->device) != hipSuccess ||
      nxcc < 1)
    nxcc = 1;
  if (coll_cus % (nxcc * kSePerXcc) || coll_cus >= c->ncu || c->ncu % nxcc) return -EINVAL;
  std::vector<uint32_t> rx((c->ncu + 31) / 32, 0), coll(rx.size(), 0);
  for (int i = 0; i < c->ncu; ++i) (i >= c->ncu - coll_cus ? coll : rx)[i / 32] |= 1u << (i % 32);
  hipStream_t a = nullptr, b = nullptr;
  if (hipExtStreamCreateWithCUMask(&a, (uint32_t)rx.size(), rx.data()) != hipSuccess) return -EIO;
  if (hipExtStreamCreateWithCUMask(&b, (uint32_t)coll.size(), coll.data()) != hipSuccess) {
    (void)hipStreamDestroy(a);
    return -EIO;
  }
  drop_split_streams(c);   // a pair of another CU count, no communicator since
  {
    std::lock_guard<std::mutex> g(g_split_mu);
    g_split_owned[a] = c;
    g_split_owned[b] = c;
    g_split_retired.erase(a);
    g_split_retired.erase(b);
  }
  c->split_rx = a;
  c->split_coll = b;
  c->split_cus = coll_cus;
  *rx_stream = a;
  *coll_stream = b;
  c->coll_cus = coll_cus;
  return 0;
}

int pptk_rx_stream_destroy(void *stream) {
  if (!stream) return -EINVAL;
  const hipStream_t s = (hipStream_t)stream;
  {
    std::lock_guard<std::mutex> g(g_split_mu);
    if (g_split_owned.count(s)) return -EBUSY;   // its context destroys it
    if (g_split_retired.erase(s)) return 0;      // its context already did
  }
  return hip_rc(hipStreamDestroy(s));
}

int pptk_rx_variant_count(void) { return RX_NVARIANTS; }

int pptk_rx_last_variant(const struct pptk_rx_ctx *c) { return c ? c->last_variant : -1; }

size_t pptk_rx_permit_scratch_bytes(uint64_t n, uint32_t hash_size) {
  if (hash_size == 0 || (hash_size & (hash_size - 1)) || n > 0xffffffffull) return 0;
  return permit_scratch_bytes(n, hash_size);
}

static int permit_common(struct pptk_rx_ctx *c, const struct pptk_rx_rec *d_recs,
                         const struct pptk_rx_rec32 *d_recs32, const uint32_t *d_keys,
                         uint64_t n, int family, const uint8_t *d_subject, uint32_t *d_tokens,
                         uint8_t *d_verdict, void *d_scratch, void *stream) {
  if (!c || (family != 4 && family != 6) || n > 0xffffffffull) return -EINVAL;
  if ((family == 4 && !c->opts.iphash_bits4) || (family == 6 && !c->opts.iphash_bits6))
    return -EINVAL;   // the records carry no bucket for that family
  const uint32_t hs = c->opts.iphash_size;
  if (hs == 0 || (hs & (hs - 1))) return -EINVAL;
  if (n == 0) return 0;
  if ((!d_recs && !d_recs32 && !d_keys) || !d_tokens || !d_verdict || !d_scratch) return -EINVAL;
  DeviceScope dg(c->device);
  if (!dg.ok) return -EIO;
  PermitArgs a{};
  a.recs = d_recs32 || d_keys ? nullptr : d_recs;
  a.recs32 = d_keys ? nullptr : d_recs32;
  a.keys_in = d_keys;
  a.n = n;
  a.subject = d_subject;
  a.tokens = d_tokens;
  a.verdict = d_verdict;
  a.hash_size = hs;
  a.family = family;
  // the fused kernel's workgroups must all be resident at once (grid
  // barriers): no more than the CUs a split leaves the batches' stream
  a.ncu = c->ncu - c->coll_cus;
  a.force_passes =
      c->permit_passes || (env_tune() >= 0 && (env_tune() & PPTK_RX_TUNE_PERMIT_PASSES)) ? 1 : 0;
  return hip_rc(launch_permit(a, d_scratch, (hipStream_t)stream));
}

int pptk_rx_permit_status(struct pptk_rx_ctx *c, const void *d_scratch, void *stream) {
  if (!c || !d_scratch) return -EINVAL;
  DeviceScope dg(c->device);
  if (!dg.ok) return -EIO;
  return permit_status(d_scratch, (hipStream_t)stream);
}

int pptk_rx_permit_device(struct pptk_rx_ctx *c, const struct pptk_rx_rec *d_recs,
                          const struct pptk_rx_rec32 *d_recs32, uint64_t n, int family,
                          const uint8_t *d_subject, uint32_t *d_tokens, uint8_t *d_verdict,
                          void *d_scratch, void *stream) {
  if (!d_recs && !d_recs32) return -EINVAL;
  return permit_common(c, d_recs, d_recs32, nullptr, n, family, d_subject, d_tokens, d_verdict,
                       d_scratch, stream);
}

int pptk_rx_permit_keys_device(struct pptk_rx_ctx *c, const uint32_t *d_keys, uint64_t n,
                               int family, const uint8_t *d_subject, uint32_t *d_tokens,
                               uint8_t *d_verdict, void *d_scratch, void *stream) {
  if (!d_keys && n) return -EINVAL;
  return permit_common(c, nullptr, nullptr, d_keys, n, family, d_subject, d_tokens, d_verdict,
                       d_scratch, stream);
}

int pptk_rx_tokens_refill_device(struct pptk_rx_ctx *c, uint32_t *d_tokens, uint32_t start,
                                 uint32_t end, uint32_t add, uint32_t initial_tokens,
                                 void *stream) {
  if (!c || !d_tokens || start > end || end > c->opts.iphash_size) return -EINVAL;
  DeviceScope dg(c->device);
  if (!dg.ok) return -EIO;
  return hip_rc(launch_refill(d_tokens, start, end, add, initial_tokens, (hipStream_t)stream));
}

size_t pptk_rx_bin_scratch_bytes(uint64_t n) { return bin_scratch_bytes(n, kBinGrid); }

int pptk_rx_bin_device(struct pptk_rx_ctx *c, const uint16_t *d_len, uint64_t n,
                       uint32_t *d_perm, void *d_scratch, void *stream) {
  if (!c || (n && (!d_len || !d_perm || !d_scratch))) return -EINVAL;
  if (n > 0xffffffffull) return -EINVAL;
  DeviceScope dg(c->device);
  if (!dg.ok) return -EIO;
  return hip_rc(launch_bin(d_len, n, d_perm, d_scratch, (hipStream_t)stream, kBinGrid,
                            BinDesc{nullptr, 0, nullptr, nullptr}, kBinBounds, false));
}

}  // extern "C"
