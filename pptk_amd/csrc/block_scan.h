// block_scan.h -- the device helpers of the three-step prefix sum by which the
// batch ops place a variable-size output (rx_flowlearn.hip, ip_reass.hip,
// tx_dispatch.hip, tx_frag.hip): workgroups count, one workgroup turns the
// block counts into exclusive prefixes, a last pass adds the prefix back.
// Nothing here waits for another workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pptk {

// inclusive prefix of x over the wave's 64 lanes
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T x, uint32_t lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T y = __shfl_up(x, d);
    if ((int)lane >= d) x += y;
  }
  return x;
}

// exclusive prefix of v over the workgroup's NW waves and the workgroup's total
template <int NW, typename T>
__device__ __forceinline__ T block_excl_scan(T v, T *lds, T *total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const T incl = wave_incl_scan<T>(v, lane);
  if (lane == 63) lds[wave] = incl;
  __syncthreads();
  T base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const T t = lds[w];
    if ((uint32_t)w < wave) base += t;
    tot += t;
  }
  __syncthreads();   // lds is free for the next round
  *total = tot;
  return base + incl - v;
}

// how many counts a scan covers: nb, or where `items` is given
// ceil(*items / per) if that is smaller
__device__ __forceinline__ uint32_t scan_extent(uint32_t nb, const uint64_t *items, uint32_t per) {
  if (items) {
    const uint64_t q = (*items + per - 1) / per;
    if (q < nb) nb = (uint32_t)q;
  }
  return nb;
}

// a count an earlier pass left in device memory, clamped by the bound the
// arrays were sized for
__device__ __forceinline__ uint32_t clamped_count(const uint64_t *count, uint32_t maxc) {
  const uint64_t c = *count;
  return c < maxc ? (uint32_t)c : maxc;
}

// One workgroup of NT threads: the sum of cnt[0 .. nb), and where asked their
// exclusive prefixes in place, NT counts per round.  T holds the sums of one
// round; the prefixes are stored as 32-bit words, so the caller bounds them.
template <int NT, typename T>
__device__ __forceinline__ uint64_t scan_counts(uint32_t *cnt, uint32_t nb, bool write_prefixes,
                                                T *lds) {
  uint64_t running = 0;
  for (uint32_t base = 0; base < nb; base += NT) {
    const uint32_t k = base + threadIdx.x;
    const T v = k < nb ? cnt[k] : 0u;
    T total;
    const T ex = block_excl_scan<NT / 64, T>(v, lds, &total);
    if (write_prefixes && k < nb) cnt[k] = (uint32_t)running + (uint32_t)ex;
    running += total;
  }
  return running;
}

}  // namespace pptk
