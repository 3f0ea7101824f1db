// lat_kernel.h — client request latency on the device.
//
// A closed-loop worker has one request in flight, so its latency in virtual
// steps is the step of the accepted reply minus the step of the issue.  The
// issue step of worker w of the cluster in slot c is the stamp
// Params::lat_stamp[w][c] (laid out like wrep; compaction moves its rows with
// the slot), written wherever a worker issues (client_reply's next request,
// client_start; create time is step 0 = the zeroed array).  client_reply takes
// a sample after its duplicate check and adds it to the per-worker accumulator
// row {bins one-step counts, overflow count, sum, UINT32_MAX - min, max}, all
// u64 and all zero when empty, so a reset is a memset.
//
// Clusters run in lockstep, so the lanes of a wave mostly hold the same
// (worker, latency): the wave first folds its samples by distinct key
// (readfirstlane of the key, ballot of the lanes that match) and one lane
// issues the atomics of each distinct key with the popcount.  Only the lanes
// inside the caller's branch that hold a sample take part: the ballot and the
// readfirstlane see the active lanes alone, and a lane leaves the loop as
// soon as its key has been served.  The target is one of LAT_SLICES copies,
// chosen by the tile (in the pipelined kernel a tile's XCD), folded at readout
// by lat_reduce.
#pragma once
#include "paxisim_dev.h"

namespace pxs {

constexpr uint32_t LAT_SLICES = 8;   // a power of two
constexpr uint32_t LAT_EXTRA = 4;    // after the bins: overflow, sum, UINT32_MAX - min, max
enum { LAT_OVF = 0, LAT_SUM, LAT_NMIN, LAT_MAX };

__host__ __device__ inline size_t lat_row(uint32_t bins) { return (size_t)bins + LAT_EXTRA; }

// Worker w's request issued at step t by the cluster of lane slot c.
__device__ __forceinline__ void lat_issue(const Params& P, uint32_t w, uint64_t c, uint32_t t) {
  P.lat_stamp[(size_t)w * P.C + c] = t;
}

// An accepted reply for worker w at step t: every active lane holds a sample.
__device__ __forceinline__ void lat_sample(const Params& P, uint32_t blk, uint32_t lane, uint32_t w, uint64_t c,
                                           uint32_t t) {
  const uint32_t lat = t - P.lat_stamp[(size_t)w * P.C + c];
  const uint32_t bins = P.lat_bins;
  unsigned long long* acc = P.lat_acc + (size_t)(blk & (LAT_SLICES - 1u)) * P.WK * lat_row(bins);
  for (;;) {
    const uint32_t w0 = __builtin_amdgcn_readfirstlane(w);
    const uint32_t l0 = __builtin_amdgcn_readfirstlane(lat);
    const bool mine = w == w0 && lat == l0;
    const uint64_t m = __ballot(mine);        // the active lanes with the first lane's key
    if (mine) {
      if (lane == (uint32_t)__ffsll((unsigned long long)m) - 1u) {
        const unsigned long long n = (unsigned long long)__popcll(m);
        unsigned long long* row = acc + (size_t)w0 * lat_row(bins);
        atomicAdd(&row[l0 < bins ? l0 : bins + LAT_OVF], n);
        atomicAdd(&row[bins + LAT_SUM], n * l0);
        atomicMax(&row[bins + LAT_NMIN], (unsigned long long)(0xFFFFFFFFu - l0));
        atomicMax(&row[bins + LAT_MAX], (unsigned long long)l0);
      }
      break;
    }
  }
}

// Readout: fold the slices into out[WK][bins + LAT_EXTRA] (not part of the step).
// One definition: the unit that launches it (host_check.hip) asks for it.
#ifdef PXS_LAT_REDUCE
__global__ void lat_reduce(Params P, unsigned long long* out) {
  const size_t n = (size_t)P.WK * lat_row(P.lat_bins);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const uint32_t k = (uint32_t)(i % lat_row(P.lat_bins));
    const bool mx = k >= P.lat_bins + LAT_NMIN;
    unsigned long long v = 0;
    for (uint32_t s = 0; s < LAT_SLICES; s++) {
      const unsigned long long a = P.lat_acc[s * n + i];
      v = mx ? (a > v ? a : v) : v + a;
    }
    out[i] = v;
  }
}
#endif

}  // namespace pxs
