// mv_kernel.h — the multi-version Database and the Consensus scan over it
// (DESIGN.md §3.14, §5.15).
//
// Paxi's Database under config.MultiVersion appends every written value to
// history[key] (db.go:123-134 put), History(key) returns it (db.go:151-155) and
// HTTPClient.Consensus(k) (client.go:279-320) collects every replica's
// History(k) and requires that, index by index, the values present form a set
// of at most one.  Here replica r of a cluster keeps, per key, the count of
// values it ever put and the first mv_cap of them; a write's value is its
// command id, as in kv_val.
//
// The hook is mv_put, called from kv_exec (paxos_kernel.h) after the write
// test, in the recording units only (PXS_LAT = 1) and behind the wave-uniform
// Params::mv_cap: Multi-Paxos, the per-key protocols (paxos_exec) and EPaxos
// (epaxos_kernel.h) all execute through kv_exec, so an EPaxos re-execution
// appends again, as the reference's put does.  One count load and store and one
// 4-byte value store per executed write.
//
// Layout: values [K][N][C][mv_cap] u32, counts [K][N][C] u32 (C: the cluster
// lanes).  A row is contiguous, so a readout is one copy and the scan reads
// along it, 32 versions to a 128-B line.  Both are indexed by the local cluster
// id (gid - cluster_base), never by the slot, as the client history and the
// agreement ring are: compaction, freeze and wake move nothing.  A count keeps
// counting past mv_cap; the values past it are not kept and the readouts report
// them as dropped.  No flag is raised, so replica state, stats and flags are
// those of a run without it.
//
// A lane is one cluster and replica r's wave (or its turn in the serial kernel)
// is the only writer of the rows (., r, cluster), so the count is a plain load
// and store, also in the barrier kernel (chist_kernel.h makes the same
// argument for a worker's row).
#pragma once
#include "paxisim_dev.h"

namespace pxs {

__host__ __device__ inline size_t mv_row(const Params& P, uint32_t key, uint32_t r, uint64_t cl) {
  return ((size_t)key * SH_N(P) + r) * P.C + cl;
}

// Replica r of local cluster cl puts value v to key (db.go:123-134).
__device__ __forceinline__ void mv_put(const Params& P, uint32_t key, uint32_t r, uint64_t cl, uint32_t v) {
  const size_t row = mv_row(P, key, r, cl);
  const uint32_t n = P.mv_cnt[row];
  P.mv_cnt[row] = n + 1u;
  if (n < P.mv_cap) P.mv_val[row * P.mv_cap + n] = v;
}

// The Consensus scan (not part of the step).  One definition: the unit that
// launches it (host_check.hip) asks for it.
#ifdef PXS_MV_SCAN
constexpr uint32_t MV_WAVES = 4;        // waves per workgroup
enum { MV_FAILED = 0, MV_VERSIONS, MV_DROPPED, MV_NOUT };

// One wave per (cluster, key) pair of clusters [c0, c0 + nc), pairs dealt to the
// waves grid-stride, key-major: neighbouring waves read neighbouring clusters'
// counts.  Lane r holds replica r's count.  Lanes take the indices i of a chunk
// of 64 up to min(mv_cap, max_r n_r): for each replica in index order whose kept
// prefix reaches i, its value at i is compared with the first such replica's
// (client.go:302-319: the set of the values present has at most one member), and
// a ballot gives the pair's verdict.  Nothing is read beyond min(n_r, mv_cap).
// out: MV_FAILED pairs, the sum of n_r and of max(0, n_r - mv_cap), a wave's
// totals added once; masks (may be null): [nc] the failing keys of each cluster.
__global__ void __launch_bounds__(MV_WAVES * 64) mv_consensus_kernel(Params P, uint64_t c0, uint64_t nc,
                                                                     unsigned long long* out,
                                                                     unsigned long long* masks) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * MV_WAVES + (threadIdx.x >> 6);
  const uint64_t waves = (uint64_t)gridDim.x * MV_WAVES, pairs = nc * P.keys;
  const uint32_t H = P.mv_cap;
  unsigned long long failed = 0, versions = 0, dropped = 0;
  for (uint64_t p = wave; p < pairs; p += waves) {
    const uint32_t key = (uint32_t)(p / nc);
    const uint64_t cl = c0 + (p - (uint64_t)key * nc);
    const uint32_t n = lane < SH_N(P) ? P.mv_cnt[mv_row(P, key, lane, cl)] : 0u;
    const uint32_t kept = n < H ? n : H;
    uint32_t top = 0;
    for (uint32_t r = 0; r < SH_N(P); r++) {
      const uint32_t nr = __shfl(n, (int)r, 64), kr = __shfl(kept, (int)r, 64);
      versions += nr;
      dropped += nr - kr;
      top = kr > top ? kr : top;
    }
    bool bad = false;
    for (uint32_t i0 = 0; i0 < top && !bad; i0 += 64u) {
      const uint32_t i = i0 + lane;
      // every replica's load is issued before the first value is compared: the rows are
      // independent streams, and a wave that waited for each in turn would pay N latencies
      // per chunk.  Lanes N.. hold kept = 0, so the replicas beyond N load nothing.
      uint32_t v[PAXISIM_MAX_N], in = 0;
#pragma unroll
      for (uint32_t r = 0; r < PAXISIM_MAX_N; r++) {
        const uint32_t kr = (uint32_t)__builtin_amdgcn_readlane((int)kept, (int)r);
        v[r] = 0;
        if (i < kr) {
          v[r] = P.mv_val[mv_row(P, key, r, cl) * H + i];
          in |= 1u << r;
        }
      }
      uint32_t first = 0;
      bool have = false, differs = false;
#pragma unroll
      for (uint32_t r = 0; r < PAXISIM_MAX_N; r++) {
        if (!((in >> r) & 1u)) continue;
        if (!have) {
          first = v[r];
          have = true;
        } else if (v[r] != first) {
          differs = true;
        }
      }
      bad = __ballot(differs) != 0ull;
    }
    if (bad) {
      failed++;
      if (masks && lane == 0) atomicOr(&masks[cl - c0], 1ull << key);
    }
  }
  if (lane == 0) {      // the three totals are wave-uniform
    if (failed) atomicAdd(&out[MV_FAILED], failed);
    if (versions) atomicAdd(&out[MV_VERSIONS], versions);
    if (dropped) atomicAdd(&out[MV_DROPPED], dropped);
  }
}
#endif

}  // namespace pxs
