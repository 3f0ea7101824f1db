// trace_kernel.h — message traces of chosen clusters, recorded on the device
// (DESIGN.md §3.15, §5.17).
//
// A Paxi deployment's message trace is what every replica's transport delivers,
// link by link (transport.go:146-165, socket.go:111-118 Recv).  Here the trace
// of replica r of a traced cluster is what r's inbox holds when its step t
// begins: per source 0..N-1 and then the client queue (src = N), the records in
// FIFO order - exactly what paxisim_read_inbox returns just before step t.
//
// The hook is trace_inbox, called where a replica-step reads its per-source
// counts (sim_core.h replica_step): after client_start, so a late
// worker's first request is in the box, and before a crashed replica's discard
// loop zeroes the counts, so the records socket.Recv throws away are in the
// trace.  It runs before Proto::dispatch, so one site per loop form covers every
// protocol.  It exists in the recording units only (PXS_LAT = 1), behind the
// wave-uniform Params::tr_cap and step window; a poisoned or frozen cluster runs
// no replica-step, so nothing is recorded for it.
//
// Layout: slots [row][N][tr_cap] of 32 B, {step, src, 0, 0} and the 16-byte
// mailbox record verbatim, written with two 16-byte stores; counts [row][N] u32.
// The row of a cluster comes from tr_row, a table indexed by the local cluster
// id (gid - cluster_base), never by the slot: compaction, freeze, wake and the
// two pools move nothing.  The table is read once per replica-step of a step
// inside the window, not per message.  A count keeps counting past tr_cap; the
// records past it are not kept and the readout reports them as dropped.  No flag
// is raised and no replica state is touched.
//
// A lane is one cluster and replica r's wave (or its turn in the serial kernel)
// is the only writer of the row (cluster, r), so the count is a plain load and
// store, also in the barrier kernel (mv_kernel.h makes the same argument).
#pragma once
#include "paxisim_dev.h"

namespace pxs {

constexpr uint32_t TR_NONE = 0xFFFFFFFFu;   // tr_row: the cluster is not traced

__host__ __device__ inline size_t trace_row(const Params& P, uint32_t row, uint32_t r) {
  return (size_t)row * SH_N(P) + r;
}

// Replica r of local cluster cl begins step t with the inbox boxes box0 + s, s < NS.
__device__ __forceinline__ void trace_inbox(const Params& P, uint64_t cl, uint32_t r, uint32_t t, uint32_t lane,
                                            const uint8_t* l_cnt, const uint4* rec, uint32_t box0, uint32_t NS) {
  if (t < P.tr_from || t >= P.tr_to) return;         // wave-uniform
  const uint32_t row = P.tr_row[cl];
  if (row == TR_NONE) return;
  const size_t ri = trace_row(P, row, r);
  const uint32_t n0 = P.tr_cnt[ri];
  uint32_t n = n0;
  for (uint32_t s = 0; s < NS; s++) {
    const uint32_t kn = l_cnt[((box0 + s) << 6) | lane];
    for (uint32_t k = 0; k < kn; k++, n++) {
      if (n >= P.tr_cap) continue;                   // counted, not kept
      uint4* o = &P.tr_rec[(ri * P.tr_cap + n) * 2u];
      o[0] = make_uint4(t, s, 0u, 0u);
      o[1] = rec[(((box0 + s) * P.M + k) << 6) | lane];
    }
  }
  if (n != n0) P.tr_cnt[ri] = n;
}

}  // namespace pxs
