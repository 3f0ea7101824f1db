// chist_kernel.h — the client-side op history of every protocol.
//
// Paxi's benchmark appends operation{input, output, start, end} to the client's
// History for every completed request (benchmark.go:246-275).  Here worker w of
// a cluster records an op exactly where a latency sample is taken: in
// client_reply, after the duplicate check, in the recording units only
// (PXS_LAT = 1) and behind the wave-uniform Params::ch_cap.
//
// The hook is one 16-byte store {cid, reply value, start, end} and one count
// update.  start is the worker's issue stamp (lat_kernel.h), end the step of
// the accepted reply.  The key and kind of the op are functions of (cluster,
// cid) (sim_core.h wl_key / wl_write) and are derived where the history is
// read - chist_op below, used by the checker's two staging passes (lin_kernel.h)
// and by the host readout - so the key draw stays out of the handler.  A record
// whose first word has bit 31 set is literal, {1 << 31 | is_write << 30 | key,
// value, start, end}: what paxisim_client_history_load writes (cids are at
// most CMD_MASK, so the bit is free).
//
// Layout: ops [WK][C][cap] uint4, counts [WK][C] u32 (C: the cluster lanes, the
// clusters rounded up to whole tiles) - ABD's [source][C][H] with the workers
// as sources.  Both are indexed by the local
// cluster id (gid - cluster_base), never by the slot, as the agreement ring is:
// compaction and wake move nothing.  A count keeps counting past cap; the ops
// past cap are not recorded and the readout reports them as dropped.  No flag
// is raised, so replica state, stats and flags are those of a run without it.
//
// Only replica target[w] ever answers worker w (client_reply runs in the wave
// of the replica the request reached), and a lane is one cluster, so one
// thread owns a (worker, cluster) row: the count is a plain load and store,
// also in the barrier kernel, where the replicas of a cluster are the waves of
// one workgroup.
#pragma once
#include "paxisim_dev.h"

namespace pxs {

// sim_core.h: the workload's draws of command cid given h = wl_hash(kc, cid)
__device__ __forceinline__ uint32_t wl_hash(uint32_t kc, uint32_t cid);
__device__ __forceinline__ uint32_t wl_key_h(const Params& P, uint32_t h, uint32_t cid);
__device__ __forceinline__ bool wl_write_h(const Params& P, uint32_t h);

constexpr uint32_t CH_LITERAL = 1u << 31, CH_WRITE = 1u << 30;

__host__ __device__ inline size_t chist_row(const Params& P, uint32_t w, uint64_t cl) {
  return (size_t)w * P.C + cl;
}

// An accepted reply for worker w of local cluster cl (slot c) at step t.
__device__ __forceinline__ void chist_record(const Params& P, uint32_t w, uint64_t cl, uint64_t c, uint32_t cid,
                                             uint32_t value, uint32_t t) {
  const size_t row = chist_row(P, w, cl);
  const uint32_t n = P.ch_cnt[row];
  P.ch_cnt[row] = n + 1u;
  if (n < P.ch_cap) P.ch_ops[row * P.ch_cap + n] = make_uint4(cid, value, P.lat_stamp[(size_t)w * P.C + c], t);
}

// The key word of a record in the checker's form, key | write << 31, for the
// cluster whose PRNG key is kc.  The key is the index every replica executes
// the command on: a draw beyond the key space is the last index (key_fit).
__device__ __forceinline__ uint32_t chist_key(const Params& P, uint32_t kc, uint32_t x) {
  if (x & CH_LITERAL) return (x & ~(CH_LITERAL | CH_WRITE)) | ((x & CH_WRITE) << 1);
  const uint32_t h = wl_hash(kc, x);
  uint32_t k = wl_key_h(P, h, x);
  if (k >= P.keys) k = P.keys - 1u;
  return k | (wl_write_h(P, h) ? 1u << 31 : 0u);
}
// A record as the op {key | write << 31, value, start, end}: a write's value is
// its command id (op.input), a read's the reply's (op.output, 0 = nil).
__device__ __forceinline__ uint4 chist_op(const Params& P, uint32_t kc, uint4 o) {
  const uint32_t kw = chist_key(P, kc, o.x);
  if (!(o.x & CH_LITERAL) && (kw >> 31)) o.y = o.x;
  o.x = kw;
  return o;
}

// The checker's history source (lin_kernel.h LinAbd is the other): the workers
// of a cluster in index order, each worker's ops in completion order.
struct LinClient {
  static constexpr uint32_t MAX_SRC = PAXISIM_MAX_WORKERS;
  __host__ __device__ static uint32_t sources(const Params& P) { return P.WK; }
  __host__ __device__ static uint32_t per_source(const Params& P) { return P.ch_cap; }
  __device__ static uint32_t ctx(const Params& P, uint64_t c) { return P.kc[P.slot_of[c]]; }
  __device__ static uint32_t len(const Params& P, uint32_t s, uint64_t c) {
    const uint32_t n = P.ch_cnt[chist_row(P, s, c)];
    return n < P.ch_cap ? n : P.ch_cap;
  }
  __device__ static const uint4* at(const Params& P, uint32_t s, uint64_t c, uint32_t idx) {
    return &P.ch_ops[chist_row(P, s, c) * P.ch_cap + idx];
  }
  __device__ static uint32_t key(const Params& P, uint32_t kc, uint32_t x) { return chist_key(P, kc, x) & 0x7FFFFFFFu; }
  __device__ static uint4 op(const Params& P, uint32_t kc, const uint4& o) { return chist_op(P, kc, o); }
};

// Readout of one cluster (not part of the step): out[w * cap + j] is op j of
// worker w in the checker's form, cnt[w] the worker's count (past cap: dropped).
// One definition: the unit that launches it (host_check.hip) asks for it.
#ifdef PXS_CHIST_READ
__global__ void chist_read_kernel(Params P, uint64_t cl, uint4* out, uint32_t* cnt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P.WK * P.ch_cap) return;
  const uint32_t w = i / P.ch_cap, j = i - w * P.ch_cap;
  const uint32_t n = P.ch_cnt[chist_row(P, w, cl)];
  if (j == 0) cnt[w] = n;
  if (j < n) out[i] = chist_op(P, LinClient::ctx(P, cl), *LinClient::at(P, w, cl, j));
}
#endif

}  // namespace pxs
