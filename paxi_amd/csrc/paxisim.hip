// paxisim.hip — C-ABI (include/paxisim.h) over the gfx950 simulation kernels.
//
// Product path: everything here runs on the GPU.  There is no CPU fallback;
// a handle whose device cannot be initialised fails paxisim_create with
// PAXISIM_EDEVICE.
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <new>
#include <type_traits>
#include <utility>
#include <algorithm>
#include <vector>

#define PXS_LAT_REDUCE   // this unit defines and launches lat_reduce (lat_kernel.h)
#define PXS_CHIST_READ   // and chist_read_kernel (chist_kernel.h)
#define PXS_MV_SCAN      // and mv_consensus_kernel (mv_kernel.h)
#include "epaxos_kernel.h"
#include "lin_kernel.h"
#include "paxisim_dev.h"
#include "sim_core.h"
#include "create_plan.h"
#include "pool_plan.h"
#include "shape_plan.h"
#include "snapshot_kernel.h"
#include "snapshot_plan.h"
#include "step_ops.h"
#include "verdict_kernel.h"
#include "../../include/paxisim_shape.h"

using namespace pxs;

static_assert(PLAN_EP_NMAX == EP_NMAX, "create_plan.h check_config: the EPaxos replica limit");
#define HIPCHK(expr)                                                                  \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess)                                                             \
      return fail(PAXISIM_EDEVICE, "%s failed: %s", #expr, hipGetErrorString(e_));    \
  } while (0)

// A cluster pool: a slot region that is stepped, compacted and phase-binned on
// its own stream.  Swaps never cross regions; slot_of / cl_of and every array stay global.
struct Pool {
  uint32_t base = 0, end = 0;      // slots [base, end); base a multiple of 512
  uint32_t* d_cmp = nullptr;       // [0] bound (absolute), [1] lnew, [2] npairs, [3] live, [4] live before lnew, then block sums
  uint32_t* d_pairs = nullptr;     // [2][C/2+64]: dead slots below lnew, live slots above it
  uint32_t* d_ph = nullptr;        // phase binning: class counts, region, per-block sums
  uint32_t* d_pipe = nullptr;      // [0,8) tickets, [8] error, [16, 16 + max(C/64, 64)) chunks done per tile
  hipStream_t stream = nullptr;    // one pool: the handle's stream
  hipEvent_t ev = nullptr;         // join: the pool's work so far (two pools only)
  uint32_t last_cmp = 0;
};

struct paxisim {
  paxisim_config cfg;
  paxisim_workload wl;
  paxisim_fault_process fp;
  Params P;
  uint32_t zone_of[PAXISIM_MAX_N], node_of[PAXISIM_MAX_N];
  std::vector<DevFault> faults;
  DevFault* d_faults = nullptr;
  uint32_t* d_move = nullptr;      // moving-Mu key CDF tables (paxisim_workload.move_cdf)
  void* arena = nullptr;
  size_t arena_bytes = 0;
  uint64_t* d_scratch = nullptr;   // reductions
  hipStream_t stream = nullptr;
  StepOps ops{};
  int lds_set = -1;                // dynamic-LDS ceiling set for ops on this handle's device
  // the fixed-shape unit (k_paxos5f.hip): shape_fit: the handle has the shape in every
  // field but the scripted-fault count, the one pinned field that changes after create; fixed: ops is that unit's
  bool shape_fit = false, fixed = false;
  uint32_t t = 0;
  uint32_t S = 32;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> evs;
  double kernel_ms = 0;
  uint64_t launches = 0;
  // live-cluster compaction: per pool, the scratch in Pool
  uint32_t cmp_every = 50;         // steps between compactions
  // pipelined serial launches (sim_core.h sim_serial_pipe): up to pipe_max chunks of S steps per launch
  uint32_t pipe_max = 4;
  uint32_t pipe_slots = 0;         // PAXISIM_PIPE_SLOTS: cap on the persistent grid (0: none)
  // cluster pools: pool[0] alone steps on `stream`; two pools step on streams of their own, and
  // everything that is not a step stays on `stream` behind a join (join_pools)
  Pool pool[MAX_POOLS];
  uint32_t npools = 1;
  hipEvent_t ev_main = nullptr;    // join: the handle's stream so far
  bool pools_ahead = false;        // steps were launched since the last join
  bool main_ahead = false;         // the handle's stream was used since the last step
  uint32_t late_until = 0;         // no compaction before every late worker has started
  uint32_t bound_host = 0;         // last bound read back (diagnostics)
  uint64_t lin_big = 0, lin_nmax = 0;   // last linearizability scan: partitions above LIN_SMAX, largest
  // client request latency (lat_kernel.h): P.lat_stamp, P.lat_acc and the folded readout [WK][bins + LAT_EXTRA]
  unsigned long long* d_lat_out = nullptr;
  size_t lat_bytes = 0;
  size_t ch_bytes = 0;             // client-side op history (chist_kernel.h): P.ch_ops and P.ch_cnt
  size_t mv_bytes = 0;             // multi-version Database (mv_kernel.h): P.mv_val and P.mv_cnt
  // device message trace (trace_kernel.h): P.tr_row, P.tr_rec and P.tr_cnt; tr_rows: clusters traced
  size_t tr_bytes = 0;
  uint32_t tr_rows = 0;
  std::vector<uint32_t> tr_row;    // host copy of P.tr_row
  Knobs kn;                        // the create-time knobs as create read them (paxisim_fork creates with them)
};

static inline size_t rc_host(const Params& P, uint32_t r, uint64_t c) { return (size_t)r * P.C + c; }

// compressed (n << 4) | r  ->  the 64-bit Ballot of ballot.go:15-17
static uint64_t expand_ballot(const paxisim* h, uint32_t b) {
  if (!b) return 0;
  const uint32_t id = b & 15u;
  return ((uint64_t)(b >> 4) << 32) | ((uint64_t)h->zone_of[id] << 16) | h->node_of[id];
}

extern "C" int paxisim_abi_version(void) { return PAXISIM_ABI_VERSION; }
extern "C" const char* paxisim_last_error(void) { return g_err; }

// ---------------------------------------------------------------------------
// kernels: init, stats reduction, state gather, agreement scan
// ---------------------------------------------------------------------------
__global__ void init_kernel(Params P) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= P.C) return;
  const uint32_t blk = (uint32_t)(c / LANES), lane = (uint32_t)(c % LANES);
  uint8_t* img = P.image + (size_t)blk * P.img.bytes;
  P.kc[c] = cluster_key(P.seed, P.cluster_base + c);
  P.slot_of[c] = (uint32_t)c;
  P.cl_of[c] = (uint32_t)c;
  reinterpret_cast<uint32_t*>(img + P.img.off_poison)[lane] = 0xFFFFFFFFu;
  if (P.protocol == PAXISIM_PAXOS)
    for (uint32_t r = 0; r < P.N; r++) P.slot[rc(P, r, c)] = 0xFFFFFFFFu;   // slot: -1 (paxos.go:45)
  if (P.protocol == PAXISIM_WPAXOS)                                         // fresh kpaxos instances
    for (uint32_t k = 0; k < P.keys; k++)
      for (uint32_t r = 0; r < P.N; r++)
        wp_write(P, blk, k, r, lane, make_uint4(0u, 0xFFFFFFFFu, 0u, 0u), make_uint4(0u, 0u, 0u, POL_NONE));
  if (P.protocol == PAXISIM_EPAXOS) {                                      // replica.go:37-47: -1 everywhere
    for (uint32_t k = 0; k < 3 * P.N * P.N; k++) P.ep_sce[(size_t)k * P.C + c] = 0xFFFFFFFFu;
    for (uint32_t k = 0; k < P.N * P.keys * P.N; k++) P.ep_cf[(size_t)k * P.C + c] = 0xFFFFFFFFu;
    for (uint32_t k = 0; k < P.keys * P.N; k++) P.ep_max[(size_t)k * P.C + c] = 0xFFFFFFFFu;
  }
  if (c >= P.clusters) return;
  uint8_t* cnt = img + P.img.off_cnt;
  uint32_t* wcur = reinterpret_cast<uint32_t*>(img + P.img.off_wcur);
  uint32_t* wiss = reinterpret_cast<uint32_t*>(img + P.img.off_wiss);
  uint4* rec = P.rec + (size_t)blk * P.rec_per_block;
  for (uint32_t w = 0; w < P.WK; w++) {         // each worker's first request waits at step 0
    if (P.start_step[w]) continue;              // joins later (client_start, sim_core.h)
    const uint32_t box = (0u * P.N + P.target[w]) * P.NS + P.N;
    const uint32_t k = cnt[(box << 6) | lane];
    rec[((box * P.M + k) << 6) | lane] = make_uint4(PAXISIM_MSG_REQUEST, 0u, 0u, 1u + w);
    cnt[(box << 6) | lane] = (uint8_t)(k + 1u);
    wcur[(w << 6) | lane] = 1u + w;
    wiss[(w << 6) | lane] = 1u;
  }
}

constexpr int NRED = NSTAT + 8;   // counters + flagged bits

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

__global__ void stats_kernel(Params P, uint64_t* out) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = c < P.clusters;
  uint32_t cf = 0;
  for (int k = 0; k < NSTAT; k++) {
    uint64_t v = 0;
    if (live)
      for (uint32_t r = 0; r < P.N; r++) v += P.stats[krc(P, k, r, c)];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd((unsigned long long*)&out[k], (unsigned long long)v);
  }
  if (live)
    for (uint32_t r = 0; r < P.N; r++) cf |= P.flags[rc(P, r, c)];
  for (int b = 0; b < 8; b++) {
    uint64_t v = wave_sum((cf >> b) & 1u);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd((unsigned long long*)&out[NSTAT + b], (unsigned long long)v);
  }
}

__global__ void gather_kernel(Params P, uint64_t lo, uint64_t n, paxisim_replica_state* out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * P.N) return;
  const uint64_t c = slot_of(P, lo + i / P.N);
  const uint32_t r = (uint32_t)(i % P.N);
  const size_t j = rc(P, r, c);
  paxisim_replica_state s;
  memset(&s, 0, sizeof s);
  s.ballot = P.ballot[j];             // compressed; expanded on the host
  s.slot = (int32_t)P.slot[j];
  s.execute = (int32_t)P.execute[j];
  s.active = P.meta[j] & 1u;
  s.p1_acks = P.meta[j] >> 16;
  s.flags = P.flags[j];
  s.digest = P.digest[j];
  s.npending = P.npend[j] & NPEND_MASK;
  for (int k = 0; k < PAXISIM_NMSG; k++) s.delivered[k] = P.stats[krc(P, ST_DELIV0 + k, r, c)];
  s.client_requests = P.stats[krc(P, ST_CLIENT, r, c)];
  s.sent = P.stats[krc(P, ST_SENT, r, c)];
  s.dropped = P.stats[krc(P, ST_DROPPED, r, c)];
  s.discarded = P.stats[krc(P, ST_DISCARDED, r, c)];
  s.commits = P.stats[krc(P, ST_COMMITS, r, c)];
  s.replies = P.stats[krc(P, ST_REPLIES, r, c)];
  if (P.protocol == PAXISIM_ABD) {   // op counter, Done ops recorded, KV digest, live ops
    const uint8_t* img = P.image + (c / LANES) * (size_t)P.img.bytes;
    const uint32_t lane = (uint32_t)(c % LANES);
    const uint32_t* kv_val = reinterpret_cast<const uint32_t*>(img + P.img.off_a);
    const uint32_t* kv_ver = reinterpret_cast<const uint32_t*>(img + P.img.off_b);
    const uint32_t* ops = reinterpret_cast<const uint32_t*>(img + P.img.off_c);
    uint64_t d = 0;
    for (uint32_t k = 0; k < P.keys; k++) {
      const uint32_t ki = ((r * P.keys + k) << 6) | lane;
      d = mix64(d ^ (((uint64_t)kv_ver[ki] << 32) | kv_val[ki]));
    }
    uint32_t live = 0;
    for (uint32_t k = 0; k < P.OW; k++) {
      const uint32_t st = ops[(((r * P.OW + k) * ABD_OPF + 2) << 6) | lane] & 3u;
      live += st == ABD_GET || st == ABD_SET;
    }
    s.ballot = 0;
    s.active = 0;
    s.p1_acks = 0;
    s.digest = d;
    s.npending = live;
  }
  if (P.protocol == PAXISIM_EPAXOS) {   // own log head, executed prefix over all logs (paxisim.h)
    int32_t ex = 0;
    for (uint32_t o = 0; o < P.N; o++) ex += (int32_t)P.ep_sce[(((size_t)2 * P.N + o) * P.N + r) * P.C + c] + 1;
    s.ballot = 0;
    s.slot = (int32_t)P.ep_sce[(((size_t)0 * P.N + r) * P.N + r) * P.C + c];
    s.execute = ex;
    s.active = 0;
    s.p1_acks = 0;
    s.npending = 0;
  }
  if (P.protocol == PAXISIM_WPAXOS) {   // aggregate over the key instances (paxisim.h read_state)
    uint32_t hi = 0, led = 0, act = 0, ex = 0, np = 0, em = 0;
    uint64_t d = 0;
    for (uint32_t k = 0; k < P.keys; k++) {
      uint4 a, b;
      wp_read(P, c / LANES, k, r, (uint32_t)(c % LANES), a, b);
      const uint32_t exists = (a.w >> 1) & 1u;
      hi = a.x > hi ? a.x : hi;
      led += exists && ((a.w & 1u) || bal_id(a.x) == r);    // Replica.keys() replica.go:110-118
      act += a.w & 1u;
      ex += a.z;
      np += b.x;
      em |= exists << k;
      d = mix64(d ^ ((uint64_t)b.y | ((uint64_t)b.z << 32)));
    }
    s.ballot = hi;
    s.slot = (int32_t)led;
    s.execute = (int32_t)ex;
    s.active = act;
    s.p1_acks = em;
    s.npending = np;
    s.digest = d;
  }
  s.executions = P.protocol == PAXISIM_EPAXOS ? P.execute[j] : P.protocol == PAXISIM_ABD ? 0u : (uint32_t)s.execute;
  s.executed_writes = P.kv ? P.kv_ver[j] : 0u;
  out[i] = s;
}

// read_instances: one record per (cluster, replica, instance)
__global__ void gather_inst_kernel(Params P, uint64_t lo, uint64_t n, paxisim_instance_state* out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (P.protocol == PAXISIM_EPAXOS) {   // (replica, owner log): slot, executed + 1, committed + 1
    if (i >= n * P.N * P.N) return;
    const uint64_t c = slot_of(P, lo + i / (P.N * P.N));
    const uint32_t r = (uint32_t)((i / P.N) % P.N), o = (uint32_t)(i % P.N);
    paxisim_instance_state s;
    memset(&s, 0, sizeof s);
    auto sce = [&](uint32_t k) { return (int32_t)P.ep_sce[(((size_t)k * P.N + o) * P.N + r) * P.C + c]; };
    s.slot = sce(0);
    s.execute = sce(2) + 1;
    s.p1_acks = (uint32_t)(sce(1) + 1);
    s.exists = 1;
    s.policy_last = POL_NONE;
    out[i] = s;
    return;
  }
  if (i >= n * P.NI) return;
  const uint64_t c = slot_of(P, lo + i / P.NI);
  const uint32_t r = (uint32_t)((i / P.NK) % P.N), k = (uint32_t)(i % P.NK);
  paxisim_instance_state s;
  memset(&s, 0, sizeof s);
  if (P.protocol == PAXISIM_WPAXOS) {
    const size_t si = wp_si(P, c / LANES, k, r, (uint32_t)(c % LANES));
    uint4 a, b;
    wp_read(P, c / LANES, k, r, (uint32_t)(c % LANES), a, b);
    s.ballot = a.x;
    s.slot = (int32_t)a.y;
    s.execute = (int32_t)a.z;
    s.active = a.w & 1u;
    s.exists = (a.w >> 1) & 1u;
    s.p1_acks = a.w >> 16;
    s.npending = b.x;
    s.digest = (uint64_t)b.y | ((uint64_t)b.z << 32);
    s.policy_last = b.w & 0xFFu;
    s.policy_hits = (b.w >> 8) & 0xFFu;
    if (P.policy == PAXISIM_POLICY_MAJORITY) {
      const uint4 h0 = P.wpx[3 * si], h1 = P.wpx[3 * si + 1], m = P.wpx[3 * si + 2];
      const uint32_t w[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
      uint32_t h = 0x811C9DC5u;
      for (uint32_t j = 0; j < P.N; j++) h = fmix32(h ^ (((w[j >> 1] >> ((j & 1u) * 16u)) & 0xFFFFu) | j << 16));
      s.policy_state[0] = m.x;
      s.policy_state[1] = m.y;
      s.policy_state[2] = h;
    } else if (P.policy == PAXISIM_POLICY_EMA) {
      const uint4 m = P.wpx[3 * si + 2];
      s.policy_state[0] = m.x;
      s.policy_state[1] = m.y;
      s.policy_state[2] = m.z;
    }
  } else {
    const size_t j = rc(P, r, c);
    s.ballot = P.ballot[j];
    s.slot = (int32_t)P.slot[j];
    s.execute = (int32_t)P.execute[j];
    s.active = P.meta[j] & 1u;
    s.exists = 1;
    s.p1_acks = P.meta[j] >> 16;
    s.npending = P.npend[j] & NPEND_MASK;
    s.digest = P.digest[j];
    s.policy_last = POL_NONE;
  }
  out[i] = s;
}

// Agreement scan (client.go:279-320; tla/wpaxos.tla Safety): replicas that
// executed the same number of slots must hold the same digest, and digest
// checkpoints taken at the same executed count must agree.  The per-cluster body is verdict_kernel.h agree_bad, which the
// verdict pass calls too, so the count and the PAXISIM_V_AGREE bit cannot drift apart.
__global__ void check_kernel(Params P, uint64_t* out) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t bad = 0;
  if (c < P.clusters && P.protocol != PAXISIM_EPAXOS) bad = agree_bad(P, c) ? 1u : 0u;   // EPaxos: no single log (paxisim.h)
  bad = wave_sum(bad);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd((unsigned long long*)out, (unsigned long long)bad);
}

// Pipelined launches (sim_core.h sim_serial_pipe) need the dispatcher to deal a
// launch's workgroups to 8 XCDs in turn (any rotation): each XCD's ticket queue
// then has exactly one workgroup per ticket.  This records the XCD of 64
// workgroups; create turns pipelining off when they are not dealt that way
// (another compute partition mode), rather than let chunks go unrun.
__global__ void xcc_probe(uint32_t* out) {
  if (threadIdx.x == 0) out[blockIdx.x] = __builtin_amdgcn_s_getreg((20) | (0 << 6) | ((32 - 1) << 11));   // HW_REG_XCC_ID
}

// paxisim_inject: one client request record into (bucket b, dst r, src client)
__global__ void inject_kernel(Params P, uint64_t cl, uint32_t r, uint32_t b, uint32_t cid, uint32_t* status) {
  if (threadIdx.x != 0) return;
  const uint64_t c = slot_of(P, cl);
  const uint32_t blk = (uint32_t)(c / LANES), lane = (uint32_t)(c % LANES);
  uint8_t* cnt = P.image + (size_t)blk * P.img.bytes + P.img.off_cnt;
  const uint32_t box = (b * P.N + r) * P.NS + P.N;
  const uint32_t k = cnt[(box << 6) | lane];
  if (k >= P.M) {
    *status = 1;
    return;
  }
  P.rec[(size_t)blk * P.rec_per_block + (((box * P.M + k) << 6) | lane)] = make_uint4(PAXISIM_MSG_REQUEST, 0u, 0u, cid);
  cnt[(box << 6) | lane] = (uint8_t)(k + 1u);
  *status = 0;
}

// paxisim_read_inbox: replica r's bucket b, source by source, FIFO order
__global__ void read_inbox_kernel(Params P, uint64_t cl, uint32_t r, uint32_t b, paxisim_inbox_record* out,
                                  uint32_t cap, uint32_t* n_out) {
  if (threadIdx.x != 0) return;
  const uint64_t c = slot_of(P, cl);
  const uint32_t blk = (uint32_t)(c / LANES), lane = (uint32_t)(c % LANES);
  const uint8_t* cnt = P.image + (size_t)blk * P.img.bytes + P.img.off_cnt;
  const uint4* rec = P.rec + (size_t)blk * P.rec_per_block;
  uint32_t n = 0;
  for (uint32_t src = 0; src < P.NS; src++) {
    const uint32_t box = (b * P.N + r) * P.NS + src;
    const uint32_t k_n = cnt[(box << 6) | lane];
    for (uint32_t k = 0; k < k_n; k++, n++) {
      if (n >= cap) continue;
      const uint4 m = rec[((box * P.M + k) << 6) | lane];
      out[n] = paxisim_inbox_record{src, m.x, m.y, m.z, m.w};
    }
  }
  *n_out = n;
}

// paxisim_deliver: n records appended to (bucket b, dst r, src)
__global__ void deliver_kernel(Params P, uint64_t cl, uint32_t r, uint32_t src, uint32_t b,
                               const paxisim_inbox_record* in, uint32_t n, uint32_t* status) {
  if (threadIdx.x != 0) return;
  const uint64_t c = slot_of(P, cl);
  const uint32_t blk = (uint32_t)(c / LANES), lane = (uint32_t)(c % LANES);
  uint8_t* cnt = P.image + (size_t)blk * P.img.bytes + P.img.off_cnt;
  const uint32_t box = (b * P.N + r) * P.NS + src;
  const uint32_t k = cnt[(box << 6) | lane];
  if (k + n > P.M) {
    *status = 1;
    return;
  }
  uint4* rec = P.rec + (size_t)blk * P.rec_per_block;
  for (uint32_t i = 0; i < n; i++)
    rec[(((box * P.M + k + i) << 6) | lane)] = make_uint4(in[i].hdr, in[i].ballot, in[i].slot, in[i].cid);
  cnt[(box << 6) | lane] = (uint8_t)(k + n);
  *status = 0;
}

// paxisim_commands: the workload's key and kind of each command id
__global__ void command_kernel(Params P, uint64_t cl, const uint32_t* cids, uint32_t n, uint32_t* keys,
                               uint32_t* writes) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t kc = P.kc[slot_of(P, cl)];
  keys[i] = wl_key(P, kc, cids[i]);
  writes[i] = wl_write(P, kc, cids[i]) ? 1u : 0u;
}

// paxisim_read_log: one thread per slot of one instance's window
__global__ void read_log_kernel(Params P, uint64_t cl, uint32_t r, uint32_t key, int32_t lo, uint32_t n,
                                paxisim_log_entry* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t c = slot_of(P, cl);
  const uint32_t blk = (uint32_t)(c / LANES), lane = (uint32_t)(c % LANES);
  const int32_t s = lo + (int32_t)i;
  paxisim_log_entry o;
  memset(&o, 0, sizeof o);
  o.slot = s;
  int32_t execute;
  uint32_t eb, ec, ea, ex;
  const uint32_t w = (uint32_t)s & (P.W - 1u);
  if (P.protocol == PAXISIM_WPAXOS) {
    const size_t si = wp_si(P, blk, key, r, lane);
    uint4 a, b;
    wp_read(P, blk, key, r, lane, a, b);
    execute = (int32_t)a.z;
    const uint32_t* e = P.wlog + si * P.wlog_str + w * 4u;
    eb = e[0]; ec = e[1]; ea = e[2]; ex = e[3];
  } else {
    execute = (int32_t)P.execute[rc(P, r, c)];
    const uint8_t* img = P.image + (size_t)blk * P.img.bytes;
    const uint32_t li = ((r * P.W + w) << 6) | lane;
    if (P.packed) {
      const uint4 e = P.plog[(size_t)blk * (P.N * P.W * LANES) + li];
      eb = e.x; ec = e.y; ea = e.z; ex = e.w;
    } else {
      eb = reinterpret_cast<const uint32_t*>(img + P.img.off_a)[li];
      ec = reinterpret_cast<const uint32_t*>(img + P.img.off_b)[li];
      ea = reinterpret_cast<const uint32_t*>(img + P.img.off_c)[li];
      ex = P.reqx[(size_t)blk * (P.N * P.W * LANES) + li];
    }
  }
  if (s >= execute && s < execute + (int32_t)P.W) {
    o.flags = PAXISIM_LOG_HELD;
    if (ec & EF_EXISTS) {
      o.flags |= PAXISIM_LOG_EXISTS | ((ec & EF_COMMIT) ? PAXISIM_LOG_COMMIT : 0u) |
                 ((ec & EF_QUORUM) ? PAXISIM_LOG_QUORUM : 0u) |
                 ((ec & (EF_REQSELF | EF_REQEXT)) ? PAXISIM_LOG_REQUEST : 0u);
      o.ballot = eb;                                          // compressed; expanded on the host
      o.cmd = ec & CMD_MASK;
      o.acks = ea;
      o.request = (ec & EF_REQSELF) ? ((ec & CMD_MASK) | (PAXISIM_CLIENT_SRC << 27)) : (ec & EF_REQEXT) ? ex : 0u;
    }
  }
  out[i] = o;
}


// ---------------------------------------------------------------------------
// Live-cluster compaction.  A Paxos cluster whose mailboxes
// are empty at the end of a launch is at a fixed point: Paxi has no timers or
// retries, so nothing in it changes again unless a request is injected.  Its
// only evolving state is the random fault process of its links, which no
// handler can observe while no message moves.  Every cmp_every steps the
// slots [0, bound) are partitioned so that live clusters fill whole 64-cluster
// tiles at the front: the k-th quiescent slot below lnew swaps all its state
// with the k-th live slot above it, and slots [lnew, bound) freeze (frz =
// the step they stopped at).  Workgroups past the bound exit at once, so
// launches stop paying for lanes whose clusters have died.  A request
// injected into a frozen cluster wakes its tile: the link fault process is
// replayed over the frozen steps, so the trajectory is exactly the one the
// oracle computes without any of this.
// ---------------------------------------------------------------------------
constexpr uint32_t CB = 1024;                    // slots per counting block
enum { CM_BOUND = 0, CM_LNEW, CM_NPAIRS, CM_LIVE, CM_LBL, CM_SUMS = 8 };

template <typename T>
__device__ __forceinline__ void swap_rows(T* a, size_t rows, size_t C, uint64_t p, uint64_t q, uint32_t j) {
  for (size_t k = j; k < rows; k += LANES) {
    const T v = a[k * C + p];
    a[k * C + p] = a[k * C + q];
    a[k * C + q] = v;
  }
}
// lane-fastest per-block regions: element (row, lane) of block b at base + b*bstride + row*64 + lane
template <typename T>
__device__ __forceinline__ void swap_lanes(T* base, size_t bstride, size_t rows, uint64_t p, uint64_t q, uint32_t j) {
  T* bp = base + (p / LANES) * bstride + (p % LANES);
  T* bq = base + (q / LANES) * bstride + (q % LANES);
  for (size_t k = j; k < rows; k += LANES) {
    const T v = bp[k * LANES];
    bp[k * LANES] = bq[k * LANES];
    bq[k * LANES] = v;
  }
}

// Swap every per-slot datum of the Paxos step kernel between slots p and q
// (one wave per pair, lane j takes every 64th element).  Only live data moves
// (round 5): pending / forward entries past their counts and the ghost table
// of a replica that never raised GHOST are never read before they are written
// (paxos_kernel.h), so a pair moves max(count_p, count_q) of them; the
// agreement ring is indexed by cluster id, not slot (sim_core.h agree_drain),
// and does not move at all.
static_assert(PMAX + FMAX == LANES, "swap_slots: one lane per pending / forwards entry");
__device__ void swap_slots(const Params& P, uint64_t p, uint64_t q, uint32_t j) {
  const size_t C = P.C, N = P.N;
  // live extents, read before any row moves (uniform across the wave)
  for (uint32_t r = 0; r < N; r++) {
    const size_t ip = (size_t)r * C + p, iq = (size_t)r * C + q;
    const uint32_t np0 = P.npend[ip] & NPEND_MASK, np1 = P.npend[iq] & NPEND_MASK;
    const uint32_t nf0 = P.nfwd[ip] & NFWD_MASK, nf1 = P.nfwd[iq] & NFWD_MASK;
    const bool gh = ((P.flags[ip] | P.flags[iq]) & PAXISIM_F_GHOST) != 0u;
    const uint32_t np = np0 > np1 ? np0 : np1, nf = nf0 > nf1 ? nf0 : nf1;
    // lane j < 32: pending entry j, 32 <= j < 64: forwards entry j - 32 (PMAX = FMAX = 32)
    uint32_t* a = nullptr;
    if (j < PMAX && j < np) a = P.pend + ((size_t)j * P.NI + r) * C;
    else if (j >= PMAX && j - PMAX < nf) a = P.fwd + ((size_t)(j - PMAX) * N + r) * C;
    uint32_t vp = 0, vq = 0;
    uint4 gp = make_uint4(0u, 0u, 0u, 0u), gq = gp;
    uint4* g = nullptr;
    if (gh && j < GMAX) g = P.gst + ((size_t)j * P.NI + r) * C;
    if (a) { vp = a[p]; vq = a[q]; }
    if (g) { gp = g[p]; gq = g[q]; }
    if (a) { a[p] = vq; a[q] = vp; }
    if (g) { g[p] = gq; g[q] = gp; }
  }
  swap_rows(P.ballot, 7 * N, C, p, q, j);        // ballot slot execute meta flags npend (+ committed bits) nfwd (+ exists bits)
  swap_rows(P.digest, N, C, p, q, j);
  swap_rows(P.kc, 1, C, p, q, j);
  swap_rows(P.link_drop, 2 * N * N, C, p, q, j);   // link_drop then link_slow
  swap_rows(P.ck_e, (size_t)CKR * P.NI, C, p, q, j);
  swap_rows(P.ck_d, (size_t)CKR * P.NI, C, p, q, j);
  swap_rows(P.stats, (size_t)NSTAT * N, C, p, q, j);
  swap_rows(P.kv_val, P.kv ? (size_t)P.keys * N : 0, C, p, q, j);
  swap_rows(P.kv_ver, P.kv ? N : 0, C, p, q, j);
  swap_rows(P.wrep, P.WK, C, p, q, j);
  if (P.lat_bins) swap_rows(P.lat_stamp, P.WK, C, p, q, j);   // the issue stamps belong to the cluster
  swap_rows(P.frz, 1, C, p, q, j);
  swap_rows(P.qf, 1, C, p, q, j);
  if (P.phase_sort) swap_rows(P.phase, 1, C, p, q, j);
  // log windows: the packed entries (rows of 64 uint4), or the request side table beside the image's planes
  if (P.packed) swap_lanes(P.plog, (size_t)N * P.W * LANES, (size_t)N * P.W, p, q, j);
  else swap_lanes(P.reqx, (size_t)N * P.W * LANES, (size_t)N * P.W, p, q, j);
  // LDS image: u32 rows (log window a/b/c where it has them, worker tables, poison), then u8 mailbox counts
  swap_lanes(reinterpret_cast<uint32_t*>(P.image), P.img.bytes / 4u, P.img.off_cnt / (LANES * 4u), p, q, j);
  {
    uint8_t* cp = P.image + (p / LANES) * (size_t)P.img.bytes + P.img.off_cnt + (p % LANES);
    uint8_t* cq = P.image + (q / LANES) * (size_t)P.img.bytes + P.img.off_cnt + (q % LANES);
    uint4* rp = P.rec + (p / LANES) * (size_t)P.rec_per_block + (p % LANES);
    uint4* rq = P.rec + (q / LANES) * (size_t)P.rec_per_block + (q % LANES);
    const uint32_t nbox = P.D * P.N * P.NS;
    for (uint32_t b = j; b < nbox; b += LANES) {           // records in flight, then their counts
      const uint32_t kp = cp[b * LANES], kq = cq[b * LANES];
      const uint32_t kn = kp > kq ? kp : kq;
      for (uint32_t k = 0; k < kn; k++) {
        const size_t o = (size_t)(b * P.M + k) * LANES;
        const uint4 v = rp[o];
        rp[o] = rq[o];
        rq[o] = v;
      }
      cp[b * LANES] = (uint8_t)kq;
      cq[b * LANES] = (uint8_t)kp;
    }
  }
  if (j == 0) {
    const uint32_t a = P.cl_of[p], b = P.cl_of[q];
    P.cl_of[p] = b;
    P.cl_of[q] = a;
    P.slot_of[b] = (uint32_t)p;
    P.slot_of[a] = (uint32_t)q;
  }
}

// The compaction and phase-binning kernels work on one pool's region: slot s = base + ..., the
// bound in cm[CM_BOUND] absolute and never past the region's end.
__global__ void cmp_count(Params P, uint32_t* cm, uint32_t base) {
  const uint64_t s = base + (uint64_t)blockIdx.x * CB + threadIdx.x;
  const int live = s < cm[CM_BOUND] && !P.qf[s];
  const int n = __syncthreads_count(live);
  if (threadIdx.x == 0) cm[CM_SUMS + blockIdx.x] = (uint32_t)n;
}

// one workgroup of CB threads: exclusive scan of the block counts, then the
// new bound and the number of pairs to swap
__global__ void cmp_scan(Params P, uint32_t* cm, uint32_t nb, uint32_t base) {
  __shared__ uint32_t sh[CB];
  __shared__ uint32_t carry;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (uint32_t base = 0; base < nb; base += CB) {
    const uint32_t v = base + tid < nb ? cm[CM_SUMS + base + tid] : 0u;
    sh[tid] = v;
    __syncthreads();
    for (uint32_t off = 1; off < CB; off <<= 1) {
      const uint32_t t = tid >= off ? sh[tid - off] : 0u;
      __syncthreads();
      sh[tid] += t;
      __syncthreads();
    }
    if (base + tid < nb) cm[CM_SUMS + base + tid] = carry + sh[tid] - v;
    __syncthreads();
    if (tid == 0) carry += sh[CB - 1];
    __syncthreads();
  }
  const uint32_t live = carry, bound = cm[CM_BOUND];
  uint32_t lnew = base + (live + LANES - 1u) / LANES * LANES;
  if (lnew > bound) lnew = bound;
  const uint32_t b = (lnew - base) / CB;
  const uint64_t s = base + (uint64_t)b * CB + tid;
  const int cnt = __syncthreads_count(s < lnew && !P.qf[s]);
  const uint32_t lbl = (b < nb ? cm[CM_SUMS + b] : live) + (uint32_t)cnt;   // live slots below lnew
  if (tid == 0) {
    cm[CM_LNEW] = lnew;
    cm[CM_LIVE] = live;
    cm[CM_LBL] = lbl;
    cm[CM_NPAIRS] = live - lbl;
  }
}

__global__ void cmp_index(Params P, uint32_t* cm, uint32_t* lo, uint32_t* hi, uint32_t base) {
  __shared__ uint32_t wsum[CB / LANES];
  const uint64_t s = base + (uint64_t)blockIdx.x * CB + threadIdx.x;
  const uint32_t bound = cm[CM_BOUND], lnew = cm[CM_LNEW], lbl = cm[CM_LBL], np = cm[CM_NPAIRS];
  const bool live = s < bound && !P.qf[s];
  const uint64_t m = __ballot(live);
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint32_t inw = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) wsum[w] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t off = 0;
  for (uint32_t k = 0; k < w; k++) off += wsum[k];
  const uint32_t before = cm[CM_SUMS + blockIdx.x] + off + inw;     // live slots in [base, s)
  if (s >= bound) return;
  if (!live && s < lnew) {
    const uint32_t k = (uint32_t)s - base - before;                // dead slots in [base, s)
    if (k < np) lo[k] = (uint32_t)s;
  } else if (live && s >= lnew) {
    hi[before - lbl] = (uint32_t)s;
  }
}

__global__ void cmp_swap(Params P, const uint32_t* cm, const uint32_t* lo, const uint32_t* hi) {
  const uint32_t np = cm[CM_NPAIRS];
  for (uint32_t k = blockIdx.x; k < np; k += gridDim.x) swap_slots(P, lo[k], hi[k], threadIdx.x);
}

__global__ void cmp_freeze(Params P, uint32_t* cm, uint32_t t, uint32_t base) {
  const uint64_t s = base + (uint64_t)blockIdx.x * CB + threadIdx.x;
  if (s >= cm[CM_LNEW] && s < cm[CM_BOUND]) P.frz[s] = t;
}
__global__ void cmp_setbound(uint32_t* cm) { cm[CM_BOUND] = cm[CM_LNEW]; }

__global__ void swap_one(Params P, uint64_t p, uint64_t q) { swap_slots(P, p, q, threadIdx.x); }

// ---------------------------------------------------------------------------
// Phase binning.  After the live/dead partition, the stepped
// slots [0, bound) are grouped by class - the phase residue each live cluster
// was busiest at in the last launch, then the quiescent slots - with the same
// pair swaps: pass p moves every class-p slot into the region [base_p, end_p)
// by swapping the k-th misplaced slot inside it with the k-th class-p slot
// beyond it.  Slots that kept their phase stay where they are, so a pass costs
// the clusters whose phase drifted.
// ---------------------------------------------------------------------------
enum { PH_N = 0, PH_BASE = 8, PH_END = 9, PH_SUMS = 16 };   // PH_N + class: classes 0..period (quiescent last)
__device__ __forceinline__ uint32_t ph_class(const Params& P, uint64_t s) {
  return P.qf[s] ? P.phase_period : P.phase[s];
}
__global__ void ph_classes(Params P, const uint32_t* cm, uint32_t* ph, uint32_t base) {
  const uint64_t s = base + (uint64_t)blockIdx.x * CB + threadIdx.x;
  const uint32_t bound = cm[CM_BOUND];
  const uint32_t c = s < bound ? ph_class(P, s) : 0xFFu;
  for (uint32_t k = 0; k <= P.phase_period; k++) {
    const int n = __syncthreads_count(c == k);
    if (threadIdx.x == 0 && n) atomicAdd(&ph[PH_N + k], (uint32_t)n);
  }
}
// region of class p: [sum of classes < p, + count of p)
__global__ void ph_region(uint32_t* ph, uint32_t p, uint32_t base) {
  uint32_t b = base;
  for (uint32_t k = 0; k < p; k++) b += ph[PH_N + k];
  ph[PH_BASE] = b;
  ph[PH_END] = b + ph[PH_N + p];
}
// per block: misplaced slots inside the region (class != p) and class-p slots beyond it
__global__ void ph_count(Params P, const uint32_t* cm, uint32_t* ph, uint32_t p, uint32_t nb, uint32_t sbase) {
  const uint64_t s = sbase + (uint64_t)blockIdx.x * CB + threadIdx.x;
  const uint32_t bound = cm[CM_BOUND], base = ph[PH_BASE], end = ph[PH_END];
  const uint32_t c = s < bound ? ph_class(P, s) : 0xFFu;
  const int in = __syncthreads_count(s >= base && s < end && c != p);
  const int out = __syncthreads_count(s >= end && s < bound && c == p);
  if (threadIdx.x == 0) {
    ph[PH_SUMS + blockIdx.x] = (uint32_t)in;
    ph[PH_SUMS + nb + blockIdx.x] = (uint32_t)out;
  }
}
// exclusive scans of both count arrays (one workgroup); the pair count to cm
__global__ void ph_scan(uint32_t* cm, uint32_t* ph, uint32_t nb) {
  __shared__ uint32_t sh[CB];
  __shared__ uint32_t carry;
  const uint32_t tid = threadIdx.x;
  for (uint32_t a = 0; a < 2; a++) {
    uint32_t* arr = ph + PH_SUMS + a * nb;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < nb; base += CB) {
      const uint32_t v = base + tid < nb ? arr[base + tid] : 0u;
      sh[tid] = v;
      __syncthreads();
      for (uint32_t off = 1; off < CB; off <<= 1) {
        const uint32_t t = tid >= off ? sh[tid - off] : 0u;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
      }
      if (base + tid < nb) arr[base + tid] = carry + sh[tid] - v;
      __syncthreads();
      if (tid == 0) carry += sh[CB - 1];
      __syncthreads();
    }
    if (a == 0 && tid == 0) cm[CM_NPAIRS] = carry;   // misplaced inside = class-p outside
  }
}
__global__ void ph_index(Params P, const uint32_t* cm, const uint32_t* ph, uint32_t p, uint32_t nb, uint32_t* lo,
                         uint32_t* hi, uint32_t sbase) {
  __shared__ uint32_t wa[CB / LANES], wb[CB / LANES];
  const uint64_t s = sbase + (uint64_t)blockIdx.x * CB + threadIdx.x;
  const uint32_t bound = cm[CM_BOUND], base = ph[PH_BASE], end = ph[PH_END];
  const uint32_t c = s < bound ? ph_class(P, s) : 0xFFu;
  const bool in = s >= base && s < end && c != p, out = s >= end && s < bound && c == p;
  const uint64_t ma = __ballot(in), mb = __ballot(out);
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  if (lane == 0) { wa[w] = (uint32_t)__popcll(ma); wb[w] = (uint32_t)__popcll(mb); }
  __syncthreads();
  uint32_t oa = 0, ob = 0;
  for (uint32_t k = 0; k < w; k++) { oa += wa[k]; ob += wb[k]; }
  const uint64_t below = (1ull << lane) - 1ull;
  if (in) lo[ph[PH_SUMS + blockIdx.x] + oa + (uint32_t)__popcll(ma & below)] = (uint32_t)s;
  if (out) hi[ph[PH_SUMS + nb + blockIdx.x] + ob + (uint32_t)__popcll(mb & below)] = (uint32_t)s;
}

// Wake: the link fault process of slots [s0, s1) over the steps they were frozen
__global__ void replay_kernel(Params P, uint64_t s0, uint64_t s1, uint32_t tnow) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t c = s0 + i / P.N;
  if (c >= s1) return;
  Rep<0> x;
  x.r = (uint32_t)(i % P.N);
  x.c = c;
  x.kc = P.kc[c];
  const uint32_t poison =
      reinterpret_cast<const uint32_t*>(P.image + (c / LANES) * (size_t)P.img.bytes + P.img.off_poison)[c % LANES];
  uint32_t du[Rep<0>::NL], su[Rep<0>::NL];
  for (uint32_t d = 0; d < Rep<0>::NL; d++) {
    du[d] = d < P.N ? P.link_drop[krc(P, d, x.r, c)] : 0u;
    su[d] = d < P.N ? P.link_slow[krc(P, d, x.r, c)] : 0u;
  }
  for (uint32_t t = P.frz[c]; t < tnow && t <= poison; t++) {   // the step kernel's gate: poison >= t
    x.t = t;
    x.hs = step_key(x.kc, t);
    fault_process<0>(P, x, du, su);
  }
}

// ---------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------
static int pipe_check(paxisim* h);

// Every entry point but paxisim_step works on the handle's stream.  With two pools it first makes
// that stream wait for what the pools' streams have been given (an event on each), and notes that
// the next paxisim_step must make the pools' streams wait for the handle's; consecutive steps with
// nothing between them add no dependency between streams.
static int enter(paxisim* h) {
  HIPCHK(hipSetDevice(h->cfg.device));
  if (h->npools > 1) {
    if (h->pools_ahead) {
      for (uint32_t p = 0; p < h->npools; p++) {
        HIPCHK(hipEventRecord(h->pool[p].ev, h->pool[p].stream));
        HIPCHK(hipStreamWaitEvent(h->stream, h->pool[p].ev, 0));
      }
      h->pools_ahead = false;
    }
    h->main_ahead = true;
  }
  return 0;
}

// Kernel time: one pool, the sum of the launches' times; two pools, whose launches overlap, the
// length of the union of their [start, end] intervals, each taken against the batch's first event.
static int flush_events(paxisim* h) {
  const bool any = !h->evs.empty();
  std::vector<std::pair<double, double>> iv;
  for (auto& e : h->evs) {
    float ms = 0;
    HIPCHK(hipEventSynchronize(e.second));
    HIPCHK(hipEventElapsedTime(&ms, e.first, e.second));
    if (h->npools > 1) {
      float at = 0;
      if (e.first != h->evs[0].first) {
        HIPCHK(hipEventSynchronize(h->evs[0].second));   // the base event has been reached
        // the other pool's launch may have started before the base event: a negative offset
        if (hipEventElapsedTime(&at, h->evs[0].first, e.first) != hipSuccess) {
          (void)hipGetLastError();
          HIPCHK(hipEventElapsedTime(&at, e.first, h->evs[0].first));
          at = -at;
        }
      }
      iv.emplace_back((double)at, (double)at + ms);
    } else {
      h->kernel_ms += ms;
    }
  }
  if (h->npools > 1) h->kernel_ms += interval_union(iv);
  for (auto& e : h->evs) {
    (void)hipEventDestroy(e.first);
    (void)hipEventDestroy(e.second);
  }
  h->evs.clear();
  // after the waits: the error word is read once every timed launch has ended
  return any ? pipe_check(h) : 0;
}

extern "C" int paxisim_destroy(paxisim* h) {
  if (!h) return 0;
  (void)hipSetDevice(h->cfg.device);
  for (uint32_t p = 0; p < h->npools; p++)
    if (h->pool[p].stream) (void)hipStreamSynchronize(h->pool[p].stream);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  flush_events(h);
  if (h->arena) (void)hipFree(h->arena);
  if (h->d_faults) (void)hipFree(h->d_faults);
  if (h->d_move) (void)hipFree(h->d_move);
  if (h->d_scratch) (void)hipFree(h->d_scratch);
  for (Pool& pl : h->pool) {
    if (pl.d_cmp) (void)hipFree(pl.d_cmp);
    if (pl.d_pairs) (void)hipFree(pl.d_pairs);
    if (pl.d_ph) (void)hipFree(pl.d_ph);
    if (pl.d_pipe) (void)hipFree(pl.d_pipe);
    if (pl.ev) (void)hipEventDestroy(pl.ev);
    if (pl.stream && pl.stream != h->stream) (void)hipStreamDestroy(pl.stream);
  }
  if (h->ev_main) (void)hipEventDestroy(h->ev_main);
  if (h->P.lat_stamp) (void)hipFree(h->P.lat_stamp);
  if (h->P.lat_acc) (void)hipFree(h->P.lat_acc);
  if (h->d_lat_out) (void)hipFree(h->d_lat_out);
  if (h->P.ch_ops) (void)hipFree(h->P.ch_ops);
  if (h->P.ch_cnt) (void)hipFree(h->P.ch_cnt);
  if (h->P.mv_val) (void)hipFree(h->P.mv_val);
  if (h->P.mv_cnt) (void)hipFree(h->P.mv_cnt);
  if (h->P.tr_row) (void)hipFree(const_cast<uint32_t*>(h->P.tr_row));
  if (h->P.tr_rec) (void)hipFree(h->P.tr_rec);
  if (h->P.tr_cnt) (void)hipFree(h->P.tr_cnt);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return 0;
}

static StepOps step_ops_for(uint32_t protocol, uint32_t N, bool wlds, bool serial) {
  if (serial) {
    if (protocol == PAXISIM_WPAXOS) return wpaxos_serial_step_ops(N, wlds);
    if (protocol == PAXISIM_ABD) return abd_serial_step_ops(N);
    if (protocol == PAXISIM_EPAXOS) return epaxos_serial_step_ops(N);
    return paxos_serial_step_ops(N);
  }
  if (protocol == PAXISIM_WPAXOS) return wpaxos_step_ops(N, wlds);
  if (protocol == PAXISIM_ABD) return abd_step_ops(N);
  if (protocol == PAXISIM_EPAXOS) return epaxos_step_ops(N);
  return paxos_step_ops(N);
}

// The same units built with PXS_LAT = 1 (paxisim_dev.h): the step kernels that record client
// request latency.  Their StepOps and Params are the declarations of step_ops.h and
// paxisim_dev.h under another namespace, so the layouts are equal.
namespace pxs_lat {
pxs::StepOps paxos_serial_step_ops(uint32_t N);
pxs::StepOps abd_serial_step_ops(uint32_t N);
pxs::StepOps wpaxos_serial_step_ops(uint32_t N, bool lds);
pxs::StepOps epaxos_serial_step_ops(uint32_t N);
pxs::StepOps paxos_step_ops(uint32_t N);
pxs::StepOps abd_step_ops(uint32_t N);
pxs::StepOps wpaxos_step_ops(uint32_t N, bool lds);
pxs::StepOps epaxos_step_ops(uint32_t N);
}  // namespace pxs_lat
static StepOps lat_step_ops_for(uint32_t protocol, uint32_t N, bool wlds, bool serial) {
  if (serial) {
    if (protocol == PAXISIM_WPAXOS) return pxs_lat::wpaxos_serial_step_ops(N, wlds);
    if (protocol == PAXISIM_ABD) return pxs_lat::abd_serial_step_ops(N);
    if (protocol == PAXISIM_EPAXOS) return pxs_lat::epaxos_serial_step_ops(N);
    return pxs_lat::paxos_serial_step_ops(N);
  }
  if (protocol == PAXISIM_WPAXOS) return pxs_lat::wpaxos_step_ops(N, wlds);
  if (protocol == PAXISIM_ABD) return pxs_lat::abd_step_ops(N);
  if (protocol == PAXISIM_EPAXOS) return pxs_lat::epaxos_step_ops(N);
  return pxs_lat::paxos_step_ops(N);
}

// The 5-replica Multi-Paxos serial unit compiled for config 2's fixed shape (k_paxos5f.hip, shape.h)
// and its recording twin, again the declarations of step_ops.h under namespaces of their own.
namespace pxs_fix {
pxs::StepOps paxos5_fixed_step_ops();
}
namespace pxs_fix_lat {
pxs::StepOps paxos5_fixed_step_ops();
}

// The step unit a handle runs: the fixed-shape one while the handle has the shape (shape_plan.h),
// else the generic one of its protocol and N; the recording build of either once latency is enabled.
// Both units keep the same state in the same layout and take the same launch shape, so a handle
// changes unit between two launches with nothing to convert.
static ShapeFields shape_fields(const Params& P) {
  return ShapeFields{P.N, P.NS, P.NI, P.NK, P.Z, P.W, P.q1, P.q2, P.kv, P.dist, P.rwc, P.thrifty, P.ephemeral,
                     P.nfaults, P.late_workers, P.max_requests, P.locality_ppm, P.move_every, P.key_tail};
}
static void select_unit(paxisim* h) {
  const bool serial = h->ops.serial;
  const bool fixed = h->shape_fit && serial && shape_fields_fit(shape_fields(h->P));
  const bool lat = h->P.lat_bins != 0;
  StepOps ops = fixed ? (lat ? pxs_fix_lat::paxos5_fixed_step_ops() : pxs_fix::paxos5_fixed_step_ops())
                      : (lat ? lat_step_ops_for(h->P.protocol, h->P.N, h->P.wlds != 0, serial)
                             : step_ops_for(h->P.protocol, h->P.N, h->P.wlds != 0, serial));
  h->ops = ops;
  h->fixed = fixed;
  h->lds_set = -1;   // the dynamic-LDS ceiling is per kernel
}

static hipError_t ensure_lds(paxisim* h);

static size_t count_blocks(size_t slots) { return (slots + CB - 1) / CB; }
// a pool's pipeline words: the header, then the chunks done per tile (the XCD probe writes 64 words there)
static size_t pipe_words(size_t C) { return 16 + (C / LANES > 64 ? C / LANES : 64); }
// a pool's compaction and phase-binning scratch, for a region of nblk counting blocks
static hipError_t pool_scratch(Pool& pl, size_t C, size_t nblk) {
  hipError_t e = hipMalloc(&pl.d_cmp, sizeof(uint32_t) * (CM_SUMS + nblk));
  if (e == hipSuccess) e = hipMalloc(&pl.d_pairs, sizeof(uint32_t) * 2 * (C / 2 + LANES));
  if (e == hipSuccess) e = hipMalloc(&pl.d_ph, sizeof(uint32_t) * (PH_SUMS + 2 * nblk));
  return e;
}

// the wave slots the handle's step kernel keeps resident on the current device (0: not known)
static uint32_t resident_slots(paxisim* h) {
  int dev = 0, cus = 0, per = 0;
  const bool ok = ensure_lds(h) == hipSuccess && hipGetDevice(&dev) == hipSuccess &&
                  hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
                  h->ops.occupancy(h->P, &per) == hipSuccess && cus > 0 && per > 0;
  (void)hipGetLastError();
  return ok ? (uint32_t)(cus * per) : 0u;
}

// Cluster pools.  Two pools only for a handle that compacts and runs pipelined
// serial launches (Multi-Paxos); every other handle runs one.  PAXISIM_POOLS=1|2 decides; without it a
// 5-replica handle takes two when its tiles are at least four times the resident wave slots (config 2:
// 16,384 tiles against 2,048 slots, +2.7% in both mirrored pairs; no test-size handle).  The 9-replica
// unit is left out by rule: config 4 measured -0.7% with two pools.  The split is a multiple of 8 tiles
// as near the middle as that allows (pool_plan.h); if it leaves a region empty the handle runs one pool.
static int pools_setup(paxisim* h, const Knobs& kn) {
  const Params& P = h->P;
  if (kn.pools < 0) return fail(PAXISIM_EINVAL, "PAXISIM_POOLS must be 1 or 2");
  const bool can = P.compact && h->pipe_max > 1;   // pipelined (plan_schedule)
  const uint32_t tiles = (uint32_t)(P.C / LANES);
  const uint32_t slots = pool_want_asks_slots(kn.pools, can, P.N) ? resident_slots(h) : 0u;
  const uint32_t split = pool_want(kn.pools, can, P.N, tiles, slots) > 1 ? pool_split_tile(tiles, h->cfg.clusters) : 0u;
  if (!split) return 0;
  Pool& a = h->pool[0];
  Pool& b = h->pool[1];
  const size_t C = P.C;
  a.end = b.base = split * LANES;
  b.end = (uint32_t)C;
  b.last_cmp = pool_first_cmp(1, h->S);
  hipError_t e;
  a.stream = nullptr;
  h->npools = 2;   // from here on paxisim_destroy frees what was made
  if ((e = hipStreamCreateWithFlags(&a.stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipStreamCreateWithFlags(&b.stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&a.ev, hipEventDisableTiming)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&b.ev, hipEventDisableTiming)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&h->ev_main, hipEventDisableTiming)) != hipSuccess ||
      (e = pool_scratch(b, C, count_blocks(C - b.base))) != hipSuccess ||
      (e = hipMalloc(&b.d_pipe, sizeof(uint32_t) * pipe_words(C))) != hipSuccess ||
      // the pipeline words of pool 0 with their spin limit; the error word starts clear
      (e = hipMemcpyAsync(b.d_pipe, a.d_pipe, sizeof(uint32_t) * 16, hipMemcpyDeviceToDevice, h->stream)) != hipSuccess)
    return fail(PAXISIM_EDEVICE, "cluster pool setup failed: %s", hipGetErrorString(e));
  return 0;
}

// Pipelined launches (serial kernels): pool 0's pipeline words with the poll limit of a chunk wait
// (sim_core.h pipe_item), and the XCD probe - workgroups must go round robin over the 8 XCDs, in any
// rotation, or the handle does not pipeline (*probe_ok).
static int pipe_setup(paxisim* h, const Knobs& kn, bool* probe_ok) {
  uint32_t*& q = h->pool[0].d_pipe;
  uint32_t xcc[64] = {0};
  const uint32_t spin = kn.has_pipe_spin ? kn.pipe_spin : PXS_PIPE_SPIN_DEFAULT;
  hipError_t e;
  if ((e = hipMalloc(&q, sizeof(uint32_t) * pipe_words(h->P.C))) != hipSuccess ||
      (e = hipMemsetAsync(q, 0, sizeof(uint32_t) * 16, h->stream)) != hipSuccess ||
      (e = hipMemcpyAsync(q + 9, &spin, sizeof spin, hipMemcpyHostToDevice, h->stream)) != hipSuccess)
    return fail(PAXISIM_EDEVICE, "pipelined launch setup failed: %s", hipGetErrorString(e));
  xcc_probe<<<64, 64, 0, h->stream>>>(q + 16);
  if ((e = hipGetLastError()) != hipSuccess ||
      (e = hipMemcpyAsync(xcc, q + 16, sizeof xcc, hipMemcpyDeviceToHost, h->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(h->stream)) != hipSuccess)
    return fail(PAXISIM_EDEVICE, "XCD probe failed: %s", hipGetErrorString(e));
  for (uint32_t b = 0; b < 64; b++)
    if ((xcc[b] & 7u) != ((xcc[0] + b) & 7u) || xcc[b] > 7u) *probe_ok = false;
  return 0;
}

// Everything of paxisim_create after `new`: the plan (create_plan.h) between the device calls it
// needs.  On a failure the caller destroys the partly built handle.
static int create_on_device(paxisim* h, const Knobs& kn, uint32_t variant, uint32_t N) {
  const paxisim_config* cfg = &h->cfg;
  Params& P = h->P;
  fill_params(P, h->zone_of, h->node_of, h->S, cfg, &h->wl, &h->fp, variant, N, kn);
  h->ops = step_ops_for(P.protocol, N, P.wlds != 0, kn.serial);
  KernelFacts kf;
  if (h->ops.attrs(&kf.vgprs, &kf.max_threads) != hipSuccess) kf.vgprs = 0;
  kf.staged = h->ops.staged;
  kf.serial = h->ops.serial;
  kf.has_pipe = h->ops.launch_pipe != nullptr;
  if (const int rc = plan_lds(P, kn, kf)) return rc;

  // the arena: sized, placed, bound.  PAXISIM_ARENA_PAD_MB reserves that much device memory first
  // and frees it once the arena is placed; PAXISIM_ARENA_CONTIG=1 asks for physically contiguous
  // memory.  Placement only.
  const ArenaSize sz = carve_arena(P, cfg->policy, nullptr, false);
  void* pad = nullptr;
  if (kn.arena_pad_mb > 0) (void)hipMalloc(&pad, (size_t)kn.arena_pad_mb << 20);
  hipError_t e = kn.arena_contig ? hipExtMallocWithFlags(&h->arena, sz.total, hipDeviceMallocContiguous)
                                 : hipMalloc(&h->arena, sz.total);
  if (pad) (void)hipFree(pad);
  if (e != hipSuccess) return fail(PAXISIM_ENOMEM, "hipMalloc(%zu bytes) failed: %s", sz.total, hipGetErrorString(e));
  h->arena_bytes = sz.total;
  carve_arena(P, cfg->policy, (char*)h->arena, true);

  const size_t C = P.C;
  if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipMalloc(&h->d_scratch, sizeof(uint64_t) * 64)) != hipSuccess ||
      (e = pool_scratch(h->pool[0], C, count_blocks(cfg->clusters))) != hipSuccess ||
      (e = hipMalloc(&h->d_faults, sizeof(DevFault) * PAXISIM_MAX_FAULTS)) != hipSuccess ||
      (e = hipMemsetAsync(h->arena, 0, sz.zero_bytes, h->stream)) != hipSuccess)
    return fail(PAXISIM_EDEVICE, "device setup failed: %s", hipGetErrorString(e));
  if (P.move_every) {   // the moving-Mu tables (the caller's buffer is not kept)
    const size_t mb = (size_t)P.move_tables * PAXISIM_MAX_KEYS * sizeof(uint32_t);
    if ((e = hipMalloc(&h->d_move, mb)) != hipSuccess ||
        (e = hipMemcpy(h->d_move, h->wl.move_cdf, mb, hipMemcpyHostToDevice)) != hipSuccess)
      return fail(PAXISIM_EDEVICE, "move_cdf upload failed: %s", hipGetErrorString(e));
    P.move_cdf = h->d_move;
  }
  h->wl.move_cdf = nullptr;
  P.faults = h->d_faults;
  P.bound = h->pool[0].d_cmp;
  h->pool[0].stream = h->stream;
  h->pool[0].end = (uint32_t)C;

  bool probe_ok = true;
  if (plan_pipe(kn, kf) > 1)
    if (const int rc = pipe_setup(h, kn, &probe_ok)) return rc;
  const Schedule sc = plan_schedule(P, kn, kf, h->S, probe_ok);
  P.compact = sc.compact;
  h->late_until = sc.late_until;
  h->pipe_max = sc.pipe_max;
  h->cmp_every = sc.cmp_every;
  h->pipe_slots = kn.pipe_slots;
  if (const int rc = pools_setup(h, kn)) return rc;
  // the plan stands: a handle of the fixed shape takes the unit compiled for it (same layout, same
  // launch shape; the scripted faults of a handle being created are none yet)
  h->shape_fit = !(shape_misfit(cfg, &h->wl, 0u, ShapeKnobs{kn.serial, kn.shape}, P.packed != 0) & ~SHAPE_NFAULTS);
  if (h->shape_fit) select_unit(h);

  // every pool's bound: the clusters of its region
  uint32_t b0 = (uint32_t)cfg->clusters;
  h->bound_host = b0;
  for (uint32_t p = h->npools; p-- > 1 && e == hipSuccess;)
    e = hipMemcpyAsync(h->pool[p].d_cmp, &b0, sizeof b0, hipMemcpyHostToDevice, h->stream);
  if (h->npools > 1) b0 = h->pool[0].end;
  if (e == hipSuccess) e = hipMemcpyAsync(h->pool[0].d_cmp, &b0, sizeof b0, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) init_kernel<<<(unsigned)((C + 255) / 256), 256, 0, h->stream>>>(P);
  if (e != hipSuccess || (e = hipGetLastError()) != hipSuccess || (e = hipStreamSynchronize(h->stream)) != hipSuccess)
    return fail(PAXISIM_EDEVICE, "init kernel failed: %s", hipGetErrorString(e));
  return 0;
}

extern "C" int paxisim_create(const paxisim_config* cfg, const paxisim_workload* wl, const paxisim_fault_process* fp,
                              paxisim** out) {
  if (!cfg || !wl || !out) return fail(PAXISIM_EINVAL, "null argument");
  // M2Paxos and KPaxos are per-key Paxos like WPaxos: same kernel and state, a
  // different request path and quorums (P.variant)
  paxisim_config ncfg = *cfg;
  const uint32_t variant = cfg->protocol;
  if (variant == PAXISIM_M2PAXOS || variant == PAXISIM_KPAXOS) ncfg.protocol = PAXISIM_WPAXOS;
  cfg = &ncfg;
  paxisim_fault_process nofp;
  memset(&nofp, 0, sizeof nofp);
  if (!fp) fp = &nofp;
  const Knobs kn = knobs_from_env();
  uint32_t N = 0;
  if (const int rc = check_config(cfg, wl, fp, kn, &N)) return rc;
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (cfg->device < 0 || cfg->device >= ndev) return fail(PAXISIM_EDEVICE, "device %d not present (%d visible)", cfg->device, ndev);
  HIPCHK(hipSetDevice(cfg->device));

  paxisim* h = new (std::nothrow) paxisim();
  if (!h) return fail(PAXISIM_ENOMEM, "oom");
  h->cfg = *cfg;
  h->wl = *wl;
  h->fp = *fp;
  h->kn = kn;
  if (const int rc = create_on_device(h, kn, variant, N)) {
    paxisim_destroy(h);
    return rc;
  }
  *out = h;
  return 0;
}

extern "C" int paxisim_fault_add(paxisim* h, const paxisim_fault* f) {
  if (!h || !f) return fail(PAXISIM_EINVAL, "null argument");
  if (h->faults.size() == PAXISIM_MAX_FAULTS) return fail(PAXISIM_EINVAL, "fault table full");
  if (f->kind > PAXISIM_FAULT_CRASH || f->src >= h->P.N || (f->dst != PAXISIM_ALL_DST && f->dst >= h->P.N))
    return fail(PAXISIM_EINVAL, "bad fault");
  if (f->kind == PAXISIM_FAULT_SLOW && f->param > h->cfg.max_delay)
    return fail(PAXISIM_EINVAL, "slow delay exceeds max_delay");
  if (const int jrc = enter(h)) return jrc;
  h->faults.push_back(dev_fault(*f));
  HIPCHK(hipMemcpyAsync(h->d_faults, h->faults.data(), h->faults.size() * sizeof(DevFault),
                        hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->P.nfaults = (uint32_t)h->faults.size();
  if (h->fixed) select_unit(h);   // a scripted fault leaves the fixed shape: the generic unit from the next launch on
  return 0;
}

extern "C" int paxisim_step_unit(paxisim* h, uint32_t* unit) {
  if (!h || !unit) return fail(PAXISIM_EINVAL, "null argument");
  *unit = h->fixed ? PAXISIM_UNIT_FIXED_PAXOS5 : PAXISIM_UNIT_GENERIC;
  return 0;
}

static hipError_t ensure_lds(paxisim* h) {
  const int lds = (int)(h->P.G * h->P.lds_bytes);
  if (h->lds_set != lds) {            // per handle, so per device
    hipError_t e = h->ops.set_lds(lds);
    if (e != hipSuccess) return e;
    h->lds_set = lds;
  }
  return hipSuccess;
}

static Region region_of(const paxisim* h, const Pool& pl) {
  return Region{pl.base / LANES, (pl.end - pl.base) / LANES, pl.d_cmp, h->pipe_slots};
}

static hipError_t launch_any(paxisim* h, const Pool& pl, uint32_t t0, uint32_t n) {
  const hipError_t e = ensure_lds(h);
  return e != hipSuccess ? e : h->ops.launch(h->P, pl.stream, t0, n, region_of(h, pl));
}

// After a pipelined launch every live tile must have run all K chunks; a tile
// that did not (a wait that gave up, or waves missing from an XCD's queue)
// sets the error word, which the host reads at the next sync (pipe_check).
__global__ void pipe_verify(const uint32_t* bound, uint32_t* q, uint32_t K, uint32_t tile0) {
  const uint32_t tiles = (*bound + LANES - 1u) / LANES;   // the pool's live tiles: [tile0, tiles)
  for (uint32_t i = tile0 + blockIdx.x * blockDim.x + threadIdx.x; i < tiles; i += gridDim.x * blockDim.x)
    if (q[16 + i] != K) atomicOr(&q[8], 2u);
}

// K chunks of n steps in one pipelined launch (sim_core.h sim_serial_pipe)
static hipError_t launch_pipe(paxisim* h, const Pool& pl, uint32_t t0, uint32_t n, uint32_t K) {
  hipError_t e = ensure_lds(h);          // the serial instances set both kernels' ceilings
  if (e != hipSuccess) return e;
  const Region rg = region_of(h, pl);
  // tickets and chunk counts restart; the error word q[8] is sticky (cleared at create only)
  if ((e = hipMemsetAsync(pl.d_pipe, 0, sizeof(uint32_t) * 8, pl.stream)) != hipSuccess ||
      (e = hipMemsetAsync(pl.d_pipe + 16 + rg.tile0, 0, sizeof(uint32_t) * rg.tiles, pl.stream)) != hipSuccess)
    return e;
  if ((e = h->ops.launch_pipe(h->P, pl.stream, t0, n, K, pl.d_pipe, rg)) != hipSuccess) return e;
  pipe_verify<<<64, 256, 0, pl.stream>>>(pl.d_cmp, pl.d_pipe, K, rg.tile0);
  return hipGetLastError();
}

// a pipelined launch whose wait gave up (q[9], PAXISIM_PIPE_SPIN) left its tiles unstepped: fail loudly
// The copy is ordered on h->stream (a non-blocking stream: a null-stream
// hipMemcpy would not wait for the launches in flight), so the word read is
// the one every earlier launch left.  Every readout entry point calls this
// first, so no caller gets stats or state of a step that did not fully run.
// Each pool's words are read on that pool's stream; the error is the handle's, whichever pool set it.
static int pipe_check(paxisim* h) {
  if (!h->pool[0].d_pipe) return 0;
  uint32_t w[8] = {0};   // q[8..16): error word, spin limit, the first give-up
  for (uint32_t p = 0; p < h->npools && !w[0]; p++) {
    HIPCHK(hipMemcpyAsync(w, h->pool[p].d_pipe + 8, sizeof w, hipMemcpyDeviceToHost, h->pool[p].stream));
    HIPCHK(hipStreamSynchronize(h->pool[p].stream));
  }
  if (!w[0]) return 0;
  if (w[0] & 1u)
    return fail(PAXISIM_EDEVICE, "pipelined step launch: a chunk wait timed out (xcd %u ticket %u tile %u chunk %u: "
                "done[tile] = %u, xcd tickets taken %u)", w[2], w[3], w[4], w[5], w[6], w[7]);
  return fail(PAXISIM_EDEVICE, "pipelined step launch: a tile missed chunks");
}

// One pool's compaction at step t, on the pool's stream: its region's slots only.
static int compact(paxisim* h, Pool& pl, uint32_t t) {
  const Params& P = h->P;
  const uint64_t top = pl.end < h->cfg.clusters ? pl.end : h->cfg.clusters;   // the region's clusters end here
  const unsigned nb = (unsigned)((top - pl.base + CB - 1) / CB);
  const uint32_t base = pl.base;
  uint32_t* lo = pl.d_pairs;
  uint32_t* hi = pl.d_pairs + (P.C / 2 + LANES);
  hipStream_t st = pl.stream;
  cmp_count<<<nb, CB, 0, st>>>(P, pl.d_cmp, base);
  cmp_scan<<<1, CB, 0, st>>>(P, pl.d_cmp, nb, base);
  cmp_index<<<nb, CB, 0, st>>>(P, pl.d_cmp, lo, hi, base);
  cmp_swap<<<4096, LANES, 0, st>>>(P, pl.d_cmp, lo, hi);
  cmp_freeze<<<nb, CB, 0, st>>>(P, pl.d_cmp, t, base);
  cmp_setbound<<<1, 1, 0, st>>>(pl.d_cmp);
  if (P.phase_sort) {   // group the stepped slots by phase class
    uint32_t* ph = pl.d_ph;
    HIPCHK(hipMemsetAsync(ph, 0, PH_SUMS * sizeof(uint32_t), st));
    ph_classes<<<nb, CB, 0, st>>>(P, pl.d_cmp, ph, base);
    for (uint32_t p = 0; p < P.phase_period; p++) {   // classes 0..period-1; the quiescent ones end up last
      ph_region<<<1, 1, 0, st>>>(ph, p, base);
      ph_count<<<nb, CB, 0, st>>>(P, pl.d_cmp, ph, p, nb, base);
      ph_scan<<<1, CB, 0, st>>>(pl.d_cmp, ph, nb);
      ph_index<<<nb, CB, 0, st>>>(P, pl.d_cmp, ph, p, nb, lo, hi, base);
      cmp_swap<<<4096, LANES, 0, st>>>(P, pl.d_cmp, lo, hi);
    }
  }
  HIPCHK(hipGetLastError());
  pl.last_cmp = t;
  return 0;
}

// A request for a frozen cluster: move it to the first frozen slot, replay the
// fault process of that slot's tile up to now and step the tile again.
static int wake(paxisim* h, uint64_t cluster) {
  const Params& P = h->P;
  uint32_t bounds[MAX_POOLS] = {0, 0}, slot = 0;
  for (uint32_t p = 0; p < h->npools; p++)
    HIPCHK(hipMemcpyAsync(&bounds[p], h->pool[p].d_cmp + CM_BOUND, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(&slot, P.slot_of + cluster, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  // the pool whose region holds the slot: the cluster wakes there, at that pool's bound
  const uint32_t wp = h->npools > 1 && slot >= h->pool[1].base ? 1u : 0u;
  const Pool& pl = h->pool[wp];
  const uint32_t bound = bounds[wp];
  h->bound_host = bound;
  if (slot < bound) return 0;
  if (slot != bound) swap_one<<<1, LANES, 0, h->stream>>>(P, bound, slot);
  uint64_t end = (uint64_t)bound + LANES;
  if (end > pl.end) end = pl.end;
  if (end > h->cfg.clusters) end = h->cfg.clusters;
  const uint64_t n = (end - bound) * P.N;
  replay_kernel<<<(unsigned)((n + 63) / 64), 64, 0, h->stream>>>(P, bound, end, h->t);
  const uint32_t nb32 = (uint32_t)end;
  HIPCHK(hipMemcpyAsync(pl.d_cmp + CM_BOUND, &nb32, 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  h->bound_host = nb32;
  return 0;
}

__global__ void read_client_kernel(Params P, uint64_t cl, paxisim_worker_state* out) {
  const uint32_t w = threadIdx.x;
  if (w >= P.WK) return;
  const uint64_t c = slot_of(P, cl);
  const uint8_t* img = P.image + (c / LANES) * (size_t)P.img.bytes;
  const uint32_t wi = (w << 6) | (uint32_t)(c % LANES);
  paxisim_worker_state s;
  s.cid = reinterpret_cast<const uint32_t*>(img + P.img.off_wcur)[wi];
  s.issued = reinterpret_cast<const uint32_t*>(img + P.img.off_wiss)[wi];
  s.reply_value = P.wrep[(size_t)w * P.C + c];
  s.pad = 0;
  out[w] = s;
}

extern "C" int paxisim_read_client(paxisim* h, uint64_t cluster, paxisim_worker_state* out, uint32_t cap,
                                   uint32_t* n_out) {
  if (!h || !n_out || (cap && !out)) return fail(PAXISIM_EINVAL, "null argument");
  if (cluster >= h->cfg.clusters) return fail(PAXISIM_ERANGE, "bad cluster");
  if (const int jrc = enter(h)) return jrc;
  if (const int rc = pipe_check(h)) return rc;   // results only of launches that fully ran
  const uint32_t n = h->P.WK;
  *n_out = n;
  if (!cap || !n) return 0;
  paxisim_worker_state* d = nullptr;
  HIPCHK(hipMalloc(&d, n * sizeof(paxisim_worker_state)));
  read_client_kernel<<<1, 64, 0, h->stream>>>(h->P, cluster, d);
  hipError_t e = hipGetLastError();
  std::vector<paxisim_worker_state> tmp(n);
  if (e == hipSuccess) e = hipMemcpyAsync(tmp.data(), d, n * sizeof(paxisim_worker_state), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(PAXISIM_EDEVICE, "read_client: %s", hipGetErrorString(e));
  for (uint32_t w = 0; w < n && w < cap; w++) out[w] = tmp[w];
  return 0;
}

__global__ void read_kv_kernel(Params P, uint64_t cl, uint32_t r, uint32_t n, uint32_t* out) {
  const uint32_t k = threadIdx.x + blockIdx.x * blockDim.x;
  if (k >= n) return;
  const uint64_t c = slot_of(P, cl);
  if (P.protocol == PAXISIM_ABD)
    out[k] = reinterpret_cast<const uint32_t*>(P.image + (c / LANES) * (size_t)P.img.bytes +
                                               P.img.off_a)[((r * P.keys + k) << 6) | (c % LANES)];
  else
    out[k] = P.kv_val[((size_t)k * P.N + r) * P.C + c];
}

// Database.Get (db.go:116-121) of keys [0, n) of one replica
extern "C" int paxisim_read_kv(paxisim* h, uint64_t cluster, uint32_t replica, uint32_t* values, uint32_t n) {
  if (!h || (n && !values)) return fail(PAXISIM_EINVAL, "null argument");
  if (cluster >= h->cfg.clusters || replica >= h->P.N || n > h->P.keys) return fail(PAXISIM_ERANGE, "bad key range");
  if (h->P.protocol != PAXISIM_ABD && !h->P.kv) return fail(PAXISIM_EUNSUPP, "replicas keep no Database (config.kv = 0)");
  if (n == 0) return 0;
  if (const int jrc = enter(h)) return jrc;
  if (const int rc = pipe_check(h)) return rc;   // results only of launches that fully ran
  uint32_t* d = nullptr;
  HIPCHK(hipMalloc(&d, n * sizeof(uint32_t)));
  read_kv_kernel<<<(n + 63) / 64, 64, 0, h->stream>>>(h->P, cluster, replica, n, d);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(values, d, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(PAXISIM_EDEVICE, "read_kv: %s", hipGetErrorString(e));
  return 0;
}

extern "C" int paxisim_active_clusters(paxisim* h, uint64_t* active) {
  if (!h || !active) return fail(PAXISIM_EINVAL, "null argument");
  if (const int jrc = enter(h)) return jrc;
  if (const int rc = pipe_check(h)) return rc;   // results only of launches that fully ran
  uint32_t bounds[MAX_POOLS] = {0, 0}, bound = 0;
  for (uint32_t p = 0; p < h->npools; p++)
    HIPCHK(hipMemcpyAsync(&bounds[p], h->pool[p].d_cmp + CM_BOUND, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (uint32_t p = 0; p < h->npools; p++) bound += bounds[p] - h->pool[p].base;   // the pools' stepped slots
  h->bound_host = bound;
  *active = bound;
  return 0;
}

// b1, base1: the second pool's bound and first slot (one pool: base1 past every slot)
__global__ void activity_kernel(Params P, uint64_t lo, uint64_t n, uint32_t* out, const uint32_t* b1, uint64_t base1) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t s = slot_of(P, lo + i);
  out[i] = s < (s < base1 ? *P.bound : *b1) ? 0xFFFFFFFFu : P.frz[s];
}

extern "C" int paxisim_quorum(const paxisim_config* cfg, uint32_t kind, uint32_t ack_mask, int* satisfied) {
  if (!cfg || !satisfied) return fail(PAXISIM_EINVAL, "null argument");
  if (cfg->n_zones == 0 || cfg->n_zones > PAXISIM_MAX_ZONES || kind > PAXISIM_Q_FGRID_Q2)
    return fail(PAXISIM_EINVAL, "bad zones or quorum kind");
  uint32_t npz[PAXISIM_MAX_ZONES], zmask[PAXISIM_MAX_ZONES], N = 0;
  for (uint32_t z = 0; z < cfg->n_zones; z++) {
    if (cfg->npz[z] == 0 || N + cfg->npz[z] > PAXISIM_MAX_N) return fail(PAXISIM_EINVAL, "bad nodes per zone");
    npz[z] = cfg->npz[z];
    zmask[z] = ((1u << npz[z]) - 1u) << N;
    N += npz[z];
  }
  *satisfied = quorum_check(kind, N, cfg->n_zones, npz, zmask, cfg->fz, ack_mask & ((1u << N) - 1u)) ? 1 : 0;
  return 0;
}

extern "C" int paxisim_read_activity(paxisim* h, uint64_t lo, uint64_t n, uint32_t* frozen_at) {
  if (!h || !frozen_at) return fail(PAXISIM_EINVAL, "null argument");
  if (lo + n > h->cfg.clusters || lo + n < lo) return fail(PAXISIM_ERANGE, "cluster range");
  if (n == 0) return 0;
  if (const int jrc = enter(h)) return jrc;
  if (const int rc = pipe_check(h)) return rc;   // results only of launches that fully ran
  uint32_t* d = nullptr;
  HIPCHK(hipMalloc(&d, n * sizeof(uint32_t)));
  activity_kernel<<<(unsigned)((n + 255) / 256), 256, 0, h->stream>>>(
      h->P, lo, n, d, h->npools > 1 ? h->pool[1].d_cmp : h->P.bound, h->npools > 1 ? (uint64_t)h->pool[1].base : ~0ull);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(frozen_at, d, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(PAXISIM_EDEVICE, "read_activity: %s", hipGetErrorString(e));
  return 0;
}

extern "C" int paxisim_step(paxisim* h, uint32_t nsteps) {
  if (!h) return fail(PAXISIM_EINVAL, "null handle");
  if ((uint64_t)h->t + nsteps >= T_MAX) return fail(PAXISIM_EINVAL, "step counter would exceed 2^28");
  HIPCHK(hipSetDevice(h->cfg.device));
  if (h->npools > 1 && h->main_ahead) {   // the pools' streams wait for what the handle's stream did since
    HIPCHK(hipEventRecord(h->ev_main, h->stream));
    for (uint32_t p = 0; p < h->npools; p++) HIPCHK(hipStreamWaitEvent(h->pool[p].stream, h->ev_main, 0));
    h->main_ahead = false;
  }
  // every pool's launches of this call (pool_plan.h): chunks fused up to pipe_max, none past a due
  // compaction of that pool; all pools end at h->t + nsteps.  Nothing here waits for the device
  // or makes one pool's stream wait for the other's.
  PoolPlanIn in;
  in.t = h->t;
  in.nsteps = nsteps;
  in.S = h->S;
  in.pipe_max = h->pipe_max;
  in.cmp_every = h->cmp_every;
  in.late_until = h->late_until;
  in.compact = h->P.compact != 0;
  in.npools = h->npools;
  for (uint32_t p = 0; p < h->npools; p++) in.last_cmp[p] = h->pool[p].last_cmp;
  h->pools_ahead = true;
  for (const PoolLaunch& L : pool_plan(in)) {
    Pool& pl = h->pool[L.pool];
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a));
    hipError_t e = hipEventCreate(&b);
    if (e != hipSuccess) {
      (void)hipEventDestroy(a);
      return fail(PAXISIM_EDEVICE, "hipEventCreate: %s", hipGetErrorString(e));
    }
    if ((e = hipEventRecord(a, pl.stream)) == hipSuccess &&
        (e = L.chunks > 1 ? launch_pipe(h, pl, L.t0, L.n, L.chunks) : launch_any(h, pl, L.t0, L.n)) == hipSuccess)
      e = hipEventRecord(b, pl.stream);
    if (e != hipSuccess) {              // no leaked events on the error path
      (void)hipEventDestroy(a);
      (void)hipEventDestroy(b);
      return fail(PAXISIM_EDEVICE, "step launch: %s", hipGetErrorString(e));
    }
    h->evs.emplace_back(a, b);
    h->launches++;
    if (L.compact) {
      const int rc = compact(h, pl, L.t0 + L.chunks * L.n);
      if (rc) return rc;
    }
    if (h->evs.size() >= 256) {
      int rc = flush_events(h);
      if (rc) return rc;
    }
  }
  h->t += nsteps;
  return 0;
}

extern "C" int paxisim_sync(paxisim* h) {
  if (!h) return fail(PAXISIM_EINVAL, "null handle");
  if (const int jrc = enter(h)) return jrc;
  for (uint32_t p = 0; p < h->npools; p++) HIPCHK(hipStreamSynchronize(h->pool[p].stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return pipe_check(h);
}

extern "C" int paxisim_kernel_time(paxisim* h, double* ms, uint64_t* launches, int reset) {
  if (!h) return fail(PAXISIM_EINVAL, "null handle");
  if (const int jrc = enter(h)) return jrc;
  int rc = flush_events(h);
  if (rc) return rc;
  if (ms) *ms = h->kernel_ms;
  if (launches) *launches = h->launches;
  if (reset) {
    h->kernel_ms = 0;
    h->launches = 0;
  }
  return 0;
}

extern "C" int paxisim_inject(paxisim* h, uint64_t cluster, uint32_t replica, uint32_t cid) {
  if (!h) return fail(PAXISIM_EINVAL, "null handle");
  if (cluster >= h->cfg.clusters || replica >= h->P.N || cid < 1 || cid > CMD_MASK)
    return fail(PAXISIM_EINVAL, "bad inject (cluster %llu, replica %u, cid %u)", (unsigned long long)cluster,
                replica, cid);
  if (const int jrc = enter(h)) return jrc;
  if (h->P.compact) {
    const int rc = wake(h, cluster);
    if (rc) return rc;
  }
  uint32_t st = 0;
  inject_kernel<<<1, 64, 0, h->stream>>>(h->P, cluster, replica, h->t % h->P.D, cid, (uint32_t*)h->d_scratch);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(&st, h->d_scratch, sizeof st, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (st) return fail(PAXISIM_EINVAL, "client mailbox full");
  return 0;
}

extern "C" int paxisim_read_inbox(paxisim* h, uint64_t cluster, uint32_t replica, paxisim_inbox_record* out,
                                  uint32_t cap, uint32_t* n_out) {
  if (!h || !n_out || (cap && !out)) return fail(PAXISIM_EINVAL, "null argument");
  if (cluster >= h->cfg.clusters || replica >= h->P.N) return fail(PAXISIM_ERANGE, "bad inbox");
  if (const int jrc = enter(h)) return jrc;
  if (const int rc = pipe_check(h)) return rc;   // results only of launches that fully ran
  HIPCHK(hipStreamSynchronize(h->stream));
  const uint32_t maxn = h->P.NS * h->P.M;   // a bucket set holds at most this many
  paxisim_inbox_record* d = nullptr;
  HIPCHK(hipMalloc(&d, maxn * sizeof(paxisim_inbox_record) + 64));
  uint32_t* dn = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(d) + maxn * sizeof(paxisim_inbox_record));
  read_inbox_kernel<<<1, 64, 0, h->stream>>>(h->P, cluster, replica, h->t % h->P.D, d, maxn, dn);
  hipError_t e = hipGetLastError();
  uint32_t n = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&n, dn, sizeof n, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e == hipSuccess && cap)
    e = hipMemcpy(out, d, (n < cap ? n : cap) * sizeof(paxisim_inbox_record), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(PAXISIM_EDEVICE, "read_inbox: %s", hipGetErrorString(e));
  *n_out = n;
  return 0;
}

extern "C" int paxisim_commands(paxisim* h, uint64_t cluster, const uint32_t* cids, uint32_t n, uint32_t* keys,
                                uint32_t* writes) {
  if (!h || (n && (!cids || !keys || !writes))) return fail(PAXISIM_EINVAL, "null argument");
  if (cluster >= h->cfg.clusters) return fail(PAXISIM_ERANGE, "bad cluster");
  if (n == 0) return 0;
  if (const int jrc = enter(h)) return jrc;
  if (const int rc = pipe_check(h)) return rc;   // results only of launches that fully ran
  uint32_t* d = nullptr;
  HIPCHK(hipMalloc(&d, 3ull * n * sizeof(uint32_t)));
  hipError_t e = hipMemcpyAsync(d, cids, n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) {
    command_kernel<<<(n + 255) / 256, 256, 0, h->stream>>>(h->P, cluster, d, n, d + n, d + 2 * n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(keys, d + n, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(writes, d + 2 * n, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(PAXISIM_EDEVICE, "commands: %s", hipGetErrorString(e));
  return 0;
}

extern "C" int paxisim_deliver(paxisim* h, uint64_t cluster, uint32_t replica, uint32_t src,
                               const paxisim_inbox_record* recs, uint32_t n) {
  if (!h || (n && !recs)) return fail(PAXISIM_EINVAL, "null argument");
  if (cluster >= h->cfg.clusters || replica >= h->P.N || src > h->P.N)
    return fail(PAXISIM_EINVAL, "bad deliver (cluster %llu, replica %u, src %u)", (unsigned long long)cluster,
                replica, src);
  if (n == 0) return 0;
  if (n > h->P.M) return fail(PAXISIM_EINVAL, "mailbox full");
  if (const int jrc = enter(h)) return jrc;
  if (h->P.compact) {
    const int rc = wake(h, cluster);
    if (rc) return rc;
  }
  paxisim_inbox_record* d = nullptr;
  HIPCHK(hipMalloc(&d, n * sizeof(paxisim_inbox_record)));
  hipError_t e = hipMemcpyAsync(d, recs, n * sizeof(paxisim_inbox_record), hipMemcpyHostToDevice, h->stream);
  uint32_t st = 0;
  if (e == hipSuccess) {
    deliver_kernel<<<1, 64, 0, h->stream>>>(h->P, cluster, replica, src, h->t % h->P.D, d, n,
                                            (uint32_t*)h->d_scratch);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&st, h->d_scratch, sizeof st, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(PAXISIM_EDEVICE, "deliver: %s", hipGetErrorString(e));
  if (st) return fail(PAXISIM_EINVAL, "mailbox full");
  return 0;
}

extern "C" int paxisim_read_log(paxisim* h, uint64_t cluster, uint32_t replica, uint32_t key, int32_t slot_lo,
                                uint32_t n, paxisim_log_entry* out) {
  if (!h || !out) return fail(PAXISIM_EINVAL, "null argument");
  if (h->cfg.protocol == PAXISIM_EPAXOS || h->cfg.protocol == PAXISIM_ABD)   // no Paxos window in the image
    return fail(PAXISIM_EUNSUPP, "read_log: the protocol keeps no Paxos log (EPaxos: read_instances)");
  if (cluster >= h->cfg.clusters || replica >= h->P.N || key >= h->P.NK) return fail(PAXISIM_ERANGE, "bad entry");
  if (n == 0) return 0;
  if (const int jrc = enter(h)) return jrc;
  if (const int rc = pipe_check(h)) return rc;   // results only of launches that fully ran
  paxisim_log_entry* d = nullptr;
  HIPCHK(hipMalloc(&d, n * sizeof(paxisim_log_entry)));
  read_log_kernel<<<(n + 63) / 64, 64, 0, h->stream>>>(h->P, cluster, replica, key, slot_lo, n, d);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(out, d, n * sizeof(paxisim_log_entry), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(PAXISIM_EDEVICE, "read_log: %s", hipGetErrorString(e));
  for (uint32_t i = 0; i < n; i++) out[i].ballot = expand_ballot(h, (uint32_t)out[i].ballot);
  return 0;
}

extern "C" int paxisim_stats_get(paxisim* h, paxisim_stats* out) {
  if (!h || !out) return fail(PAXISIM_EINVAL, "null argument");
  if (const int jrc = enter(h)) return jrc;
  if (const int rc = pipe_check(h)) return rc;   // results only of launches that fully ran
  uint64_t red[NRED];
  HIPCHK(hipMemsetAsync(h->d_scratch, 0, sizeof(uint64_t) * NRED, h->stream));
  stats_kernel<<<(unsigned)(h->P.C / 256 + 1), 256, 0, h->stream>>>(h->P, h->d_scratch);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(red, h->d_scratch, sizeof red, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  memset(out, 0, sizeof *out);
  out->steps = h->t;
  out->clusters = h->cfg.clusters;
  for (int k = 0; k < PAXISIM_NMSG; k++) {
    out->delivered[k] = red[ST_DELIV0 + k];
    out->delivered_total += red[ST_DELIV0 + k];
  }
  out->client_requests = red[ST_CLIENT];
  out->sent = red[ST_SENT];
  out->dropped = red[ST_DROPPED];
  out->discarded = red[ST_DISCARDED];
  out->commits = red[ST_COMMITS];
  out->replies = red[ST_REPLIES];
  out->agree_compared = red[ST_AGC];
  out->agree_missed = red[ST_AGM];
  out->agree_mismatch = red[ST_AGB];
  for (int b = 0; b < 8; b++) out->flagged[b] = red[NSTAT + b];
  return 0;
}

extern "C" int paxisim_read_state(paxisim* h, uint64_t lo, uint64_t n, paxisim_replica_state* out) {
  if (!h || !out) return fail(PAXISIM_EINVAL, "null argument");
  if (lo + n > h->cfg.clusters || lo + n < lo) return fail(PAXISIM_ERANGE, "cluster range");
  if (n == 0) return 0;
  if (const int jrc = enter(h)) return jrc;
  if (const int rc = pipe_check(h)) return rc;   // results only of launches that fully ran
  const size_t cnt = (size_t)n * h->P.N;
  paxisim_replica_state* d = nullptr;
  HIPCHK(hipMalloc(&d, cnt * sizeof(paxisim_replica_state)));
  gather_kernel<<<(unsigned)((cnt + 255) / 256), 256, 0, h->stream>>>(h->P, lo, n, d);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(out, d, cnt * sizeof(paxisim_replica_state), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(PAXISIM_EDEVICE, "read_state: %s", hipGetErrorString(e));
  for (size_t i = 0; i < cnt; i++) out[i].ballot = expand_ballot(h, (uint32_t)out[i].ballot);
  return 0;
}

extern "C" int paxisim_read_instances(paxisim* h, uint64_t lo, uint64_t n, paxisim_instance_state* out) {
  if (!h || !out) return fail(PAXISIM_EINVAL, "null argument");
  if (lo + n > h->cfg.clusters || lo + n < lo) return fail(PAXISIM_ERANGE, "cluster range");
  if (n == 0) return 0;
  if (const int jrc = enter(h)) return jrc;
  if (const int rc = pipe_check(h)) return rc;   // results only of launches that fully ran
  const uint32_t ni = h->P.protocol == PAXISIM_EPAXOS ? h->P.N * h->P.N : h->P.NI;   // per cluster; EPaxos: (replica, owner log)
  const size_t cnt = (size_t)n * ni;
  paxisim_instance_state* d = nullptr;
  HIPCHK(hipMalloc(&d, cnt * sizeof(paxisim_instance_state)));
  gather_inst_kernel<<<(unsigned)((cnt + 255) / 256), 256, 0, h->stream>>>(h->P, lo, n, d);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(out, d, cnt * sizeof(paxisim_instance_state), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(PAXISIM_EDEVICE, "read_instances: %s", hipGetErrorString(e));
  for (size_t i = 0; i < cnt; i++) out[i].ballot = expand_ballot(h, (uint32_t)out[i].ballot);
  return 0;
}

extern "C" int paxisim_check(paxisim* h, uint64_t* violations) {
  if (!h || !violations) return fail(PAXISIM_EINVAL, "null argument");
  if (const int jrc = enter(h)) return jrc;
  if (const int rc = pipe_check(h)) return rc;   // results only of launches that fully ran
  HIPCHK(hipMemsetAsync(h->d_scratch, 0, sizeof(uint64_t), h->stream));
  check_kernel<<<(unsigned)(h->P.C / 256 + 1), 256, 0, h->stream>>>(h->P, h->d_scratch);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(violations, h->d_scratch, sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int paxisim_occupancy(paxisim* h, int* blocks_per_cu, uint32_t* lds_bytes, uint32_t* staged) {
  if (!h || !blocks_per_cu) return fail(PAXISIM_EINVAL, "null argument");
  if (const int jrc = enter(h)) return jrc;
  HIPCHK(h->ops.occupancy(h->P, blocks_per_cu));
  *blocks_per_cu *= (int)h->P.G;    // 64-cluster tiles resident per CU
  if (lds_bytes) *lds_bytes = h->P.lds_bytes;
  if (staged) *staged = h->P.J;
  return 0;
}

extern "C" int paxisim_device_bytes(paxisim* h, uint64_t* bytes) {
  if (!h || !bytes) return fail(PAXISIM_EINVAL, "null argument");
  *bytes = h->arena_bytes + h->lat_bytes + h->ch_bytes + h->mv_bytes + h->tr_bytes;
  return 0;
}

// ---------------------------------------------------------------------------
// Client request latency (include/paxisim.h, DESIGN.md §3.12, lat_kernel.h)
// ---------------------------------------------------------------------------
static size_t lat_acc_words(const Params& P) { return (size_t)LAT_SLICES * P.WK * lat_row(P.lat_bins); }

extern "C" int paxisim_latency_enable(paxisim* h, uint32_t bins) {
  if (!h) return fail(PAXISIM_EINVAL, "null handle");
  if (bins < 16u || bins > PAXISIM_LAT_MAX_BINS || (bins & (bins - 1u)))
    return fail(PAXISIM_EINVAL, "latency bins must be a power of two in [16, %u]", PAXISIM_LAT_MAX_BINS);
  if (h->P.lat_bins) return fail(PAXISIM_EINVAL, "latency is already enabled");
  if (h->t) return fail(PAXISIM_EINVAL, "latency can only be enabled before the first step");
  if (const int jrc = enter(h)) return jrc;
  // the recording build of the handle's kernel: the same instance, so the launch shape chosen at create fits it
  const StepOps ops = lat_step_ops_for(h->P.protocol, h->P.N, h->P.wlds != 0, h->ops.serial);
  int vgprs = 0, maxthr = 0;
  if (!ops.launch || ops.serial != h->ops.serial || ops.staged != h->ops.staged ||
      ops.attrs(&vgprs, &maxthr) != hipSuccess || (!ops.serial && h->P.G * h->P.N * LANES > (uint32_t)maxthr))
    return fail(PAXISIM_EUNSUPP, "no latency-recording build of this handle's step kernel");
  Params P = h->P;
  P.lat_bins = bins;
  // every worker present at create issued its first request at step 0: the zeroed stamps
  const size_t sb = sizeof(uint32_t) * P.WK * P.C, ab = sizeof(unsigned long long) * lat_acc_words(P);
  const size_t ob = sizeof(unsigned long long) * P.WK * lat_row(bins);
  unsigned long long* o = nullptr;
  hipError_t e;
  if ((e = hipMalloc(&P.lat_stamp, sb)) != hipSuccess || (e = hipMalloc(&P.lat_acc, ab)) != hipSuccess ||
      (e = hipMalloc(&o, ob)) != hipSuccess || (e = hipMemsetAsync(P.lat_stamp, 0, sb, h->stream)) != hipSuccess ||
      (e = hipMemsetAsync(P.lat_acc, 0, ab, h->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(h->stream)) != hipSuccess) {
    if (P.lat_stamp) (void)hipFree(P.lat_stamp);
    if (P.lat_acc) (void)hipFree(P.lat_acc);
    if (o) (void)hipFree(o);
    return fail(PAXISIM_ENOMEM, "latency buffers (%zu bytes): %s", sb + ab + ob, hipGetErrorString(e));
  }
  h->P = P;
  h->ops = ops;
  h->lds_set = -1;        // the dynamic-LDS ceiling is per kernel
  if (h->fixed) select_unit(h);   // the recording twin of the fixed-shape unit
  h->d_lat_out = o;
  h->lat_bytes = sb + ab + ob;
  return 0;
}

extern "C" int paxisim_latency_reset(paxisim* h) {
  if (!h) return fail(PAXISIM_EINVAL, "null handle");
  if (!h->P.lat_bins) return fail(PAXISIM_EINVAL, "latency is not enabled");
  if (const int jrc = enter(h)) return jrc;
  // on the launch stream: after every step launched so far, before the next one
  HIPCHK(hipMemsetAsync(h->P.lat_acc, 0, sizeof(unsigned long long) * lat_acc_words(h->P), h->stream));
  return 0;
}

extern "C" int paxisim_latency_get(paxisim* h, uint32_t worker, paxisim_latency* out, uint64_t* hist) {
  if (!h || !out) return fail(PAXISIM_EINVAL, "null argument");
  if (!h->P.lat_bins) return fail(PAXISIM_EINVAL, "latency is not enabled");
  if (worker != PAXISIM_ALL_WORKERS && worker >= h->P.WK) return fail(PAXISIM_EINVAL, "no worker %u", worker);
  if (const int jrc = enter(h)) return jrc;
  if (const int rc = pipe_check(h)) return rc;   // results only of launches that fully ran
  const uint32_t bins = h->P.lat_bins;
  const size_t row = lat_row(bins), n = (size_t)h->P.WK * row;
  lat_reduce<<<(unsigned)((n + 255) / 256), 256, 0, h->stream>>>(h->P, h->d_lat_out);
  HIPCHK(hipGetLastError());
  std::vector<unsigned long long> acc(n);
  HIPCHK(hipMemcpyAsync(acc.data(), h->d_lat_out, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  memset(out, 0, sizeof *out);
  out->bins = bins;
  out->min = 0xFFFFFFFFu;
  if (hist) memset(hist, 0, sizeof(uint64_t) * bins);
  for (uint32_t w = 0; w < h->P.WK; w++) {
    if (worker != PAXISIM_ALL_WORKERS && w != worker) continue;
    const unsigned long long* a = acc.data() + (size_t)w * row;
    uint64_t cnt = a[bins + LAT_OVF];
    for (uint32_t b = 0; b < bins; b++) {
      cnt += a[b];
      if (hist) hist[b] += a[b];
    }
    out->count += cnt;
    out->sum += a[bins + LAT_SUM];
    out->overflow += a[bins + LAT_OVF];
    if (cnt) {
      out->min = std::min(out->min, 0xFFFFFFFFu - (uint32_t)a[bins + LAT_NMIN]);
      out->max = std::max(out->max, (uint32_t)a[bins + LAT_MAX]);
    }
  }
  return 0;
}

extern "C" int paxisim_latency_stat_of(const paxisim_latency* l, const uint64_t* hist, double step_ms,
                                       paxisim_latency_stat* out) {
  if (!l || !hist || !out) return fail(PAXISIM_EINVAL, "null argument");
  if (l->bins > PAXISIM_LAT_MAX_BINS) return fail(PAXISIM_ERANGE, "bins exceeds PAXISIM_LAT_MAX_BINS");
  if (l->count == 0) return fail(PAXISIM_EINVAL, "no samples");
  memset(out, 0, sizeof *out);
  out->size = l->count;
  out->mean = (double)l->sum * step_ms / (double)l->count;
  out->min = l->min * step_ms;
  out->max = l->max * step_ms;
  out->exact = 1;
  // stat.go:44-66: element int(p * size) of the sorted samples
  const double ps[4] = {0.5, 0.95, 0.99, 0.999};
  double* dst[4] = {&out->median, &out->p95, &out->p99, &out->p999};
  for (int k = 0; k < 4; k++) {
    uint64_t idx = (uint64_t)(ps[k] * (double)l->count);
    if (idx >= l->count) idx = l->count - 1;
    uint64_t cum = 0;
    uint32_t b = 0;
    for (; b < l->bins; b++) {
      cum += hist[b];
      if (idx < cum) break;
    }
    if (b < l->bins) {
      *dst[k] = b * step_ms;
    } else {                      // inside the overflow bin: only its bounds are known
      *dst[k] = out->max;
      out->exact = 0;
    }
  }
  return 0;
}

// Completed ABD operations of one cluster, 5 words per op {key, is_write,
// value, start, end}, replicas in index order, each in completion order.
extern "C" int paxisim_history(paxisim* h, uint64_t cluster, uint32_t* buf, uint32_t cap_ops, uint32_t* n_out) {
  if (!h || !n_out) return fail(PAXISIM_EINVAL, "null argument");
  if (cluster >= h->cfg.clusters) return fail(PAXISIM_ERANGE, "cluster");
  if (const int jrc = enter(h)) return jrc;
  if (const int rc = pipe_check(h)) return rc;   // results only of launches that fully ran
  HIPCHK(hipStreamSynchronize(h->stream));   // step kernels run on the non-blocking h->stream
  const Params& P = h->P;
  std::vector<uint32_t> len(P.N);
  for (uint32_t r = 0; r < P.N; r++)
    HIPCHK(hipMemcpy(&len[r], &P.execute[rc_host(P, r, cluster)], 4, hipMemcpyDeviceToHost));
  uint32_t n = 0;
  for (uint32_t r = 0; r < P.N && P.H; r++) {
    std::vector<uint4> tmp(len[r]);
    if (len[r])
      HIPCHK(hipMemcpy(tmp.data(), &P.hist[((size_t)r * P.C + cluster) * P.H], len[r] * sizeof(uint4),
                       hipMemcpyDeviceToHost));
    for (uint32_t j = 0; j < len[r]; j++, n++) {
      if (!buf || n >= cap_ops) continue;
      uint32_t* o = buf + 5 * (size_t)n;
      o[0] = tmp[j].x & 0x7FFFFFFFu;
      o[1] = tmp[j].x >> 31;
      o[2] = tmp[j].y;
      o[3] = tmp[j].z;
      o[4] = tmp[j].w;
    }
  }
  *n_out = n;
  return 0;
}

// History.ReadFile (history.go:115-178) into the device history of one replica.
extern "C" int paxisim_history_load(paxisim* h, uint64_t cluster, uint32_t replica, const uint32_t* ops, uint32_t n) {
  if (!h || (n && !ops)) return fail(PAXISIM_EINVAL, "null argument");
  if (cluster >= h->cfg.clusters || replica >= h->P.N) return fail(PAXISIM_ERANGE, "bad replica");
  if (h->P.protocol != PAXISIM_ABD) return fail(PAXISIM_EUNSUPP, "op history is kept by ABD only");
  if (n > h->P.H) return fail(PAXISIM_EINVAL, "%u ops exceed history capacity %u", n, h->P.H);
  if (const int jrc = enter(h)) return jrc;
  HIPCHK(hipStreamSynchronize(h->stream));
  const Params& P = h->P;
  std::vector<uint4> tmp(n ? n : 1);
  for (uint32_t j = 0; j < n; j++) {
    const uint32_t* o = ops + 5 * (size_t)j;
    if (o[0] >= h->P.keys || o[1] > 1u) return fail(PAXISIM_EINVAL, "op %u: bad key (keys = %u) or is_write", j, h->P.keys);
    tmp[j] = make_uint4(o[0] | (o[1] << 31), o[2], o[3], o[4]);
  }
  if (n)
    HIPCHK(hipMemcpy(&P.hist[((size_t)replica * P.C + cluster) * P.H], tmp.data(), n * sizeof(uint4),
                     hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(&P.execute[rc_host(P, replica, cluster)], &n, 4, hipMemcpyHostToDevice));
  return 0;
}

// History.Linearizable over the history source S of every cluster (lin_kernel.h): LinAbd, the
// replicas' completed ABD ops, or LinClient, the workers' ops of any protocol (chist_kernel.h).
template <class S>
static int lin_scan(paxisim* h, uint64_t* anomalies, uint64_t* ops, uint64_t* skipped, uint32_t* mark = nullptr,
                    uint32_t mark_bit = 0) {
  if (const int jrc = enter(h)) return jrc;
  if (const int rc = pipe_check(h)) return rc;   // results only of launches that fully ran
  HIPCHK(hipStreamSynchronize(h->stream));
  const Params& P = h->P;
  // clusters per launch: each gets a stage of sources * per_source ops (ABD: N*H; its history grouped by key).
  // The stage takes up to a quarter of the free HBM (2-16 GiB): fewer, longer
  // launches leave less of each launch's last round of workgroups idle
  // (config 3: 21 -> 6 launches); PAXISIM_LIN_STAGE_MB overrides (A/B).
  const size_t cap = (size_t)S::sources(P) * S::per_source(P);
  size_t budget = 2ull << 30, freeb = 0, totb = 0;
  if (hipMemGetInfo(&freeb, &totb) == hipSuccess) budget = std::max(budget, std::min<size_t>(freeb / 4, 16ull << 30));
  if (const char* e = getenv("PAXISIM_LIN_STAGE_MB")) budget = std::max<size_t>(1, (size_t)atoll(e)) << 20;
  const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(P.clusters, budget / (cap * sizeof(uint4))));
  uint4* stage = nullptr;
  uint2* big = nullptr;
  unsigned long long* out = nullptr;
  uint8_t* bws = nullptr;
  size_t bws_bytes = 0;
  const size_t nout = LIN_NOUT + 8;
  auto cleanup = [&]() {
    (void)hipFree(stage);
    (void)hipFree(big);
    (void)hipFree(out);
    (void)hipFree(bws);
  };
  hipError_t e = hipMalloc(&stage, chunk * cap * sizeof(uint4));
  if (e == hipSuccess) e = hipMalloc(&big, chunk * P.keys * sizeof(uint2));
  if (e == hipSuccess) e = hipMalloc(&out, nout * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemsetAsync(out, 0, nout * sizeof(unsigned long long), h->stream);
  const uint32_t lds = LIN_LW * LIN_SORT_BYTES;
  unsigned long long tot[LIN_NOUT] = {0};
  for (uint64_t c0 = 0; e == hipSuccess && c0 < P.clusters; c0 += chunk) {
    const uint64_t nc = std::min<uint64_t>(chunk, P.clusters - c0);
    if ((e = hipMemsetAsync(out + LIN_BIG, 0, 2 * sizeof(unsigned long long), h->stream)) != hipSuccess) break;
    lin_cluster_kernel<S><<<(unsigned)nc, LIN_LW * 64, lds, h->stream>>>(P, c0, stage, out, big, mark, mark_bit);
    unsigned long long bc[2] = {0, 0};
    if ((e = hipGetLastError()) != hipSuccess) break;
    if ((e = hipMemcpyAsync(bc, out + LIN_BIG, sizeof bc, hipMemcpyDeviceToHost, h->stream)) != hipSuccess) break;
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) break;
    if (bc[0]) {   // partitions above LIN_SMAX ops: one wave each, scratch in HBM
      tot[LIN_BIG] += bc[0];
      tot[LIN_NMAX] = std::max<unsigned long long>(tot[LIN_NMAX], bc[1]);
      const uint32_t nw = (uint32_t)((bc[1] + 63u) / 64u);     // bc[1] <= LIN_VMAX (larger: skipped)
      const size_t per = lin_scratch_bytes(nw, true);
      const uint32_t waves = (uint32_t)std::max<unsigned long long>(
          1, std::min<unsigned long long>(std::min<unsigned long long>(bc[0], 2048), (2ull << 30) / per));
      const size_t need = (size_t)waves * per;
      if (need > bws_bytes) {
        (void)hipFree(bws);
        bws = nullptr;
        bws_bytes = 0;
        if ((e = hipMalloc(&bws, need)) != hipSuccess) break;
        bws_bytes = need;
      }
      const uint32_t* idmap = std::is_same<S, LinAbd>::value ? P.cl_of : nullptr;   // LinAbd walks slots
      if (nw <= 64u)
        lin_big_kernel<1><<<waves, 64, 0, h->stream>>>(stage, big, (uint32_t)bc[0], bws, nw, out, mark, mark_bit, c0,
                                                       (uint32_t)cap, idmap);
      else
        lin_big_kernel<LIN_WPL_MAX><<<waves, 64, 0, h->stream>>>(stage, big, (uint32_t)bc[0], bws, nw, out, mark,
                                                                 mark_bit, c0, (uint32_t)cap, idmap);
      if ((e = hipGetLastError()) != hipSuccess) break;
    }
  }
  uint64_t res[LIN_NOUT + 8] = {0};
  if (e == hipSuccess) e = hipMemcpyAsync(res, out, sizeof res, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  cleanup();
  if (e != hipSuccess) return fail(PAXISIM_EDEVICE, "linearizable: %s", hipGetErrorString(e));
#ifdef PXS_LIN_STAMPS
  fprintf(stderr, "lin stamps (wave-cycles): p1 %llu p2 %llu sort %llu run %llu | add %llu look %llu merge %llu reach %llu\n",
          (unsigned long long)res[LIN_NOUT + 0], (unsigned long long)res[LIN_NOUT + 1], (unsigned long long)res[LIN_NOUT + 2],
          (unsigned long long)res[LIN_NOUT + 3], (unsigned long long)res[LIN_NOUT + 4], (unsigned long long)res[LIN_NOUT + 5],
          (unsigned long long)res[LIN_NOUT + 6], (unsigned long long)res[LIN_NOUT + 7]);
#endif
  h->lin_big = tot[LIN_BIG];
  h->lin_nmax = tot[LIN_NMAX];
  if (anomalies) *anomalies = res[LIN_ANOM];
  if (ops) *ops = res[LIN_OPS];
  if (skipped) *skipped = res[LIN_SKIP];   // partitions above LIN_VMAX ops (not checked)
  return 0;
}

extern "C" int paxisim_linearizable(paxisim* h, uint64_t* anomalies, uint64_t* ops, uint64_t* skipped) {
  if (!h) return fail(PAXISIM_EINVAL, "null handle");
  if (h->P.protocol != PAXISIM_ABD || h->P.H == 0)
    return fail(PAXISIM_EUNSUPP, "linearizability scan needs protocol ABD with history > 0");
  return lin_scan<LinAbd>(h, anomalies, ops, skipped);
}

// ---------------------------------------------------------------------------
// Client-side op history of every protocol (include/paxisim.h, DESIGN.md §3.13, chist_kernel.h)
// ---------------------------------------------------------------------------
extern "C" int paxisim_client_history_enable(paxisim* h, uint32_t ops_per_worker) {
  if (!h) return fail(PAXISIM_EINVAL, "null handle");
  if (ops_per_worker == 0 || ops_per_worker > PAXISIM_CLIENT_HISTORY_MAX)
    return fail(PAXISIM_EINVAL, "ops_per_worker must be in [1, %u]", PAXISIM_CLIENT_HISTORY_MAX);
  if (h->P.ch_cap) return fail(PAXISIM_EINVAL, "the client history is already enabled");
  if (h->t) return fail(PAXISIM_EINVAL, "the client history can only be enabled before the first step");
  if (!h->P.lat_bins)
    return fail(PAXISIM_EINVAL, "the client history needs the recording step kernels and their issue stamps: "
                                "call paxisim_latency_enable first");
  if (h->P.protocol != PAXISIM_ABD && !h->P.kv)
    return fail(PAXISIM_EUNSUPP, "replies carry no read values (config.kv = 0)");
  if (const int jrc = enter(h)) return jrc;
  Params P = h->P;
  P.ch_cap = ops_per_worker;
  const size_t cb = sizeof(uint32_t) * P.WK * P.C, ob = sizeof(uint4) * P.WK * P.C * (size_t)ops_per_worker;
  hipError_t e;
  if ((e = hipMalloc(&P.ch_cnt, cb)) != hipSuccess || (e = hipMalloc(&P.ch_ops, ob)) != hipSuccess ||
      (e = hipMemsetAsync(P.ch_cnt, 0, cb, h->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(h->stream)) != hipSuccess) {
    if (P.ch_cnt) (void)hipFree(P.ch_cnt);
    if (P.ch_ops) (void)hipFree(P.ch_ops);
    return fail(PAXISIM_ENOMEM, "client history buffers (%zu bytes): %s", cb + ob, hipGetErrorString(e));
  }
  h->P = P;
  h->ch_bytes = cb + ob;
  return 0;
}

// The ops of one cluster, 5 words per op {key, is_write, value, start, end}, workers in index
// order, each in completion order; *dropped_out: the ops past ops_per_worker, counted only.
extern "C" int paxisim_client_history(paxisim* h, uint64_t cluster, uint32_t* buf, uint32_t cap_ops, uint32_t* n_out,
                                      uint32_t* dropped_out) {
  if (!h || !n_out) return fail(PAXISIM_EINVAL, "null argument");
  if (!h->P.ch_cap) return fail(PAXISIM_EINVAL, "the client history is not enabled");
  if (cluster >= h->cfg.clusters) return fail(PAXISIM_ERANGE, "cluster");
  if (const int jrc = enter(h)) return jrc;
  if (const int rc = pipe_check(h)) return rc;   // results only of launches that fully ran
  const Params& P = h->P;
  const uint32_t tot = P.WK * P.ch_cap;
  uint4* d_ops = nullptr;
  uint32_t* d_cnt = nullptr;
  std::vector<uint4> tmp(tot);
  std::vector<uint32_t> cnt(P.WK);
  hipError_t e = hipMalloc(&d_ops, tot * sizeof(uint4));
  if (e == hipSuccess) e = hipMalloc(&d_cnt, P.WK * sizeof(uint32_t));
  if (e == hipSuccess) {
    chist_read_kernel<<<(tot + 255u) / 256u, 256, 0, h->stream>>>(P, cluster, d_ops, d_cnt);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(tmp.data(), d_ops, tot * sizeof(uint4), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(cnt.data(), d_cnt, P.WK * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  (void)hipFree(d_ops);
  (void)hipFree(d_cnt);
  if (e != hipSuccess) return fail(PAXISIM_EDEVICE, "client history: %s", hipGetErrorString(e));
  uint32_t n = 0, dropped = 0;
  for (uint32_t w = 0; w < P.WK; w++) {
    const uint32_t len = std::min(cnt[w], P.ch_cap);
    dropped += cnt[w] - len;
    for (uint32_t j = 0; j < len; j++, n++) {
      if (!buf || n >= cap_ops) continue;
      const uint4& r = tmp[(size_t)w * P.ch_cap + j];
      uint32_t* o = buf + 5 * (size_t)n;
      o[0] = r.x & 0x7FFFFFFFu;
      o[1] = r.x >> 31;
      o[2] = r.y;
      o[3] = r.z;
      o[4] = r.w;
    }
  }
  *n_out = n;
  if (dropped_out) *dropped_out = dropped;
  return 0;
}

// History.ReadFile (history.go:115-178) into the device history of one worker: literal records.
extern "C" int paxisim_client_history_load(paxisim* h, uint64_t cluster, uint32_t worker, const uint32_t* ops,
                                           uint32_t n) {
  if (!h || (n && !ops)) return fail(PAXISIM_EINVAL, "null argument");
  if (!h->P.ch_cap) return fail(PAXISIM_EINVAL, "the client history is not enabled");
  if (cluster >= h->cfg.clusters || worker >= h->P.WK) return fail(PAXISIM_ERANGE, "bad worker");
  if (n > h->P.ch_cap) return fail(PAXISIM_EINVAL, "%u ops exceed history capacity %u", n, h->P.ch_cap);
  if (const int jrc = enter(h)) return jrc;
  if (const int rc = pipe_check(h)) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  const Params& P = h->P;
  std::vector<uint4> tmp(n ? n : 1);
  for (uint32_t j = 0; j < n; j++) {
    const uint32_t* o = ops + 5 * (size_t)j;
    if (o[0] >= P.keys || o[1] > 1u) return fail(PAXISIM_EINVAL, "op %u: bad key (keys = %u) or is_write", j, P.keys);
    tmp[j] = make_uint4(CH_LITERAL | (o[1] ? CH_WRITE : 0u) | o[0], o[2], o[3], o[4]);
  }
  const size_t row = chist_row(P, worker, cluster);
  if (n) HIPCHK(hipMemcpy(&P.ch_ops[row * P.ch_cap], tmp.data(), n * sizeof(uint4), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(&P.ch_cnt[row], &n, 4, hipMemcpyHostToDevice));
  return 0;
}

extern "C" int paxisim_client_linearizable(paxisim* h, uint64_t* anomalies, uint64_t* ops, uint64_t* skipped) {
  if (!h) return fail(PAXISIM_EINVAL, "null handle");
  if (!h->P.ch_cap) return fail(PAXISIM_EINVAL, "the client history is not enabled");
  return lin_scan<LinClient>(h, anomalies, ops, skipped);
}

// ---------------------------------------------------------------------------
// Multi-version Database and Consensus (include/paxisim.h, DESIGN.md §3.14, mv_kernel.h)
// ---------------------------------------------------------------------------
extern "C" int paxisim_multiversion_enable(paxisim* h, uint32_t versions_per_key) {
  if (!h) return fail(PAXISIM_EINVAL, "null handle");
  if (versions_per_key == 0 || versions_per_key > PAXISIM_MV_MAX)
    return fail(PAXISIM_EINVAL, "versions_per_key must be in [1, %u]", PAXISIM_MV_MAX);
  if (h->P.mv_cap) return fail(PAXISIM_EINVAL, "multiversion is already enabled");
  if (h->t) return fail(PAXISIM_EINVAL, "multiversion can only be enabled before the first step");
  if (!h->P.lat_bins)
    return fail(PAXISIM_EINVAL, "multiversion needs the recording step kernels: call paxisim_latency_enable first");
  if (h->P.protocol == PAXISIM_ABD)
    return fail(PAXISIM_EUNSUPP, "ABD's KV is written by versioned Sets, not by Execute of a log: no put order to record");
  if (!h->P.kv) return fail(PAXISIM_EUNSUPP, "replicas keep no Database (config.kv = 0)");
  if (const int jrc = enter(h)) return jrc;
  Params P = h->P;
  P.mv_cap = versions_per_key;
  const size_t rows = (size_t)P.keys * P.N * P.C;
  const size_t cb = sizeof(uint32_t) * rows, vb = cb * versions_per_key;
  hipError_t e;
  if ((e = hipMalloc(&P.mv_cnt, cb)) != hipSuccess || (e = hipMalloc(&P.mv_val, vb)) != hipSuccess ||
      (e = hipMemsetAsync(P.mv_cnt, 0, cb, h->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(h->stream)) != hipSuccess) {
    if (P.mv_cnt) (void)hipFree(P.mv_cnt);
    if (P.mv_val) (void)hipFree(P.mv_val);
    return fail(PAXISIM_ENOMEM, "multiversion buffers (%zu bytes): %s", cb + vb, hipGetErrorString(e));
  }
  h->P = P;
  h->mv_bytes = cb + vb;
  return 0;
}

// Database.History(key) of one replica: the row is contiguous and indexed by the cluster id, so
// the readout is a copy of the count and one of the kept values.
extern "C" int paxisim_kv_history(paxisim* h, uint64_t cluster, uint32_t replica, uint32_t key, uint32_t* values,
                                  uint32_t cap, uint32_t* n_out, uint32_t* dropped_out) {
  if (!h || !n_out) return fail(PAXISIM_EINVAL, "null argument");
  if (!h->P.mv_cap) return fail(PAXISIM_EINVAL, "multiversion is not enabled");
  if (cluster >= h->cfg.clusters) return fail(PAXISIM_ERANGE, "cluster");
  if (replica >= h->P.N || key >= h->P.keys) return fail(PAXISIM_EINVAL, "no replica %u or key %u", replica, key);
  if (const int jrc = enter(h)) return jrc;
  if (const int rc = pipe_check(h)) return rc;   // results only of launches that fully ran
  const Params& P = h->P;
  const size_t row = mv_row(P, key, replica, cluster);
  uint32_t n = 0;
  HIPCHK(hipMemcpyAsync(&n, &P.mv_cnt[row], sizeof n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  const uint32_t kept = std::min(n, P.mv_cap), take = values ? std::min(kept, cap) : 0u;
  if (take) {
    HIPCHK(hipMemcpyAsync(values, &P.mv_val[row * P.mv_cap], take * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  *n_out = kept;
  if (dropped_out) *dropped_out = n - kept;
  return 0;
}

// client.go:279-320 over clusters [lo, lo + n): totals into tot[MV_NOUT], the failing keys of each
// cluster into masks (either may be null).
static int mv_scan(paxisim* h, uint64_t lo, uint64_t n, uint64_t* tot, uint64_t* masks) {
  if (const int jrc = enter(h)) return jrc;
  if (const int rc = pipe_check(h)) return rc;   // results only of launches that fully ran
  const Params& P = h->P;
  unsigned long long* d_masks = nullptr;
  if (masks) {
    HIPCHK(hipMalloc(&d_masks, n * sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d_masks, 0, n * sizeof(unsigned long long), h->stream);
    if (e != hipSuccess) {
      (void)hipFree(d_masks);
      return fail(PAXISIM_EDEVICE, "consensus: %s", hipGetErrorString(e));
    }
  }
  unsigned long long* out = reinterpret_cast<unsigned long long*>(h->d_scratch);
  uint64_t res[MV_NOUT] = {0, 0, 0};
  // a wave per (cluster, key), dealt grid-stride: enough workgroups to fill the device, no more
  const uint64_t pairs = n * P.keys;
  const unsigned grid = (unsigned)std::min<uint64_t>((pairs + MV_WAVES - 1) / MV_WAVES, 8192);
  hipError_t e = hipMemsetAsync(out, 0, sizeof res, h->stream);
  if (e == hipSuccess) {
    mv_consensus_kernel<<<grid, MV_WAVES * 64, 0, h->stream>>>(P, lo, n, out, d_masks);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(res, out, sizeof res, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess && masks)
    e = hipMemcpyAsync(masks, d_masks, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (d_masks) (void)hipFree(d_masks);
  if (e != hipSuccess) return fail(PAXISIM_EDEVICE, "consensus: %s", hipGetErrorString(e));
  if (tot)
    for (int i = 0; i < MV_NOUT; i++) tot[i] = res[i];
  return 0;
}

extern "C" int paxisim_consensus(paxisim* h, uint64_t* failed, uint64_t* versions, uint64_t* dropped) {
  if (!h) return fail(PAXISIM_EINVAL, "null handle");
  if (!h->P.mv_cap) return fail(PAXISIM_EINVAL, "multiversion is not enabled");
  uint64_t tot[MV_NOUT];
  if (const int rc = mv_scan(h, 0, h->cfg.clusters, tot, nullptr)) return rc;
  if (failed) *failed = tot[MV_FAILED];
  if (versions) *versions = tot[MV_VERSIONS];
  if (dropped) *dropped = tot[MV_DROPPED];
  return 0;
}

extern "C" int paxisim_consensus_failed(paxisim* h, uint64_t cluster_lo, uint64_t n, uint64_t* key_masks) {
  if (!h || (n && !key_masks)) return fail(PAXISIM_EINVAL, "null argument");
  if (!h->P.mv_cap) return fail(PAXISIM_EINVAL, "multiversion is not enabled");
  if (cluster_lo > h->cfg.clusters || n > h->cfg.clusters - cluster_lo) return fail(PAXISIM_ERANGE, "cluster range");
  if (n == 0) return 0;
  return mv_scan(h, cluster_lo, n, nullptr, key_masks);
}

// ---------------------------------------------------------------------------
// Message traces of chosen clusters (include/paxisim.h, DESIGN.md §3.15, trace_kernel.h)
// ---------------------------------------------------------------------------
extern "C" int paxisim_trace_enable(paxisim* h, const uint64_t* clusters, uint32_t n_clusters,
                                    uint32_t records_per_replica, uint32_t step_from, uint32_t step_to) {
  if (!h) return fail(PAXISIM_EINVAL, "null handle");
  if (h->P.tr_cap) return fail(PAXISIM_EINVAL, "tracing is already enabled");
  if (h->t) return fail(PAXISIM_EINVAL, "tracing can only be enabled before the first step");
  if (!h->P.lat_bins)
    return fail(PAXISIM_EINVAL, "tracing needs the recording step kernels: call paxisim_latency_enable first");
  if (n_clusters == 0 || n_clusters > PAXISIM_TRACE_MAX_CLUSTERS || !clusters)
    return fail(PAXISIM_EINVAL, "n_clusters must be in [1, %u]", PAXISIM_TRACE_MAX_CLUSTERS);
  if (records_per_replica == 0 || records_per_replica > PAXISIM_TRACE_MAX_RECORDS)
    return fail(PAXISIM_EINVAL, "records_per_replica must be in [1, %u]", PAXISIM_TRACE_MAX_RECORDS);
  if (step_from >= step_to) return fail(PAXISIM_EINVAL, "empty step window [%u, %u)", step_from, step_to);
  std::vector<uint32_t> row(h->P.C, TR_NONE);
  for (uint32_t i = 0; i < n_clusters; i++) {
    if (clusters[i] >= h->cfg.clusters)
      return fail(PAXISIM_ERANGE, "traced cluster %llu outside the handle", (unsigned long long)clusters[i]);
    if (row[clusters[i]] != TR_NONE)
      return fail(PAXISIM_EINVAL, "cluster %llu is listed twice", (unsigned long long)clusters[i]);
    row[clusters[i]] = i;
  }
  if (const int jrc = enter(h)) return jrc;
  Params P = h->P;
  P.tr_cap = records_per_replica;
  P.tr_from = step_from;
  P.tr_to = step_to;
  const size_t rows = (size_t)n_clusters * P.N;
  const size_t tb = sizeof(uint32_t) * row.size(), cb = sizeof(uint32_t) * rows;
  const size_t rb = 2 * sizeof(uint4) * rows * records_per_replica;
  uint32_t* d_row = nullptr;
  hipError_t e;
  if ((e = hipMalloc(&d_row, tb)) != hipSuccess || (e = hipMalloc(&P.tr_cnt, cb)) != hipSuccess ||
      (e = hipMalloc(&P.tr_rec, rb)) != hipSuccess ||
      (e = hipMemcpyAsync(d_row, row.data(), tb, hipMemcpyHostToDevice, h->stream)) != hipSuccess ||
      (e = hipMemsetAsync(P.tr_cnt, 0, cb, h->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(h->stream)) != hipSuccess) {
    if (d_row) (void)hipFree(d_row);
    if (P.tr_cnt) (void)hipFree(P.tr_cnt);
    if (P.tr_rec) (void)hipFree(P.tr_rec);
    return fail(PAXISIM_ENOMEM, "trace buffers (%zu bytes): %s", tb + cb + rb, hipGetErrorString(e));
  }
  P.tr_row = d_row;
  h->P = P;
  h->tr_bytes = tb + cb + rb;
  h->tr_rows = n_clusters;
  h->tr_row.swap(row);
  return 0;
}

// The row is contiguous and found by the cluster id, so the readout is a copy of the count and one
// of the kept slots.
extern "C" int paxisim_trace_read(paxisim* h, uint64_t cluster, uint32_t replica, paxisim_trace_record* out,
                                  uint32_t cap, uint32_t* n_out, uint32_t* dropped_out) {
  if (!h || !n_out) return fail(PAXISIM_EINVAL, "null argument");
  if (!h->P.tr_cap) return fail(PAXISIM_EINVAL, "tracing is not enabled");
  if (cluster >= h->cfg.clusters || h->tr_row[cluster] == TR_NONE)
    return fail(PAXISIM_EINVAL, "cluster %llu is not traced", (unsigned long long)cluster);
  if (replica >= h->P.N) return fail(PAXISIM_EINVAL, "no replica %u", replica);
  if (const int jrc = enter(h)) return jrc;
  if (const int rc = pipe_check(h)) return rc;   // results only of launches that fully ran
  const Params& P = h->P;
  const size_t ri = trace_row(P, h->tr_row[cluster], replica);
  uint32_t n = 0;
  HIPCHK(hipMemcpyAsync(&n, &P.tr_cnt[ri], sizeof n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  const uint32_t kept = std::min(n, P.tr_cap), take = out ? std::min(kept, cap) : 0u;
  if (take) {
    std::vector<uint4> tmp(2 * (size_t)take);
    HIPCHK(hipMemcpyAsync(tmp.data(), &P.tr_rec[ri * P.tr_cap * 2], tmp.size() * sizeof(uint4), hipMemcpyDeviceToHost,
                          h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (uint32_t k = 0; k < take; k++) {
      const uint4 &a = tmp[2 * (size_t)k], &m = tmp[2 * (size_t)k + 1];
      out[k] = paxisim_trace_record{a.x, a.y, m.x, m.y, m.z, m.w};
    }
  }
  *n_out = kept;
  if (dropped_out) *dropped_out = n - kept;
  return 0;
}

extern "C" int paxisim_trace_totals(paxisim* h, uint64_t* records, uint64_t* dropped) {
  if (!h) return fail(PAXISIM_EINVAL, "null handle");
  if (!h->P.tr_cap) return fail(PAXISIM_EINVAL, "tracing is not enabled");
  if (const int jrc = enter(h)) return jrc;
  if (const int rc = pipe_check(h)) return rc;   // results only of launches that fully ran
  const Params& P = h->P;
  std::vector<uint32_t> cnt((size_t)h->tr_rows * P.N);
  HIPCHK(hipMemcpyAsync(cnt.data(), P.tr_cnt, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  uint64_t kept = 0, lost = 0;
  for (const uint32_t n : cnt) {
    kept += std::min(n, P.tr_cap);
    lost += n - std::min(n, P.tr_cap);
  }
  if (records) *records = kept;
  if (dropped) *dropped = lost;
  return 0;
}

// ---------------------------------------------------------------------------
// Snapshot, restore and fork (include/paxisim_snapshot.h, DESIGN.md §3.16, snapshot_plan.h,
// snapshot_kernel.h).  The arena but rec goes as plain copies; rec goes as its live records.
// ---------------------------------------------------------------------------
static_assert(SNAP_LAT_SLICES == LAT_SLICES && SNAP_LAT_EXTRA == LAT_EXTRA, "snapshot_plan.h: the latency accumulators");
static_assert(SNAP_CMP_WORDS == CM_SUMS, "snapshot_plan.h: a pool's compaction words");
static_assert(sizeof(DevFault) == 48, "include/paxisim_snapshot.h: the FAULTS section");
extern "C" const char* paxisim_build_id(void);

// What every readout does first: join the pools, check the pipelined launches, sync the stream.
static int quiesce(paxisim* h) {
  if (const int jrc = enter(h)) return jrc;
  for (uint32_t p = 0; p < h->npools; p++) HIPCHK(hipStreamSynchronize(h->pool[p].stream));
  if (const int rc = pipe_check(h)) return rc;   // a sticky pipeline error refuses
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// the moving-Mu tables back from the device: the handle keeps no host copy (create_on_device)
static int move_tables_host(paxisim* h, std::vector<uint32_t>& out) {
  out.clear();
  if (!h->d_move) return 0;
  out.resize((size_t)h->P.move_tables * PAXISIM_MAX_KEYS);
  HIPCHK(hipMemcpyAsync(out.data(), h->d_move, out.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

static int handle_plan(paxisim* h, PlanWords* pw) {
  std::vector<uint32_t> mv;
  if (const int rc = move_tables_host(h, mv)) return rc;
  Params Q = h->P;
  const ArenaSize sz = carve_arena(Q, h->cfg.policy, nullptr, false);
  PlanExtra x;
  x.arena_zero = sz.zero_bytes;
  x.arena_total = sz.total;
  x.serial = h->ops.serial;
  x.staged = h->ops.staged;
  x.chunk = h->S;
  x.pipe_max = h->pipe_max;
  x.cmp_every = h->cmp_every;
  x.late_until = h->late_until;
  x.pipe_slots = h->pipe_slots;
  x.npools = h->npools;
  x.pool1_base = h->npools > 1 ? h->pool[1].base : 0u;
  x.move_cdf = mv.empty() ? nullptr : mv.data();
  paxisim_config cfg = h->cfg;
  cfg.protocol = h->P.variant;   // the protocol the caller asked for
  *pw = plan_words(cfg, h->wl, h->fp, h->P, x);
  return 0;
}

static unsigned snap_grid(uint64_t blocks) { return (unsigned)((blocks + SNAP_WAVES - 1) / SNAP_WAVES); }

// The count pass: per-block live records, scanned to each block's offset in the packed stream;
// *d_offs: [blocks + 1] on the device (the caller frees it), the grand total in its last word and *total.
static int mbox_count_pass(paxisim* h, unsigned long long** d_offs, uint64_t* total) {
  const Params& P = h->P;
  const uint64_t blocks = P.C / LANES;
  unsigned long long* d = nullptr;
  hipError_t e = hipMalloc(&d, (blocks + 1) * sizeof(unsigned long long));
  if (e != hipSuccess) return fail(PAXISIM_ENOMEM, "snapshot count buffer (%llu bytes): %s",
                                   (unsigned long long)((blocks + 1) * 8), hipGetErrorString(e));
  unsigned long long tot = 0;
  mbox_count<<<snap_grid(blocks), SNAP_WAVES * LANES, 0, h->stream>>>(P.image, P.img, P.D * P.N * P.NS, P.M, blocks, d);
  mbox_scan<<<1, 1024, 0, h->stream>>>(d, blocks, d + blocks);
  if ((e = hipGetLastError()) == hipSuccess)
    e = hipMemcpyAsync(&tot, d + blocks, sizeof tot, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return fail(PAXISIM_EDEVICE, "snapshot count pass: %s", hipGetErrorString(e));
  }
  *d_offs = d;
  *total = tot;
  return 0;
}

static int snap_header_of(paxisim* h, uint64_t records, PlanWords* pw, SnapHeader* H) {
  if (const int rc = handle_plan(h, pw)) return rc;
  *H = snap_header(paxisim_build_id(), *pw, h->P.variant, h->P, h->cfg.policy, h->t, (uint32_t)h->faults.size(), h->npools,
                   snap_recorders(h->P, h->tr_rows), records);
  return 0;
}

extern "C" int paxisim_snapshot_size(paxisim* h, uint64_t* bytes) {
  if (!h || !bytes) return fail(PAXISIM_EINVAL, "null argument");
  if (const int rc = quiesce(h)) return rc;
  unsigned long long* d_offs = nullptr;
  uint64_t records = 0;
  if (const int rc = mbox_count_pass(h, &d_offs, &records)) return rc;
  (void)hipFree(d_offs);
  PlanWords pw;
  SnapHeader H;
  if (const int rc = snap_header_of(h, records, &pw, &H)) return rc;
  *bytes = H.total_bytes;
  return 0;
}

extern "C" int paxisim_snapshot(paxisim* h, void* buf, uint64_t cap, uint64_t* written) {
  if (!h || !buf) return fail(PAXISIM_EINVAL, "null argument");
  if (const int rc = quiesce(h)) return rc;
  const Params& P = h->P;
  unsigned long long* d_offs = nullptr;
  uint4* d_pack = nullptr;
  uint64_t records = 0;
  if (const int rc = mbox_count_pass(h, &d_offs, &records)) return rc;
  PlanWords pw;
  SnapHeader H;
  int rc = snap_header_of(h, records, &pw, &H);
  if (!rc && cap < H.total_bytes)
    rc = fail(PAXISIM_ERANGE, "snapshot needs %llu bytes, the buffer holds %llu", (unsigned long long)H.total_bytes,
              (unsigned long long)cap);
  if (!rc && records) {   // the packed stage, sized from the count pass
    const hipError_t e = hipMalloc(&d_pack, records * sizeof(uint4));
    if (e != hipSuccess)
      rc = fail(PAXISIM_ENOMEM, "snapshot packed stage (%llu bytes): %s", (unsigned long long)(records * sizeof(uint4)),
                hipGetErrorString(e));
  }
  if (rc) {
    (void)hipFree(d_offs);
    return rc;
  }
  uint8_t* out = static_cast<uint8_t*>(buf);
  auto at = [&](uint32_t s) { return out + snap_offset(H, s); };
  memcpy(out, &H, sizeof H);
  memcpy(at(PAXISIM_SNAP_PLAN), pw.w.data(), pw.w.size() * 8);
  if (!h->faults.empty()) memcpy(at(PAXISIM_SNAP_FAULTS), h->faults.data(), h->faults.size() * sizeof(DevFault));
  hipError_t e = hipSuccess;
  auto d2h = [&](uint8_t*& dst, const void* src, size_t n) {
    if (e == hipSuccess && n) e = hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, h->stream);
    dst += n;
  };
  for (uint32_t p = 0; p < h->npools; p++) {
    uint8_t* w = at(PAXISIM_SNAP_POOLS) + (size_t)p * SNAP_POOL_BYTES;
    memset(w, 0, SNAP_POOL_BYTES);
    memcpy(w + 4 * SNAP_CMP_WORDS, &h->pool[p].last_cmp, 4);
    d2h(w, h->pool[p].d_cmp, 4 * SNAP_CMP_WORDS);
  }
  uint8_t* w = at(PAXISIM_SNAP_ARENA);
  d2h(w, h->arena, H.section_bytes[PAXISIM_SNAP_ARENA]);
  if (records && e == hipSuccess) {
    const uint64_t blocks = P.C / LANES;
    mbox_pack<<<snap_grid(blocks), SNAP_WAVES * LANES, 0, h->stream>>>(P.image, P.img, P.rec, P.rec_per_block,
                                                                      P.D * P.N * P.NS, P.M, blocks, d_offs, records, d_pack);
    e = hipGetLastError();
    w = at(PAXISIM_SNAP_MAILBOX);
    d2h(w, d_pack, records * sizeof(uint4));
  }
  if (P.lat_bins) {
    w = at(PAXISIM_SNAP_LAT);
    d2h(w, P.lat_stamp, snap_lat_stamp_bytes(P));
    d2h(w, P.lat_acc, snap_lat_acc_bytes(P, P.lat_bins));
  }
  if (P.ch_cap) {
    w = at(PAXISIM_SNAP_CHIST);
    d2h(w, P.ch_cnt, snap_ch_cnt_bytes(P));
    d2h(w, P.ch_ops, snap_ch_ops_bytes(P, P.ch_cap));
  }
  if (P.mv_cap) {
    w = at(PAXISIM_SNAP_MV);
    d2h(w, P.mv_cnt, snap_mv_cnt_bytes(P));
    d2h(w, P.mv_val, snap_mv_val_bytes(P, P.mv_cap));
  }
  if (P.tr_cap) {
    w = at(PAXISIM_SNAP_TRACE);
    memcpy(w, h->tr_row.data(), snap_tr_row_bytes(P));
    w += snap_tr_row_bytes(P);
    d2h(w, P.tr_cnt, snap_tr_cnt_bytes(P, h->tr_rows));
    d2h(w, P.tr_rec, snap_tr_rec_bytes(P, h->tr_rows, P.tr_cap));
  }
  const hipError_t es = hipStreamSynchronize(h->stream);
  if (e == hipSuccess) e = es;
  (void)hipFree(d_offs);
  (void)hipFree(d_pack);
  if (e != hipSuccess) return fail(PAXISIM_EDEVICE, "snapshot: %s", hipGetErrorString(e));
  if (written) *written = H.total_bytes;
  return 0;
}

extern "C" int paxisim_snapshot_info(const void* buf, uint64_t bytes, struct paxisim_snapshot_info* out) {
  return snap_info(buf, bytes, out);
}

extern "C" int paxisim_restore(paxisim* h, const void* buf, uint64_t bytes) {
  if (!h || !buf) return fail(PAXISIM_EINVAL, "null argument");
  if (const int rc = quiesce(h)) return rc;
  Params& P = h->P;
  PlanWords pw;
  if (const int rc = handle_plan(h, &pw)) return rc;
  SnapHeader H;
  bool trace_carried = false;
  const SnapRecorders r = snap_recorders(P, h->tr_rows);
  if (const int rc = snap_check_restore(buf, bytes, paxisim_build_id(), pw, P, h->cfg.policy, h->npools, r, &H, &trace_carried))
    return rc;
  const uint8_t* in = static_cast<const uint8_t*>(buf);
  auto at = [&](uint32_t s) { return in + snap_offset(H, s); };
  if (trace_carried && memcmp(at(PAXISIM_SNAP_TRACE), h->tr_row.data(), snap_tr_row_bytes(P)))
    return fail(PAXISIM_EINVAL, "snapshot recorders differ: the traced clusters");
  // the pools' bounds lie inside their regions
  uint32_t cmp[MAX_POOLS][SNAP_CMP_WORDS], last_cmp[MAX_POOLS] = {0, 0};
  for (uint32_t p = 0; p < h->npools; p++) {
    const uint8_t* w = at(PAXISIM_SNAP_POOLS) + (size_t)p * SNAP_POOL_BYTES;
    memcpy(cmp[p], w, sizeof cmp[p]);
    memcpy(&last_cmp[p], w + sizeof cmp[p], 4);
    if (cmp[p][CM_BOUND] < h->pool[p].base || cmp[p][CM_BOUND] > h->pool[p].end)
      return fail(PAXISIM_EINVAL, "snapshot pool %u: bound %u outside its region [%u, %u]", p, cmp[p][CM_BOUND],
                  h->pool[p].base, h->pool[p].end);
  }
  if (H.step >= T_MAX) return fail(PAXISIM_EINVAL, "snapshot step %u", H.step);
  // the mailbox counts of the blob's images: every block's offset in the packed stream, and their
  // total, which must be the records carried (the counts decide what is live)
  const uint64_t blocks = P.C / LANES;
  const uint32_t nbox = P.D * P.N * P.NS;
  std::vector<unsigned long long> offs(blocks + 1);
  {
    const uint8_t* img0 = at(PAXISIM_SNAP_ARENA) + (P.image - static_cast<const uint8_t*>(h->arena));
    unsigned long long tot = 0;
    for (uint64_t b = 0; b < blocks; b++) {
      offs[b] = tot;
      const uint8_t* c = img0 + b * (size_t)P.img.bytes + P.img.off_cnt;
      for (size_t i = 0; i < (size_t)nbox * LANES; i++) tot += c[i] < P.M ? c[i] : P.M;
    }
    offs[blocks] = tot;
    if (tot != H.mailbox_records)
      return fail(PAXISIM_EINVAL, "snapshot mailbox counts add up to %llu records, the snapshot carries %llu", tot,
                  (unsigned long long)H.mailbox_records);
  }
  // everything the device writes need, before the first of them
  unsigned long long* d_offs = nullptr;
  uint4* d_pack = nullptr;
  const uint64_t records = H.mailbox_records;
  hipError_t e = hipMalloc(&d_offs, offs.size() * sizeof(unsigned long long));
  if (e == hipSuccess && records) e = hipMalloc(&d_pack, records * sizeof(uint4));
  if (e != hipSuccess) {
    (void)hipFree(d_offs);
    return fail(PAXISIM_ENOMEM, "restore packed stage (%llu bytes): %s", (unsigned long long)(records * sizeof(uint4)),
                hipGetErrorString(e));
  }
  auto h2d = [&](void* dst, const uint8_t*& src, size_t n) {
    if (e == hipSuccess && n) e = hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, h->stream);
    src += n;
  };
  const uint8_t* w = at(PAXISIM_SNAP_ARENA);
  h2d(h->arena, w, H.section_bytes[PAXISIM_SNAP_ARENA]);
  if (records) {
    w = reinterpret_cast<const uint8_t*>(offs.data());
    h2d(d_offs, w, offs.size() * sizeof(unsigned long long));
    w = at(PAXISIM_SNAP_MAILBOX);
    h2d(d_pack, w, records * sizeof(uint4));
    if (e == hipSuccess) {
      mbox_unpack<<<snap_grid(blocks), SNAP_WAVES * LANES, 0, h->stream>>>(P.image, P.img, P.rec, P.rec_per_block, nbox, P.M,
                                                                          blocks, d_offs, records, d_pack);
      e = hipGetLastError();
    }
  }
  for (uint32_t p = 0; p < h->npools; p++) {
    w = reinterpret_cast<const uint8_t*>(cmp[p]);
    h2d(h->pool[p].d_cmp, w, sizeof cmp[p]);
  }
  std::vector<DevFault> faults(H.n_faults);
  if (H.n_faults) memcpy(static_cast<void*>(faults.data()), at(PAXISIM_SNAP_FAULTS), H.n_faults * sizeof(DevFault));
  w = reinterpret_cast<const uint8_t*>(faults.data());
  h2d(h->d_faults, w, faults.size() * sizeof(DevFault));
  if (P.lat_bins) {
    w = at(PAXISIM_SNAP_LAT);
    h2d(P.lat_stamp, w, snap_lat_stamp_bytes(P));
    h2d(P.lat_acc, w, snap_lat_acc_bytes(P, P.lat_bins));
  }
  if (P.ch_cap) {
    w = at(PAXISIM_SNAP_CHIST);
    h2d(P.ch_cnt, w, snap_ch_cnt_bytes(P));
    h2d(P.ch_ops, w, snap_ch_ops_bytes(P, P.ch_cap));
  }
  if (P.mv_cap) {
    w = at(PAXISIM_SNAP_MV);
    h2d(P.mv_cnt, w, snap_mv_cnt_bytes(P));
    h2d(P.mv_val, w, snap_mv_val_bytes(P, P.mv_cap));
  }
  if (P.tr_cap && trace_carried) {
    w = at(PAXISIM_SNAP_TRACE) + snap_tr_row_bytes(P);
    h2d(P.tr_cnt, w, snap_tr_cnt_bytes(P, h->tr_rows));
    h2d(P.tr_rec, w, snap_tr_rec_bytes(P, h->tr_rows, P.tr_cap));
  } else if (P.tr_cap && e == hipSuccess) {   // the handle's trace alone: empty rows, recording goes on from the restored step
    e = hipMemsetAsync(P.tr_cnt, 0, snap_tr_cnt_bytes(P, h->tr_rows), h->stream);
  }
  const hipError_t es = hipStreamSynchronize(h->stream);   // the copies read the caller's buffer and these vectors
  if (e == hipSuccess) e = es;
  (void)hipFree(d_offs);
  (void)hipFree(d_pack);
  if (e != hipSuccess) return fail(PAXISIM_EDEVICE, "restore: %s (the handle's state is undefined)", hipGetErrorString(e));
  h->faults.swap(faults);
  P.nfaults = H.n_faults;
  if (h->shape_fit) select_unit(h);   // the unit follows the restored fault count (either way)
  h->t = H.step;
  for (uint32_t p = 0; p < h->npools; p++) h->pool[p].last_cmp = last_cmp[p];
  return 0;
}

extern "C" int paxisim_fork(paxisim* h, paxisim** out) {
  if (!h || !out) return fail(PAXISIM_EINVAL, "null argument");
  if (const int rc = quiesce(h)) return rc;
  std::vector<uint32_t> mv;
  if (const int rc = move_tables_host(h, mv)) return rc;
  PlanWords pw;
  if (const int rc = handle_plan(h, &pw)) return rc;
  paxisim* f = new (std::nothrow) paxisim();
  if (!f) return fail(PAXISIM_ENOMEM, "oom");
  auto drop = [&](int rc) {
    paxisim_destroy(f);
    return rc;
  };
  f->cfg = h->cfg;
  f->wl = h->wl;
  f->wl.move_cdf = mv.empty() ? nullptr : mv.data();   // create uploads its own copy and keeps no pointer
  f->fp = h->fp;
  f->kn = h->kn;
  const Params& P = h->P;
  if (const int rc = create_on_device(f, h->kn, P.variant, P.N)) return drop(rc);
  if (P.lat_bins)
    if (const int rc = paxisim_latency_enable(f, P.lat_bins)) return drop(rc);
  if (P.ch_cap)
    if (const int rc = paxisim_client_history_enable(f, P.ch_cap)) return drop(rc);
  if (P.mv_cap)
    if (const int rc = paxisim_multiversion_enable(f, P.mv_cap)) return drop(rc);
  if (P.tr_cap) {
    std::vector<uint64_t> cl(h->tr_rows);
    for (uint64_t c = 0; c < h->cfg.clusters; c++)
      if (h->tr_row[c] != TR_NONE) cl[h->tr_row[c]] = c;
    if (const int rc = paxisim_trace_enable(f, cl.data(), h->tr_rows, P.tr_cap, P.tr_from, P.tr_to)) return drop(rc);
  }
  {   // the same plan, or the copies below would not fit
    PlanWords fw;
    if (const int rc = handle_plan(f, &fw)) return drop(rc);
    for (size_t i = 0; i < pw.w.size(); i++)
      if (fw.w[i] != pw.w[i])
        return drop(fail(PAXISIM_EDEVICE, "fork: the new handle's plan differs: %s (parent %llu, fork %llu)", pw.names[i],
                         (unsigned long long)pw.w[i], (unsigned long long)fw.w[i]));
  }
  const Params& Q = f->P;
  const ArenaSize sz = [&] { Params T = P; return carve_arena(T, h->cfg.policy, nullptr, false); }();
  hipError_t e = hipSuccess;
  auto d2d = [&](void* dst, const void* src, size_t n) {
    if (e == hipSuccess && n) e = hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, f->stream);
  };
  d2d(f->arena, h->arena, sz.zero_bytes);   // everything but rec
  if (e == hipSuccess) {                    // rec: the live records, by the counts just copied
    const uint64_t blocks = P.C / LANES;
    mbox_copy_live<<<snap_grid(blocks), SNAP_WAVES * LANES, 0, f->stream>>>(Q.image, Q.img, P.rec, Q.rec, Q.rec_per_block,
                                                                           Q.D * Q.N * Q.NS, Q.M, blocks);
    e = hipGetLastError();
  }
  for (uint32_t p = 0; p < h->npools; p++) d2d(f->pool[p].d_cmp, h->pool[p].d_cmp, sizeof(uint32_t) * SNAP_CMP_WORDS);
  d2d(f->d_faults, h->d_faults, h->faults.size() * sizeof(DevFault));
  if (P.lat_bins) {
    d2d(Q.lat_stamp, P.lat_stamp, snap_lat_stamp_bytes(P));
    d2d(Q.lat_acc, P.lat_acc, snap_lat_acc_bytes(P, P.lat_bins));
  }
  if (P.ch_cap) {
    d2d(Q.ch_cnt, P.ch_cnt, snap_ch_cnt_bytes(P));
    d2d(Q.ch_ops, P.ch_ops, snap_ch_ops_bytes(P, P.ch_cap));
  }
  if (P.mv_cap) {
    d2d(Q.mv_cnt, P.mv_cnt, snap_mv_cnt_bytes(P));
    d2d(Q.mv_val, P.mv_val, snap_mv_val_bytes(P, P.mv_cap));
  }
  if (P.tr_cap) {
    d2d(Q.tr_cnt, P.tr_cnt, snap_tr_cnt_bytes(P, h->tr_rows));
    d2d(Q.tr_rec, P.tr_rec, snap_tr_rec_bytes(P, h->tr_rows, P.tr_cap));
  }
  if (e == hipSuccess) e = hipStreamSynchronize(f->stream);
  if (e != hipSuccess) return drop(fail(PAXISIM_EDEVICE, "fork: %s", hipGetErrorString(e)));
  f->faults = h->faults;
  f->P.nfaults = P.nfaults;
  if (f->shape_fit) select_unit(f);
  f->t = h->t;
  for (uint32_t p = 0; p < h->npools; p++) f->pool[p].last_cmp = h->pool[p].last_cmp;
  if (f->npools > 1) f->main_ahead = true;   // the pools' streams wait for these copies
  *out = f;
  return 0;
}

// ---------------------------------------------------------------------------
// Per-cluster verdict words and the search over them (include/paxisim_verdict.h, DESIGN.md §3.17,
// verdict_kernel.h)
// ---------------------------------------------------------------------------
static_assert(LIN_MARK_SKIPPED == PAXISIM_V_LIN_SKIPPED, "lin_kernel.h: the skipped mark is the verdict bit");
static_assert(LIN_VMAX == 16384u, "include/paxisim_verdict.h: the partition size PAXISIM_V_LIN_SKIPPED speaks of");

namespace {
struct DevBuf {   // a device allocation freed at scope exit
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
  void* release() {
    void* q = p;
    p = nullptr;
    return q;
  }
};
}  // namespace

static uint32_t verdict_bits(const paxisim* h) {
  uint32_t b = PAXISIM_V_FLAGS | PAXISIM_V_QUIET | PAXISIM_V_WAITING | PAXISIM_V_STALLED;
  if (h->P.protocol != PAXISIM_EPAXOS) b |= PAXISIM_V_AGREE;
  if (h->P.mv_cap) b |= PAXISIM_V_CONSENSUS | PAXISIM_V_TRUNCATED;
  if (h->P.protocol == PAXISIM_ABD && h->P.H) b |= PAXISIM_V_LIN | PAXISIM_V_LIN_SKIPPED;
  if (h->P.ch_cap) b |= PAXISIM_V_CLIENT_LIN | PAXISIM_V_LIN_SKIPPED | PAXISIM_V_TRUNCATED;
  return b;
}

// The scans a call asks for: refused before anything is launched.
static int verdict_scans_ok(const paxisim* h, uint32_t scans) {
  if (scans & ~PAXISIM_V_SCANS)
    return fail(PAXISIM_EINVAL, "scans 0x%x: only CONSENSUS, LIN and CLIENT_LIN are scans", scans);
  if ((scans & PAXISIM_V_LIN) && (h->P.protocol != PAXISIM_ABD || h->P.H == 0))
    return fail(PAXISIM_EUNSUPP, "the LIN scan needs protocol ABD with history > 0");
  if ((scans & PAXISIM_V_CLIENT_LIN) && !h->P.ch_cap)
    return fail(PAXISIM_EUNSUPP, "the CLIENT_LIN scan needs paxisim_client_history_enable");
  if ((scans & PAXISIM_V_CONSENSUS) && !h->P.mv_cap)
    return fail(PAXISIM_EUNSUPP, "the CONSENSUS scan needs paxisim_multiversion_enable");
  return 0;
}

// The verdict word of every cluster, evaluated now: *d_words is [clusters] on the device, complete
// when this returns; the caller frees it.
static int verdict_eval(paxisim* h, uint32_t scans, uint32_t** d_words) {
  if (const int rc = quiesce(h)) return rc;
  const Params& P = h->P;
  const uint64_t n = P.clusters;
  DevBuf words, marks, masks;
  hipError_t e = hipMalloc(&words.p, n * sizeof(uint32_t));
  if (e == hipSuccess && (scans & (PAXISIM_V_LIN | PAXISIM_V_CLIENT_LIN))) {
    // (P.C entries: a slot-walking scan marks cl_of[slot], which is below C for every slot)
    e = hipMalloc(&marks.p, P.C * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemsetAsync(marks.p, 0, P.C * sizeof(uint32_t), h->stream);
  }
  if (e == hipSuccess && (scans & PAXISIM_V_CONSENSUS)) {
    e = hipMalloc(&masks.p, n * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemsetAsync(masks.p, 0, n * sizeof(unsigned long long), h->stream);
  }
  if (e != hipSuccess) return fail(PAXISIM_ENOMEM, "verdict buffers: %s", hipGetErrorString(e));
  if (scans & PAXISIM_V_LIN)
    if (const int rc = lin_scan<LinAbd>(h, nullptr, nullptr, nullptr, marks.as<uint32_t>(), PAXISIM_V_LIN)) return rc;
  if (scans & PAXISIM_V_CLIENT_LIN)
    if (const int rc = lin_scan<LinClient>(h, nullptr, nullptr, nullptr, marks.as<uint32_t>(), PAXISIM_V_CLIENT_LIN))
      return rc;
  if (scans & PAXISIM_V_CONSENSUS) {   // mv_scan's launch, its masks kept on the device
    unsigned long long* out = reinterpret_cast<unsigned long long*>(h->d_scratch);
    const uint64_t pairs = n * P.keys;
    const unsigned grid = (unsigned)std::min<uint64_t>((pairs + MV_WAVES - 1) / MV_WAVES, 8192);
    HIPCHK(hipMemsetAsync(out, 0, MV_NOUT * sizeof(unsigned long long), h->stream));
    mv_consensus_kernel<<<grid, MV_WAVES * 64, 0, h->stream>>>(P, 0, n, out, masks.as<unsigned long long>());
    HIPCHK(hipGetLastError());
  }
  VerdictScans in;
  in.mv_masks = masks.as<unsigned long long>();
  in.marks = marks.as<uint32_t>();
  in.scans = scans;
  in.started = h->t >= h->late_until ? 1u : 0u;
  verdict_kernel<<<(unsigned)((n + 255) / 256), 256, 0, h->stream>>>(P, in, words.as<uint32_t>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));   // the scans' buffers are freed on return
  *d_words = static_cast<uint32_t*>(words.release());
  return 0;
}

// The select over n device words on `stream` (verdict_kernel.h): the matching indices, ascending.
static int select_run(hipStream_t stream, const uint32_t* d_words, uint64_t n, uint32_t any, uint32_t none,
                      uint64_t* ids, uint64_t cap, uint64_t* total) {
  *total = 0;
  if (n == 0) return 0;
  const uint64_t nwg = (n + SEL_WG - 1) / SEL_WG;
  if (nwg > 0x7FFFFFFFull)
    return fail(PAXISIM_ERANGE, "select: %llu words are more than one launch covers", (unsigned long long)n);
  DevBuf offs, out;
  hipError_t e = hipMalloc(&offs.p, (nwg + 1) * sizeof(unsigned long long));
  if (e != hipSuccess) return fail(PAXISIM_ENOMEM, "select offsets: %s", hipGetErrorString(e));
  unsigned long long* d_offs = offs.as<unsigned long long>();
  unsigned long long tot = 0;
  select_count<<<(unsigned)nwg, SEL_WG, 0, stream>>>(d_words, n, any, none, d_offs);
  select_scan<<<1, SEL_SCAN, 0, stream>>>(d_offs, nwg, d_offs + nwg);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(&tot, d_offs + nwg, sizeof tot, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  *total = tot;
  const uint64_t k = std::min<uint64_t>(tot, cap);
  if (k == 0) return 0;
  e = hipMalloc(&out.p, k * sizeof(unsigned long long));
  if (e != hipSuccess) return fail(PAXISIM_ENOMEM, "select ids (%llu): %s", (unsigned long long)k, hipGetErrorString(e));
  select_scatter<<<(unsigned)nwg, SEL_WG, 0, stream>>>(d_words, n, any, none, d_offs, out.as<unsigned long long>(), k);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(ids, out.p, k * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  return 0;
}

extern "C" int paxisim_verdict_available(paxisim* h, uint32_t* bits) {
  if (!h || !bits) return fail(PAXISIM_EINVAL, "null argument");
  if (const int rc = quiesce(h)) return rc;
  *bits = verdict_bits(h);
  return 0;
}

extern "C" int paxisim_verdicts(paxisim* h, uint32_t scans, uint64_t lo, uint64_t n, uint32_t* words) {
  if (!h || (n && !words)) return fail(PAXISIM_EINVAL, "null argument");
  if (const int rc = verdict_scans_ok(h, scans)) return rc;
  if (lo > h->cfg.clusters || n > h->cfg.clusters - lo) return fail(PAXISIM_ERANGE, "cluster range");
  if (n == 0) return 0;
  DevBuf d;
  if (const int rc = verdict_eval(h, scans, reinterpret_cast<uint32_t**>(&d.p))) return rc;
  HIPCHK(hipMemcpyAsync(words, d.as<uint32_t>() + lo, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int paxisim_find(paxisim* h, uint32_t scans, uint32_t any, uint32_t none, uint64_t* ids, uint64_t cap,
                            uint64_t* total) {
  if (!h || !total || (cap && !ids)) return fail(PAXISIM_EINVAL, "null argument");
  if ((any | none) & ~PAXISIM_V_ALL)
    return fail(PAXISIM_EINVAL, "any 0x%x / none 0x%x: bits outside the defined ones", any, none);
  if (const int rc = verdict_scans_ok(h, scans)) return rc;
  DevBuf d;
  if (const int rc = verdict_eval(h, scans, reinterpret_cast<uint32_t**>(&d.p))) return rc;
  return select_run(h->stream, d.as<uint32_t>(), h->P.clusters, any, none, ids, cap, total);
}

extern "C" int paxisim_verdict_counts(paxisim* h, uint32_t scans, uint64_t counts[32]) {
  if (!h || !counts) return fail(PAXISIM_EINVAL, "null argument");
  if (const int rc = verdict_scans_ok(h, scans)) return rc;
  DevBuf d, c;
  if (const int rc = verdict_eval(h, scans, reinterpret_cast<uint32_t**>(&d.p))) return rc;
  const uint64_t n = h->P.clusters;
  hipError_t e = hipMalloc(&c.p, 32 * sizeof(unsigned long long));
  if (e != hipSuccess) return fail(PAXISIM_ENOMEM, "verdict counts: %s", hipGetErrorString(e));
  HIPCHK(hipMemsetAsync(c.p, 0, 32 * sizeof(unsigned long long), h->stream));
  verdict_count_kernel<<<(unsigned)((n + 255) / 256), 256, 0, h->stream>>>(d.as<uint32_t>(), n,
                                                                         c.as<unsigned long long>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(counts, c.p, 32 * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int paxisim_select_words(int device, const uint32_t* words, uint64_t n, uint32_t any, uint32_t none,
                                    uint64_t* ids, uint64_t cap, uint64_t* total) {
  if (!total || (n && !words) || (cap && !ids)) return fail(PAXISIM_EINVAL, "null argument");
  *total = 0;
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(device));
  DevBuf d;
  hipError_t e = hipMalloc(&d.p, n * sizeof(uint32_t));
  if (e != hipSuccess) return fail(PAXISIM_ENOMEM, "select words (%llu): %s", (unsigned long long)n, hipGetErrorString(e));
  HIPCHK(hipMemcpy(d.p, words, n * sizeof(uint32_t), hipMemcpyHostToDevice));
  return select_run(nullptr, d.as<uint32_t>(), n, any, none, ids, cap, total);
}

// ---------------------------------------------------------------------------
// Multi-GPU behind the C-ABI: clusters shard by range across
// handles (cluster_base), the data path has no collective, and the statistics
// are summed (max for time) with one RCCL all-reduce.  RCCL is opened at run
// time, so the library loads without it and only these calls need it; a
// process that already holds librccl.so.1 (e.g. through torch) shares it.
// ---------------------------------------------------------------------------
namespace {
struct Rccl {
  bool ok = false;
  ncclResult_t (*get_unique_id)(ncclUniqueId*);
  ncclResult_t (*init_rank)(ncclComm_t*, int, ncclUniqueId, int);
  ncclResult_t (*init_all)(ncclComm_t*, int, const int*);
  ncclResult_t (*all_reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t);
  ncclResult_t (*group_start)();
  ncclResult_t (*group_end)();
  ncclResult_t (*destroy)(ncclComm_t);
  const char* (*error_string)(ncclResult_t);
};
Rccl& rccl() {
  static Rccl r;
  static bool tried = false;
  if (tried) return r;
  tried = true;
  void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!h) return r;
  auto sym = [&](const char* n) { return dlsym(h, n); };
  r.get_unique_id = reinterpret_cast<decltype(r.get_unique_id)>(sym("ncclGetUniqueId"));
  r.init_rank = reinterpret_cast<decltype(r.init_rank)>(sym("ncclCommInitRank"));
  r.init_all = reinterpret_cast<decltype(r.init_all)>(sym("ncclCommInitAll"));
  r.all_reduce = reinterpret_cast<decltype(r.all_reduce)>(sym("ncclAllReduce"));
  r.group_start = reinterpret_cast<decltype(r.group_start)>(sym("ncclGroupStart"));
  r.group_end = reinterpret_cast<decltype(r.group_end)>(sym("ncclGroupEnd"));
  r.destroy = reinterpret_cast<decltype(r.destroy)>(sym("ncclCommDestroy"));
  r.error_string = reinterpret_cast<decltype(r.error_string)>(sym("ncclGetErrorString"));
  r.ok = r.get_unique_id && r.init_rank && r.init_all && r.all_reduce && r.group_start && r.group_end && r.destroy &&
         r.error_string;
  return r;
}
}  // namespace

#define RCCLCHK(expr)                                                                      \
  do {                                                                                     \
    ncclResult_t r_ = (expr);                                                              \
    if (r_ != ncclSuccess) return fail(PAXISIM_EDEVICE, "%s: %s", #expr, rccl().error_string(r_)); \
  } while (0)

struct paxisim_dist {
  std::vector<paxisim*> h;           // handles driven by this process, one per device
  std::vector<ncclComm_t> comm;
  std::vector<void*> buf;            // per member: device buffer for the reduction
};

constexpr uint32_t DIST_MAXV = 64;   // u64 sums + f64 maxes per reduction

extern "C" int paxisim_dist_unique_id(unsigned char id[128]) {
  if (!id) return fail(PAXISIM_EINVAL, "null argument");
  if (!rccl().ok) return fail(PAXISIM_EUNSUPP, "RCCL (librccl.so.1) not available");
  ncclUniqueId u;
  RCCLCHK(rccl().get_unique_id(&u));
  memcpy(id, u.internal, NCCL_UNIQUE_ID_BYTES);
  return 0;
}

static int dist_alloc(paxisim_dist* d) {
  for (paxisim* h : d->h) {
    void* b = nullptr;
    if (const int jrc = enter(h)) return jrc;
    HIPCHK(hipMalloc(&b, 2 * DIST_MAXV * sizeof(uint64_t)));
    d->buf.push_back(b);
  }
  return 0;
}

extern "C" int paxisim_dist_destroy(paxisim_dist* d) {
  if (!d) return 0;
  for (size_t i = 0; i < d->comm.size(); i++) (void)rccl().destroy(d->comm[i]);
  for (size_t i = 0; i < d->buf.size(); i++) {
    (void)hipSetDevice(d->h[i]->cfg.device);
    (void)hipFree(d->buf[i]);
  }
  delete d;
  return 0;
}

// Single process, one handle per device (ncclCommInitAll)
extern "C" int paxisim_dist_init(paxisim* const* handles, int n, paxisim_dist** out) {
  if (!handles || n < 1 || !out) return fail(PAXISIM_EINVAL, "bad argument");
  if (!rccl().ok) return fail(PAXISIM_EUNSUPP, "RCCL (librccl.so.1) not available");
  std::vector<int> devs;
  for (int i = 0; i < n; i++) {
    if (!handles[i]) return fail(PAXISIM_EINVAL, "null handle %d", i);
    for (int d : devs)
      if (d == handles[i]->cfg.device) return fail(PAXISIM_EINVAL, "two handles on device %d", d);
    devs.push_back(handles[i]->cfg.device);
  }
  paxisim_dist* d = new (std::nothrow) paxisim_dist();
  if (!d) return fail(PAXISIM_ENOMEM, "oom");
  d->h.assign(handles, handles + n);
  d->comm.resize(n);
  ncclResult_t r = rccl().init_all(d->comm.data(), n, devs.data());
  if (r != ncclSuccess) {
    d->comm.clear();
    paxisim_dist_destroy(d);
    return fail(PAXISIM_EDEVICE, "ncclCommInitAll: %s", rccl().error_string(r));
  }
  int rc = dist_alloc(d);
  if (rc) {
    paxisim_dist_destroy(d);
    return rc;
  }
  *out = d;
  return 0;
}

// One handle per process: every rank passes the id one rank obtained from
// paxisim_dist_unique_id (the caller ships it, e.g. over its launcher)
extern "C" int paxisim_dist_init_rank(paxisim* h, const unsigned char id[128], int nranks, int rank,
                                      paxisim_dist** out) {
  if (!h || !id || nranks < 1 || rank < 0 || rank >= nranks || !out) return fail(PAXISIM_EINVAL, "bad argument");
  if (!rccl().ok) return fail(PAXISIM_EUNSUPP, "RCCL (librccl.so.1) not available");
  if (const int jrc = enter(h)) return jrc;
  paxisim_dist* d = new (std::nothrow) paxisim_dist();
  if (!d) return fail(PAXISIM_ENOMEM, "oom");
  d->h.push_back(h);
  d->comm.resize(1);
  ncclUniqueId u;
  memcpy(u.internal, id, NCCL_UNIQUE_ID_BYTES);
  ncclResult_t r = rccl().init_rank(&d->comm[0], nranks, u, rank);
  if (r != ncclSuccess) {
    d->comm.clear();
    paxisim_dist_destroy(d);
    return fail(PAXISIM_EDEVICE, "ncclCommInitRank: %s", rccl().error_string(r));
  }
  int rc = dist_alloc(d);
  if (rc) {
    paxisim_dist_destroy(d);
    return rc;
  }
  *out = d;
  return 0;
}

// Sum sums_in[i] (i < n) and max maxes_in[j] (j < m) over every member of
// every rank; member k's inputs are at sums_in[k*n], maxes_in[k*m].  The
// result (the same on every member) goes to sums_out[0..n), maxes_out[0..m).
extern "C" int paxisim_dist_allreduce(paxisim_dist* d, const uint64_t* sums_in, uint32_t n, const double* maxes_in,
                                      uint32_t m, uint64_t* sums_out, double* maxes_out) {
  if (!d || n > DIST_MAXV || m > DIST_MAXV || (n && (!sums_in || !sums_out)) || (m && (!maxes_in || !maxes_out)))
    return fail(PAXISIM_EINVAL, "bad argument");
  const size_t k = d->h.size();
  for (size_t i = 0; i < k; i++) {
    paxisim* h = d->h[i];
    if (const int jrc = enter(h)) return jrc;
    uint64_t* b = static_cast<uint64_t*>(d->buf[i]);
    if (n) HIPCHK(hipMemcpyAsync(b, sums_in + i * n, n * 8, hipMemcpyHostToDevice, h->stream));
    if (m) HIPCHK(hipMemcpyAsync(b + DIST_MAXV, maxes_in + i * m, m * 8, hipMemcpyHostToDevice, h->stream));
  }
  RCCLCHK(rccl().group_start());
  for (size_t i = 0; i < k; i++) {
    uint64_t* b = static_cast<uint64_t*>(d->buf[i]);
    if (n) (void)rccl().all_reduce(b, b, n, ncclUint64, ncclSum, d->comm[i], d->h[i]->stream);
    if (m) (void)rccl().all_reduce(b + DIST_MAXV, b + DIST_MAXV, m, ncclFloat64, ncclMax, d->comm[i], d->h[i]->stream);
  }
  RCCLCHK(rccl().group_end());
  for (size_t i = 0; i < k; i++) {
    paxisim* h = d->h[i];
    if (const int jrc = enter(h)) return jrc;
    uint64_t* b = static_cast<uint64_t*>(d->buf[i]);
    if (i == 0 && n) HIPCHK(hipMemcpyAsync(sums_out, b, n * 8, hipMemcpyDeviceToHost, h->stream));
    if (i == 0 && m) HIPCHK(hipMemcpyAsync(maxes_out, b + DIST_MAXV, m * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

// paxisim_stats summed over every handle of the job (u64 fields), and the
// largest step-kernel time of any handle (kernel_ms_max may be NULL)
extern "C" int paxisim_dist_stats(paxisim_dist* d, paxisim_stats* out, double* kernel_ms_max) {
  if (!d || !out) return fail(PAXISIM_EINVAL, "null argument");
  constexpr uint32_t NV = sizeof(paxisim_stats) / sizeof(uint64_t);
  static_assert(sizeof(paxisim_stats) % sizeof(uint64_t) == 0 && NV <= DIST_MAXV, "stats layout");
  const size_t k = d->h.size();
  std::vector<uint64_t> in(k * NV);
  std::vector<double> tin(k);
  for (size_t i = 0; i < k; i++) {
    paxisim_stats s;
    int rc = paxisim_stats_get(d->h[i], &s);
    if (rc) return rc;
    memcpy(&in[i * NV], &s, sizeof s);
    double ms = 0;
    if ((rc = paxisim_kernel_time(d->h[i], &ms, nullptr, 0))) return rc;
    tin[i] = ms;
  }
  uint64_t res[NV];
  double tmax = 0;
  int rc = paxisim_dist_allreduce(d, in.data(), NV, tin.data(), 1, res, &tmax);
  if (rc) return rc;
  memcpy(out, res, sizeof *out);
  if (kernel_ms_max) *kernel_ms_max = tmax;
  return 0;
}

#if (defined(PXS_WAVE_TIMES) || defined(PXS_TALLY)) && !defined(PXS_STAMPS)
constexpr uint32_t DBG_PER = 48;   // the stamps build's buffer size (paxisim_dev.h); two words per block used
#endif
#if defined(PXS_STAMPS) || defined(PXS_WAVE_TIMES) || defined(PXS_TALLY)
// Diagnostic builds only: per (block, replica) {setup, loop, barrier cycles, loop trips, records, steps}
// (PXS_STAMPS), per block the serial kernel's start and end clock (PXS_WAVE_TIMES, tools/wave_times.py), or
// per block the access-class tallies (PXS_TALLY, tools/tally.py).
extern "C" int paxisim_dbg_enable(paxisim* h) {
  if (const int jrc = enter(h)) return jrc;
  const size_t n = (h->P.C / LANES) * 16 * DBG_PER;
  HIPCHK(hipMalloc(&h->P.dbg, n * 8));
  HIPCHK(hipMemset(h->P.dbg, 0, n * 8));
  return 0;
}
extern "C" int paxisim_dbg_read(paxisim* h, unsigned long long* out) {
  if (const int jrc = enter(h)) return jrc;
  HIPCHK(hipStreamSynchronize(h->stream));
  const size_t n = (h->P.C / LANES) * 16 * DBG_PER;
  HIPCHK(hipMemcpy(out, h->P.dbg, n * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(h->P.dbg, 0, n * 8));
  return 0;
}
#endif
