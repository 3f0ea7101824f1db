// paxisim.hip — C-ABI (include/paxisim.h) over the gfx950 simulation kernels.
//
// Product path: everything here runs on the GPU.  There is no CPU fallback;
// a handle whose device cannot be initialised fails paxisim_create with
// PAXISIM_EDEVICE.
//
// This unit: the handle's lifecycle, step scheduling, compaction and phase binning, cluster pools,
// the pipeline and the core readouts, with their kernels.  host.h names the other host units.
#include "host.h"
#include "epaxos_kernel.h"
#include "sim_core.h"
#include "pool_plan.h"
#include "shape_plan.h"
#include "snapshot_plan.h"
#include "../../include/paxisim_shape.h"

using namespace pxs;
using namespace pxs_host;

static_assert(PLAN_EP_NMAX == EP_NMAX, "create_plan.h check_config: the EPaxos replica limit");

extern "C" int paxisim_abi_version(void) { return PAXISIM_ABI_VERSION; }
extern "C" const char* paxisim_last_error(void) { return g_err; }

// ---------------------------------------------------------------------------
// kernels: init, stats reduction, state gather
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
constexpr uint32_t CB = 1024;                    // slots per counting block (the words of Pool::d_cmp: host.h CM_*)

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
// Every entry point but paxisim_step works on the handle's stream.  With two pools it first makes
// that stream wait for what the pools' streams have been given (an event on each), and notes that
// the next paxisim_step must make the pools' streams wait for the handle's; consecutive steps with
// nothing between them add no dependency between streams.
int pxs_host::enter(paxisim* h) {
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
  for (const SnapBuf& b : snap_recorder_bufs(h->P, h->tr_rows))
    if (b.ptr) (void)hipFree(b.ptr);
  if (h->d_lat_out) (void)hipFree(h->d_lat_out);
  if (h->P.tr_row) (void)hipFree(const_cast<uint32_t*>(h->P.tr_row));
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
StepOps pxs_host::lat_step_ops_for(uint32_t protocol, uint32_t N, bool wlds, bool serial) {
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
void pxs_host::select_unit(paxisim* h) {
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
int pxs_host::create_on_device(paxisim* h, const Knobs& kn, uint32_t variant, uint32_t N) {
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
  hipError_t e;
  {
    DevBuf pad;
    if (kn.arena_pad_mb > 0) (void)pad.alloc<char>((size_t)kn.arena_pad_mb << 20);
    e = kn.arena_contig ? hipExtMallocWithFlags(&h->arena, sz.total, hipDeviceMallocContiguous)
                        : hipMalloc(&h->arena, sz.total);
  }
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
int pxs_host::pipe_check(paxisim* h) {
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

int pxs_host::enter_checked(paxisim* h) {
  if (const int jrc = enter(h)) return jrc;
  return pipe_check(h);
}

// What snapshot, restore, fork and the verdicts do first: join the pools, check the pipelined
// launches, sync the stream.
int pxs_host::quiesce(paxisim* h) {
  if (const int jrc = enter(h)) return jrc;
  for (uint32_t p = 0; p < h->npools; p++) HIPCHK(hipStreamSynchronize(h->pool[p].stream));
  if (const int rc = pipe_check(h)) return rc;   // a sticky pipeline error refuses
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
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
  HIPCHK(read_back(h, &slot, P.slot_of + cluster, 4));
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
  if (const int rc = enter_checked(h)) return rc;   // results only of launches that fully ran
  const uint32_t n = h->P.WK;
  *n_out = n;
  if (!cap || !n) return 0;
  DevBuf d;
  HIPCHK(d.alloc<paxisim_worker_state>(n));
  read_client_kernel<<<1, 64, 0, h->stream>>>(h->P, cluster, d.as<paxisim_worker_state>());
  HIPCHK(hipGetLastError());
  std::vector<paxisim_worker_state> tmp(n);
  HIPCHK(read_back(h, tmp.data(), d.p, n * sizeof(paxisim_worker_state)));
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
  if (const int rc = enter_checked(h)) return rc;   // results only of launches that fully ran
  DevBuf d;
  HIPCHK(d.alloc<uint32_t>(n));
  read_kv_kernel<<<(n + 63) / 64, 64, 0, h->stream>>>(h->P, cluster, replica, n, d.as<uint32_t>());
  HIPCHK(hipGetLastError());
  HIPCHK(read_back(h, values, d.p, n * sizeof(uint32_t)));
  return 0;
}

extern "C" int paxisim_active_clusters(paxisim* h, uint64_t* active) {
  if (!h || !active) return fail(PAXISIM_EINVAL, "null argument");
  if (const int rc = enter_checked(h)) return rc;   // results only of launches that fully ran
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
  if (const int rc = enter_checked(h)) return rc;   // results only of launches that fully ran
  DevBuf d;
  HIPCHK(d.alloc<uint32_t>(n));
  activity_kernel<<<(unsigned)((n + 255) / 256), 256, 0, h->stream>>>(
      h->P, lo, n, d.as<uint32_t>(), h->npools > 1 ? h->pool[1].d_cmp : h->P.bound,
      h->npools > 1 ? (uint64_t)h->pool[1].base : ~0ull);
  HIPCHK(hipGetLastError());
  HIPCHK(read_back(h, frozen_at, d.p, n * sizeof(uint32_t)));
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
  HIPCHK(read_back(h, &st, h->d_scratch, sizeof st));
  if (st) return fail(PAXISIM_EINVAL, "client mailbox full");
  return 0;
}

extern "C" int paxisim_read_inbox(paxisim* h, uint64_t cluster, uint32_t replica, paxisim_inbox_record* out,
                                  uint32_t cap, uint32_t* n_out) {
  if (!h || !n_out || (cap && !out)) return fail(PAXISIM_EINVAL, "null argument");
  if (cluster >= h->cfg.clusters || replica >= h->P.N) return fail(PAXISIM_ERANGE, "bad inbox");
  if (const int rc = enter_checked(h)) return rc;   // results only of launches that fully ran
  HIPCHK(hipStreamSynchronize(h->stream));
  const uint32_t maxn = h->P.NS * h->P.M;   // a bucket set holds at most this many
  DevBuf buf;   // the records, then their count
  HIPCHK(buf.alloc<char>(maxn * sizeof(paxisim_inbox_record) + 64));
  paxisim_inbox_record* d = buf.as<paxisim_inbox_record>();
  uint32_t* dn = reinterpret_cast<uint32_t*>(buf.as<char>() + maxn * sizeof(paxisim_inbox_record));
  read_inbox_kernel<<<1, 64, 0, h->stream>>>(h->P, cluster, replica, h->t % h->P.D, d, maxn, dn);
  HIPCHK(hipGetLastError());
  uint32_t n = 0;
  HIPCHK(read_back(h, &n, dn, sizeof n));
  if (cap) HIPCHK(hipMemcpy(out, d, (n < cap ? n : cap) * sizeof(paxisim_inbox_record), hipMemcpyDeviceToHost));
  *n_out = n;
  return 0;
}

extern "C" int paxisim_commands(paxisim* h, uint64_t cluster, const uint32_t* cids, uint32_t n, uint32_t* keys,
                                uint32_t* writes) {
  if (!h || (n && (!cids || !keys || !writes))) return fail(PAXISIM_EINVAL, "null argument");
  if (cluster >= h->cfg.clusters) return fail(PAXISIM_ERANGE, "bad cluster");
  if (n == 0) return 0;
  if (const int rc = enter_checked(h)) return rc;   // results only of launches that fully ran
  DevBuf buf;   // the ids, their keys, their kinds
  HIPCHK(buf.alloc<uint32_t>(3ull * n));
  uint32_t* d = buf.as<uint32_t>();
  HIPCHK(hipMemcpyAsync(d, cids, n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
  command_kernel<<<(n + 255) / 256, 256, 0, h->stream>>>(h->P, cluster, d, n, d + n, d + 2 * n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(keys, d + n, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(read_back(h, writes, d + 2 * n, n * sizeof(uint32_t)));
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
  DevBuf d;
  HIPCHK(d.alloc<paxisim_inbox_record>(n));
  HIPCHK(hipMemcpyAsync(d.p, recs, n * sizeof(paxisim_inbox_record), hipMemcpyHostToDevice, h->stream));
  uint32_t st = 0;
  deliver_kernel<<<1, 64, 0, h->stream>>>(h->P, cluster, replica, src, h->t % h->P.D, d.as<paxisim_inbox_record>(), n,
                                          (uint32_t*)h->d_scratch);
  HIPCHK(hipGetLastError());
  HIPCHK(read_back(h, &st, h->d_scratch, sizeof st));
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
  if (const int rc = enter_checked(h)) return rc;   // results only of launches that fully ran
  DevBuf d;
  HIPCHK(d.alloc<paxisim_log_entry>(n));
  read_log_kernel<<<(n + 63) / 64, 64, 0, h->stream>>>(h->P, cluster, replica, key, slot_lo, n, d.as<paxisim_log_entry>());
  HIPCHK(hipGetLastError());
  HIPCHK(read_back(h, out, d.p, n * sizeof(paxisim_log_entry)));
  for (uint32_t i = 0; i < n; i++) out[i].ballot = expand_ballot(h, (uint32_t)out[i].ballot);
  return 0;
}

extern "C" int paxisim_stats_get(paxisim* h, paxisim_stats* out) {
  if (!h || !out) return fail(PAXISIM_EINVAL, "null argument");
  if (const int rc = enter_checked(h)) return rc;   // results only of launches that fully ran
  uint64_t red[NRED];
  HIPCHK(hipMemsetAsync(h->d_scratch, 0, sizeof(uint64_t) * NRED, h->stream));
  stats_kernel<<<(unsigned)(h->P.C / 256 + 1), 256, 0, h->stream>>>(h->P, h->d_scratch);
  HIPCHK(hipGetLastError());
  HIPCHK(read_back(h, red, h->d_scratch, sizeof red));
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
  if (const int rc = enter_checked(h)) return rc;   // results only of launches that fully ran
  const size_t cnt = (size_t)n * h->P.N;
  DevBuf d;
  HIPCHK(d.alloc<paxisim_replica_state>(cnt));
  gather_kernel<<<(unsigned)((cnt + 255) / 256), 256, 0, h->stream>>>(h->P, lo, n, d.as<paxisim_replica_state>());
  HIPCHK(hipGetLastError());
  HIPCHK(read_back(h, out, d.p, cnt * sizeof(paxisim_replica_state)));
  for (size_t i = 0; i < cnt; i++) out[i].ballot = expand_ballot(h, (uint32_t)out[i].ballot);
  return 0;
}

extern "C" int paxisim_read_instances(paxisim* h, uint64_t lo, uint64_t n, paxisim_instance_state* out) {
  if (!h || !out) return fail(PAXISIM_EINVAL, "null argument");
  if (lo + n > h->cfg.clusters || lo + n < lo) return fail(PAXISIM_ERANGE, "cluster range");
  if (n == 0) return 0;
  if (const int rc = enter_checked(h)) return rc;   // results only of launches that fully ran
  const uint32_t ni = h->P.protocol == PAXISIM_EPAXOS ? h->P.N * h->P.N : h->P.NI;   // per cluster; EPaxos: (replica, owner log)
  const size_t cnt = (size_t)n * ni;
  DevBuf d;
  HIPCHK(d.alloc<paxisim_instance_state>(cnt));
  gather_inst_kernel<<<(unsigned)((cnt + 255) / 256), 256, 0, h->stream>>>(h->P, lo, n, d.as<paxisim_instance_state>());
  HIPCHK(hipGetLastError());
  HIPCHK(read_back(h, out, d.p, cnt * sizeof(paxisim_instance_state)));
  for (size_t i = 0; i < cnt; i++) out[i].ballot = expand_ballot(h, (uint32_t)out[i].ballot);
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
  // the arena, the recorders' buffers, and what the handle keeps beside them: the folded latency
  // readout and the trace's row table
  const Params& P = h->P;
  uint64_t b = h->arena_bytes;
  for (const SnapBuf& s : snap_recorder_bufs(P, h->tr_rows)) b += s.bytes;
  if (P.lat_bins) b += sizeof(unsigned long long) * P.WK * lat_row(P.lat_bins);
  if (P.tr_cap) b += snap_tr_row_bytes(P);
  *bytes = b;
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
