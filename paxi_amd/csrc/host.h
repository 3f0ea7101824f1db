// host.h — the host runtime's internal header: the handle, the error macro and the device-buffer
// owner every host unit uses, and the few functions more than one unit calls.  The units:
//   paxisim.hip        handle lifecycle, step scheduling, compaction, pools, the core readouts
//   host_check.hip     the recorders and the checks over them: latency, histories and the
//                      linearizability scans, multiversion / Consensus, traces, verdicts
//   host_snapshot.hip  snapshot, restore, fork
//   host_dist.hip      the RCCL layer
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <new>
#include <utility>
#include <algorithm>
#include <vector>

#include "paxisim_dev.h"
#include "create_plan.h"
#include "step_ops.h"

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
enum { CM_BOUND = 0, CM_LNEW, CM_NPAIRS, CM_LIVE, CM_LBL, CM_SUMS = 8 };   // the words of Pool::d_cmp

struct paxisim {
  paxisim_config cfg;
  paxisim_workload wl;
  paxisim_fault_process fp;
  pxs::Params P;
  uint32_t zone_of[PAXISIM_MAX_N], node_of[PAXISIM_MAX_N];
  std::vector<pxs::DevFault> faults;
  pxs::DevFault* d_faults = nullptr;
  uint32_t* d_move = nullptr;      // moving-Mu key CDF tables (paxisim_workload.move_cdf)
  void* arena = nullptr;
  size_t arena_bytes = 0;
  uint64_t* d_scratch = nullptr;   // reductions
  hipStream_t stream = nullptr;
  pxs::StepOps ops{};
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
  Pool pool[pxs::MAX_POOLS];
  uint32_t npools = 1;
  hipEvent_t ev_main = nullptr;    // join: the handle's stream so far
  bool pools_ahead = false;        // steps were launched since the last join
  bool main_ahead = false;         // the handle's stream was used since the last step
  uint32_t late_until = 0;         // no compaction before every late worker has started
  uint32_t bound_host = 0;         // last bound read back (diagnostics)
  uint64_t lin_big = 0, lin_nmax = 0;   // last linearizability scan: partitions above LIN_SMAX, largest
  // The recorders' buffers are P's (snapshot_plan.h snap_recorder_bufs lists them); beside them the
  // handle keeps the folded latency readout [WK][bins + LAT_EXTRA] (lat_kernel.h) ...
  unsigned long long* d_lat_out = nullptr;
  // ... and of the device message trace (trace_kernel.h) the clusters traced and P.tr_row's host copy
  uint32_t tr_rows = 0;
  std::vector<uint32_t> tr_row;
  pxs::Knobs kn;                   // the create-time knobs as create read them (paxisim_fork creates with them)
};

static inline size_t rc_host(const pxs::Params& P, uint32_t r, uint64_t c) { return (size_t)r * P.C + c; }

// compressed (n << 4) | r  ->  the 64-bit Ballot of ballot.go:15-17
static inline uint64_t expand_ballot(const paxisim* h, uint32_t b) {
  if (!b) return 0;
  const uint32_t id = b & 15u;
  return ((uint64_t)(b >> 4) << 32) | ((uint64_t)h->zone_of[id] << 16) | h->node_of[id];
}

// A device allocation freed at scope exit: every temporary of the host runtime is one, so an entry
// point checks each call with HIPCHK and returns where it fails.
struct DevBuf {
  void* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  // `count` elements of T in place of what the buffer held
  template <class T>
  hipError_t alloc(size_t count) {
    if (p) (void)hipFree(p);
    p = nullptr;
    return hipMalloc(&p, count * sizeof(T));
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};

// The readout's last step: `bytes` of a filled device buffer to the host on the handle's stream,
// complete on return.
static inline hipError_t read_back(paxisim* h, void* dst, const void* src, size_t bytes) {
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream);
  return e != hipSuccess ? e : hipStreamSynchronize(h->stream);
}

// a wave's sum in its lane 0 (the reduction kernels of paxisim.hip and host_check.hip)
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// What more than one unit calls (paxisim.hip defines them).  The linearizability scans and the
// verdicts that call them are both host_check.hip's, so lin_scan stays a static template there.
namespace pxs_host {
int enter(paxisim* h);         // every entry point but paxisim_step: the device, and the pools joined to the handle's stream
int pipe_check(paxisim* h);    // a pipelined launch that did not fully run refuses the readout
int enter_checked(paxisim* h); // enter, then pipe_check: what a readout does first
int quiesce(paxisim* h);       // enter, pipe_check and every stream idle
void select_unit(paxisim* h);
pxs::StepOps lat_step_ops_for(uint32_t protocol, uint32_t N, bool wlds, bool serial);
int create_on_device(paxisim* h, const pxs::Knobs& kn, uint32_t variant, uint32_t N);
}  // namespace pxs_host
