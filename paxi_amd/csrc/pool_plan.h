// pool_plan.h — which step launches a paxisim_step call makes (host only, no HIP types).
//
// A handle steps one or two cluster pools.  Each pool fuses
// whole chunks of S steps into pipelined launches of at most pipe_max chunks,
// none past a compaction that is due for that pool, and compacts where one is
// due - the loop paxisim_step has always run, once per pool.  Pool p starts
// with last_cmp = p * S and compacts no earlier than late_until + p * S, so the
// pools' compactions, and with them their launch boundaries, stay one chunk
// apart.  Every pool ends the call at t + nsteps.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace pxs {

constexpr uint32_t MAX_POOLS = 2;

struct PoolLaunch {
  uint32_t pool;     // which pool steps
  uint32_t t0;       // first step of the launch
  uint32_t n;        // steps per chunk
  uint32_t chunks;   // chunks fused into the launch (1: a plain launch)
  bool compact;      // the pool compacts after this launch, at t0 + chunks * n
};

struct PoolPlanIn {
  uint32_t t = 0, nsteps = 0;
  uint32_t S = 1;              // steps per chunk
  uint32_t pipe_max = 1;       // chunks per launch at most (1: not pipelined)
  uint32_t cmp_every = 1;      // steps between a pool's compactions
  uint32_t late_until = 0;     // no compaction before this step
  bool compact = false;        // the handle compacts at all
  uint32_t npools = 1;
  uint32_t last_cmp[MAX_POOLS] = {0, 0};   // updated by pool_plan
};

// the step before which pool p does not compact
inline uint32_t pool_late_until(const PoolPlanIn& in, uint32_t p) { return in.late_until + p * in.S; }
// last_cmp of pool p of a new handle
inline uint32_t pool_first_cmp(uint32_t p, uint32_t S) { return p * S; }

inline bool pool_due(const PoolPlanIn& in, uint32_t p, uint32_t last_cmp, uint32_t t) {
  return in.compact && t >= pool_late_until(in, p) && t >= last_cmp && t - last_cmp >= in.cmp_every;
}

// The launches of one call, the pools' sequences merged by start step (pool 0 first on ties), so the
// host enqueues them alternately; in.last_cmp is left at each pool's last compaction.
inline std::vector<PoolLaunch> pool_plan(PoolPlanIn& in) {
  std::vector<PoolLaunch> seq[MAX_POOLS];
  const uint32_t S = in.S ? in.S : 1u;
  for (uint32_t p = 0; p < in.npools && p < MAX_POOLS; p++) {
    uint32_t t = in.t, left = in.nsteps, last = in.last_cmp[p];
    while (left > 0) {
      const uint32_t n = left < S ? left : S;
      uint32_t K = 1;
      if (in.pipe_max > 1 && n == S)
        while (K < in.pipe_max && (uint64_t)(K + 1u) * n <= left && !pool_due(in, p, last, t + K * n)) K++;
      t += K * n;
      left -= K * n;
      const bool c = pool_due(in, p, last, t);
      if (c) last = t;
      seq[p].push_back(PoolLaunch{p, t - K * n, n, K, c});
    }
    in.last_cmp[p] = last;
  }
  std::vector<PoolLaunch> out;
  size_t i[MAX_POOLS] = {0, 0};
  for (;;) {
    int pick = -1;
    for (uint32_t p = 0; p < in.npools && p < MAX_POOLS; p++)
      if (i[p] < seq[p].size() && (pick < 0 || seq[p][i[p]].t0 < seq[pick][i[pick]].t0)) pick = (int)p;
    if (pick < 0) break;
    out.push_back(seq[pick][i[pick]++]);
  }
  return out;
}

// The region split of a handle of `tiles` 64-cluster tiles: region 0 is tiles [0, split), a multiple
// of 8 tiles as near the middle as that allows; 0 when a region would be empty (one pool).
inline uint32_t pool_split_tile(uint32_t tiles, uint64_t clusters) {
  const uint32_t s = (tiles / 2u + 4u) / 8u * 8u;
  return s == 0 || (uint64_t)s * 64u >= clusters ? 0u : s;
}

// How many pools a handle asks for.  can: it compacts and runs pipelined serial launches - every
// other handle runs one.  knob: PAXISIM_POOLS (1 or 2; 0 unset).  Without it a 5-replica handle takes
// two when its tiles are at least four times the resident wave slots (0: not known).
// pool_want_asks_slots: whether the answer depends on resident_slots (else the caller skips its
// device queries).
inline bool pool_want_asks_slots(int knob, bool can, uint32_t N) { return can && !knob && N == 5; }
inline uint32_t pool_want(int knob, bool can, uint32_t N, uint32_t tiles, uint32_t resident_slots) {
  if (pool_want_asks_slots(knob, can, N)) return resident_slots > 0 && tiles >= 4u * resident_slots ? 2u : 1u;
  return can && knob ? (uint32_t)knob : 1u;
}

// Length of the union of [start, end] intervals (any order): the time at least one launch ran.
inline double interval_union(std::vector<std::pair<double, double>> iv) {
  for (size_t a = 1; a < iv.size(); a++)   // insertion sort by start: a call has few launches
    for (size_t b = a; b > 0 && iv[b].first < iv[b - 1].first; b--) std::swap(iv[b], iv[b - 1]);
  double sum = 0, lo = 0, hi = 0;
  bool open = false;
  for (const auto& v : iv) {
    if (open && v.first <= hi) {
      if (v.second > hi) hi = v.second;
      continue;
    }
    if (open) sum += hi - lo;
    lo = v.first;
    hi = v.second > v.first ? v.second : v.first;
    open = true;
  }
  return open ? sum + (hi - lo) : sum;
}

}  // namespace pxs
