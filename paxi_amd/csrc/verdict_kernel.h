// verdict_kernel.h — per-cluster verdict words and the ordered search over them
// (include/paxisim_verdict.h).
//
// The verdict pass: one lane per local cluster id.  It reads the cluster's slot (slot_of), the
// replicas' flags, the agreement verdict (agree_bad, the body check_kernel counts with), the worker
// table and the u8 mailbox counts of the tile image, ORs in what the requested scans left per
// cluster id, and writes words[id].  Nothing here is part of a step: the kernels take their buffers
// as arguments and Params has no field for them.
//
// The select: an ordered stream compaction of the ids whose word matches a predicate, in three
// launches.  select_count writes each workgroup's match count (a wave64 ballot and a popcount per
// wave), select_scan turns the counts into exclusive offsets in one workgroup, select_scatter
// recomputes the ballots and writes id i at offset[workgroup] + the earlier waves' counts + the
// matching lanes below it.  The output is ascending and the same on every run; no position comes
// from an atomic and no workgroup waits for another.  Writes at positions >= cap are dropped; the
// total is the scan's.
#pragma once
#include "paxisim_dev.h"
#include "chist_kernel.h"
#include "mv_kernel.h"
#include "../../include/paxisim_verdict.h"

namespace pxs {

constexpr uint32_t SEL_WG = 256;      // words per select workgroup, one a lane
constexpr uint32_t SEL_SCAN = 1024;   // workgroup counts per iteration of select_scan
constexpr uint32_t SEL_WAVES = SEL_WG / 64u;

// Agreement of the cluster at slot c (client.go:279-320; tla/wpaxos.tla Safety): replicas that
// executed the same number of slots must hold the same digest, and digest checkpoints taken at the
// same executed count must agree.  Not for EPaxos, which has no single log (paxisim.h).
__device__ inline bool agree_bad(const Params& P, uint64_t c) {
  bool bad = false;
  for (uint32_t r = 0; r < P.N; r++) bad |= P.stats[krc(P, ST_AGB, r, c)] != 0;   // running check (paxos_exec)
  auto exec_digest = [&](uint32_t key, uint32_t r, uint32_t& e, uint64_t& d) {
    if (P.protocol == PAXISIM_WPAXOS) {
      uint4 a, b;
      wp_read(P, c / LANES, key, r, (uint32_t)(c % LANES), a, b);
      e = a.z;
      d = (uint64_t)b.y | ((uint64_t)b.z << 32);
    } else {
      e = P.execute[rc(P, r, c)];
      d = P.digest[rc(P, r, c)];
    }
  };
  auto ck = [&](uint32_t k, uint32_t inst) { return ((size_t)k * P.NI + inst) * P.C + c; };
  for (uint32_t key = 0; key < P.NK && !bad; key++)       // per Paxos instance (WPaxos: per key)
    for (uint32_t a = 0; a < P.N && !bad; a++)
      for (uint32_t b = a + 1; b < P.N && !bad; b++) {
        uint32_t ea, eb;
        uint64_t da, db;
        exec_digest(key, a, ea, da);
        exec_digest(key, b, eb, db);
        if (ea == eb && da != db) bad = true;
        const uint32_t ia = key * P.N + a, ib = key * P.N + b;
        for (uint32_t k = 0; k < CKR && !bad; k++) {
          const uint32_t e = P.ck_e[ck(k, ia)];
          if (!e) continue;
          for (uint32_t j = 0; j < CKR && !bad; j++)
            if (P.ck_e[ck(j, ib)] == e && P.ck_d[ck(k, ia)] != P.ck_d[ck(j, ib)]) bad = true;
        }
      }
  return bad;
}

// What the scans left for the pass, all indexed by the local cluster id (null: scan not requested).
struct VerdictScans {
  const unsigned long long* mv_masks;   // mv_consensus_kernel's failing-key masks
  const uint32_t* marks;                // PAXISIM_V_LIN / CLIENT_LIN / LIN_SKIPPED bits set by the lin kernels
  uint32_t scans;                       // the requested PAXISIM_V_* scan bits
  uint32_t started;                     // 1: every worker's start_step has passed
};

__global__ void __launch_bounds__(256) verdict_kernel(Params P, VerdictScans in, uint32_t* words) {
  const uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= P.clusters) return;
  const uint64_t c = slot_of(P, id);
  const uint32_t lane = (uint32_t)(c % LANES);
  const uint8_t* img = P.image + (c / LANES) * (size_t)P.img.bytes;
  uint32_t w = 0;
  for (uint32_t r = 0; r < P.N; r++) w |= P.flags[rc(P, r, c)];
  w &= 0xFFu;
  if (P.protocol != PAXISIM_EPAXOS && agree_bad(P, c)) w |= PAXISIM_V_AGREE;
  if (in.mv_masks) {
    if (in.mv_masks[id]) w |= PAXISIM_V_CONSENSUS;
    bool cut = false;
    for (uint32_t k = 0; k < P.keys; k++)
      for (uint32_t r = 0; r < P.N; r++) cut |= P.mv_cnt[mv_row(P, k, r, id)] > P.mv_cap;
    if (cut) w |= PAXISIM_V_TRUNCATED;
  }
  if (in.marks) w |= in.marks[id];
  if (in.scans & PAXISIM_V_CLIENT_LIN) {
    bool cut = false;
    for (uint32_t wk = 0; wk < P.WK; wk++) cut |= P.ch_cnt[chist_row(P, wk, id)] > P.ch_cap;
    if (cut) w |= PAXISIM_V_TRUNCATED;
  }
  const uint32_t* wcur = reinterpret_cast<const uint32_t*>(img + P.img.off_wcur);
  bool waiting = false;
  for (uint32_t wk = 0; wk < P.WK; wk++) waiting |= wcur[(wk << 6) | lane] != 0;
  const uint8_t* cnt = img + P.img.off_cnt;
  const uint32_t nbox = P.D * P.N * P.NS;   // every arrival step, destination and source, the client's included
  uint32_t held = 0;
  for (uint32_t b = 0; b < nbox; b++) held |= cnt[(b << 6) | lane];
  const bool quiet = held == 0 && in.started && !(w & PAXISIM_F_POISON);
  if (quiet) w |= PAXISIM_V_QUIET;
  if (waiting) w |= PAXISIM_V_WAITING;
  if (quiet && waiting) w |= PAXISIM_V_STALLED;
  words[id] = w;
}

// counts[b] += the words of [0, n) with bit b set: a ballot per bit, lane b keeps bit b's count, then
// one atomic per wave and bit that has any.
__global__ void __launch_bounds__(256) verdict_count_kernel(const uint32_t* words, uint64_t n, unsigned long long* counts) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t w = i < n ? words[i] : 0u;
  uint32_t mine = 0;
  for (uint32_t b = 0; b < 32; b++) {
    const uint32_t k = (uint32_t)__popcll(__ballot((w >> b) & 1u));
    if (lane == b) mine = k;
  }
  if (lane < 32 && mine) atomicAdd(&counts[lane], (unsigned long long)mine);
}

__device__ __forceinline__ bool select_match(uint32_t w, uint32_t any, uint32_t none) {
  return (any == 0 || (w & any) != 0) && (w & none) == 0;
}

// per_wg[g]: the matches among words [g * SEL_WG, (g + 1) * SEL_WG)
__global__ void __launch_bounds__(SEL_WG) select_count(const uint32_t* words, uint64_t n, uint32_t any, uint32_t none,
                                                        unsigned long long* per_wg) {
  __shared__ uint32_t wc[SEL_WAVES];
  const uint64_t i = (uint64_t)blockIdx.x * SEL_WG + threadIdx.x;
  const uint64_t m = __ballot(i < n && select_match(words[i < n ? i : 0], any, none));
  if ((threadIdx.x & 63u) == 0) wc[threadIdx.x >> 6] = (uint32_t)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (uint32_t k = 0; k < SEL_WAVES; k++) s += wc[k];
    per_wg[blockIdx.x] = s;
  }
}

// Exclusive scan of the workgroup counts in place (one workgroup of SEL_SCAN lanes, SEL_SCAN counts
// an iteration with a running carry); the grand total to *total.
__global__ void __launch_bounds__(SEL_SCAN) select_scan(unsigned long long* per_wg, uint64_t nwg, unsigned long long* total) {
  __shared__ unsigned long long sh[SEL_SCAN];
  __shared__ unsigned long long carry;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (uint64_t base = 0; base < nwg; base += SEL_SCAN) {
    const unsigned long long v = base + tid < nwg ? per_wg[base + tid] : 0ull;
    sh[tid] = v;
    __syncthreads();
    for (uint32_t off = 1; off < SEL_SCAN; off <<= 1) {
      const unsigned long long t = tid >= off ? sh[tid - off] : 0ull;
      __syncthreads();
      sh[tid] += t;
      __syncthreads();
    }
    if (base + tid < nwg) per_wg[base + tid] = carry + sh[tid] - v;
    __syncthreads();
    if (tid == 0) carry += sh[SEL_SCAN - 1];
    __syncthreads();
  }
  if (tid == 0) *total = carry;
}

// ids[rank] = i for every matching word i whose rank (its position among the matches) is below cap
__global__ void __launch_bounds__(SEL_WG) select_scatter(const uint32_t* words, uint64_t n, uint32_t any, uint32_t none,
                                                          const unsigned long long* offs, unsigned long long* ids,
                                                          uint64_t cap) {
  __shared__ uint32_t wc[SEL_WAVES];
  const uint64_t i = (uint64_t)blockIdx.x * SEL_WG + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const bool hit = i < n && select_match(words[i < n ? i : 0], any, none);
  const uint64_t m = __ballot(hit);
  if (lane == 0) wc[wave] = (uint32_t)__popcll(m);
  __syncthreads();
  if (!hit) return;
  uint64_t rank = offs[blockIdx.x] + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
  for (uint32_t k = 0; k < wave; k++) rank += wc[k];
  if (rank < cap) ids[rank] = i;
}

}  // namespace pxs
