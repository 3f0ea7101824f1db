// snapshot_plan.h — the host side of snapshot / restore / fork (host only, no HIP runtime calls):
// the blob's header, the section-size arithmetic, the plan fingerprint and every validation
// paxisim_restore and paxisim_snapshot_info perform (include/paxisim_snapshot.h has the format).
// host_snapshot.hip runs these between its device calls; tests/snapshot_plan_check.cpp runs them
// without a GPU.
#pragma once
#include <array>
#include <string>
#include <vector>

#include "../../include/paxisim_snapshot.h"
#include "create_plan.h"

namespace pxs {

constexpr uint32_t SNAP_NSEC = PAXISIM_SNAPSHOT_SECTIONS;
constexpr uint32_t SNAP_LAT_SLICES = 8, SNAP_LAT_EXTRA = 4;   // = LAT_SLICES, LAT_EXTRA (lat_kernel.h; host_snapshot.hip asserts it)
constexpr uint32_t SNAP_CMP_WORDS = 8;                        // = CM_SUMS: a pool's compaction words before the block sums
constexpr uint32_t SNAP_POOL_BYTES = 48;

// The blob's first 256 bytes, field for field as include/paxisim_snapshot.h documents them.  The
// library runs on little-endian hosts only (x86-64, as the ROCm stack), so the struct is the format.
struct SnapHeader {
  char magic[8];
  uint32_t version, header_bytes;
  char build_id[32];
  uint64_t plan_hash, total_bytes;
  uint32_t protocol, n_replicas;
  uint64_t clusters, cluster_base;
  uint32_t step, recorders;
  uint64_t mailbox_records;
  uint64_t section_bytes[SNAP_NSEC];
  uint32_t lat_bins, ch_cap, mv_cap, tr_cap, tr_from, tr_to, tr_rows, n_faults, n_pools, n_plan_words;
  uint8_t zero[40];
};
static_assert(sizeof(SnapHeader) == PAXISIM_SNAPSHOT_HEADER, "the documented header is 256 bytes");
static_assert(offsetof(SnapHeader, plan_hash) == 48 && offsetof(SnapHeader, protocol) == 64 &&
              offsetof(SnapHeader, step) == 88 && offsetof(SnapHeader, mailbox_records) == 96 &&
              offsetof(SnapHeader, section_bytes) == 104 && offsetof(SnapHeader, lat_bins) == 176 &&
              offsetof(SnapHeader, zero) == 216, "the documented header offsets");
constexpr char SNAP_MAGIC[8] = {'P', 'X', 'S', 'S', 'N', 'A', 'P', 0};
inline const char* const* snap_section_names() {
  static const char* const n[SNAP_NSEC] = {"plan", "faults", "pools", "arena", "mailbox", "lat", "chist", "mv", "trace"};
  return n;
}

// The recorders of a handle, as far as a snapshot's sizes and checks need them.
struct SnapRecorders {
  uint32_t lat_bins = 0, ch_cap = 0, mv_cap = 0, tr_cap = 0, tr_from = 0, tr_to = 0, tr_rows = 0;
};
inline SnapRecorders snap_recorders(const Params& P, uint32_t tr_rows) {
  SnapRecorders r;
  r.lat_bins = P.lat_bins; r.ch_cap = P.ch_cap; r.mv_cap = P.mv_cap;
  r.tr_cap = P.tr_cap; r.tr_from = P.tr_from; r.tr_to = P.tr_to; r.tr_rows = P.tr_cap ? tr_rows : 0u;
  return r;
}

// Byte sizes of the recorder buffers (the parts of each section, in section order).
inline size_t snap_lat_stamp_bytes(const Params& P) { return sizeof(uint32_t) * P.WK * (size_t)P.C; }
inline size_t snap_lat_acc_bytes(const Params& P, uint32_t bins) {
  return sizeof(uint64_t) * SNAP_LAT_SLICES * P.WK * ((size_t)bins + SNAP_LAT_EXTRA);
}
inline size_t snap_ch_cnt_bytes(const Params& P) { return sizeof(uint32_t) * P.WK * (size_t)P.C; }
inline size_t snap_ch_ops_bytes(const Params& P, uint32_t cap) { return 16u * (size_t)P.WK * P.C * cap; }
inline size_t snap_mv_cnt_bytes(const Params& P) { return sizeof(uint32_t) * (size_t)P.keys * P.N * P.C; }
inline size_t snap_mv_val_bytes(const Params& P, uint32_t cap) { return snap_mv_cnt_bytes(P) * cap; }
inline size_t snap_tr_row_bytes(const Params& P) { return sizeof(uint32_t) * (size_t)P.C; }
inline size_t snap_tr_cnt_bytes(const Params& P, uint32_t rows) { return sizeof(uint32_t) * (size_t)rows * P.N; }
inline size_t snap_tr_rec_bytes(const Params& P, uint32_t rows, uint32_t cap) { return 32u * (size_t)rows * P.N * cap; }

// Every section's size: P after plan_lds (carve_arena gives the arena's), the handle's pools,
// faults and recorders, and the live records the count pass found.
inline void snap_sections(const Params& P, uint32_t policy, uint32_t n_plan_words, uint32_t n_faults, uint32_t n_pools,
                          const SnapRecorders& r, uint64_t mailbox_records, uint64_t out[SNAP_NSEC]) {
  Params Q = P;
  out[PAXISIM_SNAP_PLAN] = 8ull * n_plan_words;
  out[PAXISIM_SNAP_FAULTS] = (uint64_t)sizeof(DevFault) * n_faults;
  out[PAXISIM_SNAP_POOLS] = (uint64_t)SNAP_POOL_BYTES * n_pools;
  out[PAXISIM_SNAP_ARENA] = carve_arena(Q, policy, nullptr, false).zero_bytes;
  out[PAXISIM_SNAP_MAILBOX] = 16ull * mailbox_records;
  out[PAXISIM_SNAP_LAT] = r.lat_bins ? snap_lat_stamp_bytes(P) + snap_lat_acc_bytes(P, r.lat_bins) : 0;
  out[PAXISIM_SNAP_CHIST] = r.ch_cap ? snap_ch_cnt_bytes(P) + snap_ch_ops_bytes(P, r.ch_cap) : 0;
  out[PAXISIM_SNAP_MV] = r.mv_cap ? snap_mv_cnt_bytes(P) + snap_mv_val_bytes(P, r.mv_cap) : 0;
  out[PAXISIM_SNAP_TRACE] =
      r.tr_cap ? snap_tr_row_bytes(P) + snap_tr_cnt_bytes(P, r.tr_rows) + snap_tr_rec_bytes(P, r.tr_rows, r.tr_cap) : 0;
}

// The recorders' device buffers in snapshot order: the one list that snapshot, restore, fork, destroy
// and paxisim_device_bytes walk, so a recorder added here is carried by all of them.  offset: the
// buffer's place in its section; the TRACE section opens with the host-side tr_row table
// (snap_tr_row_bytes), which is not a buffer of this list.  An absent recorder's entries have no bytes.
struct SnapBuf {
  uint32_t section;
  void* ptr;
  size_t bytes, offset;
  bool present;
};
constexpr uint32_t SNAP_NBUF = 8;
inline std::array<SnapBuf, SNAP_NBUF> snap_recorder_bufs(const Params& P, uint32_t tr_rows) {
  const bool lat = P.lat_bins != 0, ch = P.ch_cap != 0, mv = P.mv_cap != 0, tr = P.tr_cap != 0;
  std::array<SnapBuf, SNAP_NBUF> b = {{
      {PAXISIM_SNAP_LAT, P.lat_stamp, snap_lat_stamp_bytes(P), 0, lat},
      {PAXISIM_SNAP_LAT, P.lat_acc, snap_lat_acc_bytes(P, P.lat_bins), 0, lat},
      {PAXISIM_SNAP_CHIST, P.ch_cnt, snap_ch_cnt_bytes(P), 0, ch},
      {PAXISIM_SNAP_CHIST, P.ch_ops, snap_ch_ops_bytes(P, P.ch_cap), 0, ch},
      {PAXISIM_SNAP_MV, P.mv_cnt, snap_mv_cnt_bytes(P), 0, mv},
      {PAXISIM_SNAP_MV, P.mv_val, snap_mv_val_bytes(P, P.mv_cap), 0, mv},
      {PAXISIM_SNAP_TRACE, P.tr_cnt, snap_tr_cnt_bytes(P, tr_rows), snap_tr_row_bytes(P), tr},
      {PAXISIM_SNAP_TRACE, P.tr_rec, snap_tr_rec_bytes(P, tr_rows, P.tr_cap), 0, tr},
  }};
  for (uint32_t i = 0; i < SNAP_NBUF; i++) {
    if (!b[i].present) b[i].bytes = 0;
    if (i && b[i].section == b[i - 1].section) b[i].offset = b[i - 1].offset + b[i - 1].bytes;
  }
  return b;
}

// ---- the plan fingerprint ---------------------------------------------------------------------
// One u64 word per decision, in a fixed order with a name each, so that a refused restore can name
// the first word that differs; arrays and tables enter as a hash of their contents.  plan_hash is
// the hash of the words.
inline uint64_t snap_mix(uint64_t h, uint64_t v) { return mix64(h ^ mix64(v + 0x9E3779B97F4A7C15ULL)); }
inline uint64_t snap_hash_u32(const uint32_t* a, size_t n) {
  uint64_t h = 0x5851F42D4C957F2DULL ^ n;
  for (size_t i = 0; i < n; i++) h = snap_mix(h, a[i]);
  return h;
}
inline uint64_t snap_hash_words(const std::vector<uint64_t>& w) {
  uint64_t h = 0x2545F4914F6CDD1DULL ^ w.size();
  for (const uint64_t v : w) h = snap_mix(h, v);
  return h;
}

// What the plan holds beside the handle's config structs and Params.
struct PlanExtra {
  size_t arena_zero = 0, arena_total = 0;
  bool serial = false, staged = false;   // the kernel form (StepOps)
  uint32_t chunk = 0;                    // steps per launch chunk (the handle's S)
  uint32_t pipe_max = 0, cmp_every = 0, late_until = 0, pipe_slots = 0;
  uint32_t npools = 1, pool1_base = 0;
  const uint32_t* move_cdf = nullptr;    // [P.move_tables][PAXISIM_MAX_KEYS] (host copy), or null
};

#define PXS_PLAN_CFG(S, A) S(protocol) S(n_zones) A(npz) S(q1) S(q2) S(fz) S(thrifty) S(ephemeral_leader) \
  S(reply_when_commit) S(adaptive) S(policy_threshold) S(window) S(mbox_cap) S(max_delay) S(keys) \
  S(steps_per_launch) S(history) S(clusters) S(cluster_base) S(seed) S(policy) S(policy_interval) S(agree_ring) S(kv)
#define PXS_PLAN_WL(S, A) S(outstanding) S(max_requests) S(write_ppm) S(locality_ppm) A(target) S(distribution) \
  S(conflicts) A(key_cdf) A(start_step) S(key_min) S(key_space) S(key_tail) S(move_every) S(move_tables) S(move_loop)
#define PXS_PLAN_FP(S, A) S(drop_ppm) S(drop_len) S(slow_ppm) S(slow_len) S(slow_min) S(slow_max)
#define PXS_PLAN_P(S, A) S(N) S(Z) S(W) S(M) S(D) S(NS) S(WK) S(NK) S(NI) S(H) S(OW) S(AR) S(C) S(img.off_a) S(img.off_b) \
  S(img.off_c) S(img.off_wcur) S(img.off_wiss) S(img.off_poison) S(img.off_cnt) S(img.bytes) S(J) S(off_stage) \
  S(lds_bytes) S(lds_tail) S(off_wscr) S(G) S(rec_per_block) S(wlds) S(wcoloc) S(off_agn) S(packed) S(compact) \
  S(phase_sort) S(phase_period) S(ph_rel) S(variant) S(q1) S(q2) S(rwc) S(ephemeral) S(kspace) S(conflict_key)
#define PXS_PLAN_X(S, A) S(arena_zero) S(arena_total) S(serial) S(staged) S(chunk) S(pipe_max) S(cmp_every) S(late_until) \
  S(pipe_slots) S(npools) S(pool1_base)

struct PlanWords {
  std::vector<uint64_t> w;
  std::vector<const char*> names;
};

// cfg: as the handle keeps it, its protocol the one the caller asked for (the variant).
inline PlanWords plan_words(const paxisim_config& cfg, const paxisim_workload& wl, const paxisim_fault_process& fp,
                            const Params& P, const PlanExtra& x) {
  PlanWords o;
#define PW_S(f) o.w.push_back((uint64_t)v.f); o.names.push_back(pre #f);
#define PW_A(f) o.w.push_back(snap_hash_u32(v.f, sizeof v.f / sizeof v.f[0])); o.names.push_back(pre #f);
#define pre "config."
  { const paxisim_config& v = cfg; PXS_PLAN_CFG(PW_S, PW_A)
    uint64_t a; memcpy(&a, &v.policy_alpha, 8); o.w.push_back(a); o.names.push_back(pre "policy_alpha"); }
#undef pre
#define pre "workload."
  { const paxisim_workload& v = wl; PXS_PLAN_WL(PW_S, PW_A) }
  o.w.push_back(x.move_cdf ? snap_hash_u32(x.move_cdf, (size_t)P.move_tables * PAXISIM_MAX_KEYS) : 0u);
  o.names.push_back(pre "move_cdf");
#undef pre
#define pre "fault_process."
  { const paxisim_fault_process& v = fp; PXS_PLAN_FP(PW_S, PW_A) }
#undef pre
#define pre "plan."
  { const Params& v = P; PXS_PLAN_P(PW_S, PW_A) }
  { const PlanExtra& v = x; PXS_PLAN_X(PW_S, PW_A) }
#undef pre
#undef PW_S
#undef PW_A
  return o;
}

// ---- writing and checking a header --------------------------------------------------------------
inline SnapHeader snap_header(const char* build_id, const PlanWords& pw, uint32_t protocol, const Params& P, uint32_t policy,
                              uint32_t t, uint32_t n_faults, uint32_t n_pools, const SnapRecorders& r,
                              uint64_t mailbox_records) {
  SnapHeader H;
  memset(&H, 0, sizeof H);
  memcpy(H.magic, SNAP_MAGIC, 8);
  H.version = PAXISIM_SNAPSHOT_VERSION;
  H.header_bytes = PAXISIM_SNAPSHOT_HEADER;
  strncpy(H.build_id, build_id, sizeof H.build_id - 1);
  H.plan_hash = snap_hash_words(pw.w);
  H.protocol = protocol;
  H.n_replicas = P.N;
  H.clusters = P.clusters;
  H.cluster_base = P.cluster_base;
  H.step = t;
  H.recorders = (r.lat_bins ? PAXISIM_SNAP_HAS_LAT : 0u) | (r.ch_cap ? PAXISIM_SNAP_HAS_CHIST : 0u) |
                (r.mv_cap ? PAXISIM_SNAP_HAS_MV : 0u) | (r.tr_cap ? PAXISIM_SNAP_HAS_TRACE : 0u);
  H.mailbox_records = mailbox_records;
  H.lat_bins = r.lat_bins; H.ch_cap = r.ch_cap; H.mv_cap = r.mv_cap;
  H.tr_cap = r.tr_cap; H.tr_from = r.tr_from; H.tr_to = r.tr_to; H.tr_rows = r.tr_rows;
  H.n_faults = n_faults;
  H.n_pools = n_pools;
  H.n_plan_words = (uint32_t)pw.w.size();
  snap_sections(P, policy, H.n_plan_words, n_faults, n_pools, r, mailbox_records, H.section_bytes);
  H.total_bytes = H.header_bytes;
  for (uint32_t s = 0; s < SNAP_NSEC; s++) H.total_bytes += H.section_bytes[s];
  return H;
}

// byte offset of section s in the blob
inline uint64_t snap_offset(const SnapHeader& H, uint32_t s) {
  uint64_t o = H.header_bytes;
  for (uint32_t k = 0; k < s; k++) o += H.section_bytes[k];
  return o;
}

// What can be checked of a blob without a handle: the header is whole, magic, version, and the
// sizes add up to `bytes` and agree with the header's own counts.  *H: a copy (buf may be unaligned).
inline int snap_parse(const void* buf, uint64_t bytes, SnapHeader* H) {
  if (!buf) return fail(PAXISIM_EINVAL, "null argument");
  if (bytes < sizeof(SnapHeader))
    return fail(PAXISIM_EINVAL, "snapshot truncated: %llu bytes, the header alone is %u", (unsigned long long)bytes,
                (unsigned)sizeof(SnapHeader));
  memcpy(H, buf, sizeof *H);
  if (memcmp(H->magic, SNAP_MAGIC, 8)) return fail(PAXISIM_EINVAL, "not a snapshot: bad magic");
  if (H->version != PAXISIM_SNAPSHOT_VERSION)
    return fail(PAXISIM_EINVAL, "snapshot version %u, this library reads version %u", H->version, PAXISIM_SNAPSHOT_VERSION);
  if (H->header_bytes != PAXISIM_SNAPSHOT_HEADER)
    return fail(PAXISIM_EINVAL, "snapshot header_bytes %u, expected %u", H->header_bytes, PAXISIM_SNAPSHOT_HEADER);
  if (H->build_id[sizeof H->build_id - 1]) return fail(PAXISIM_EINVAL, "snapshot build id is not terminated");
  uint64_t sum = H->header_bytes;
  for (uint32_t s = 0; s < SNAP_NSEC; s++) {
    if (H->section_bytes[s] > ~0ull - sum)
      return fail(PAXISIM_EINVAL, "snapshot section %s: size overflows", snap_section_names()[s]);
    sum += H->section_bytes[s];
  }
  if (sum != H->total_bytes)
    return fail(PAXISIM_EINVAL, "snapshot sections add up to %llu bytes, the header says %llu", (unsigned long long)sum,
                (unsigned long long)H->total_bytes);
  if (bytes < H->total_bytes)
    return fail(PAXISIM_EINVAL, "snapshot truncated: %llu bytes of %llu", (unsigned long long)bytes,
                (unsigned long long)H->total_bytes);
  if (bytes != H->total_bytes)
    return fail(PAXISIM_EINVAL, "snapshot sections add up to %llu bytes, %llu were given", (unsigned long long)sum,
                (unsigned long long)bytes);
  if (H->section_bytes[PAXISIM_SNAP_MAILBOX] / 16u != H->mailbox_records || H->section_bytes[PAXISIM_SNAP_MAILBOX] % 16u)
    return fail(PAXISIM_EINVAL, "snapshot section mailbox: %llu bytes for %llu records",
                (unsigned long long)H->section_bytes[PAXISIM_SNAP_MAILBOX], (unsigned long long)H->mailbox_records);
  if (H->section_bytes[PAXISIM_SNAP_PLAN] != 8ull * H->n_plan_words)
    return fail(PAXISIM_EINVAL, "snapshot section plan: %llu bytes for %u words",
                (unsigned long long)H->section_bytes[PAXISIM_SNAP_PLAN], H->n_plan_words);
  if (H->n_faults > PAXISIM_MAX_FAULTS || H->section_bytes[PAXISIM_SNAP_FAULTS] != (uint64_t)sizeof(DevFault) * H->n_faults)
    return fail(PAXISIM_EINVAL, "snapshot section faults: %llu bytes for %u faults",
                (unsigned long long)H->section_bytes[PAXISIM_SNAP_FAULTS], H->n_faults);
  if (H->n_pools < 1 || H->n_pools > MAX_POOLS || H->section_bytes[PAXISIM_SNAP_POOLS] != (uint64_t)SNAP_POOL_BYTES * H->n_pools)
    return fail(PAXISIM_EINVAL, "snapshot section pools: %llu bytes for %u pools",
                (unsigned long long)H->section_bytes[PAXISIM_SNAP_POOLS], H->n_pools);
  const uint32_t rec = (H->lat_bins ? PAXISIM_SNAP_HAS_LAT : 0u) | (H->ch_cap ? PAXISIM_SNAP_HAS_CHIST : 0u) |
                       (H->mv_cap ? PAXISIM_SNAP_HAS_MV : 0u) | (H->tr_cap ? PAXISIM_SNAP_HAS_TRACE : 0u);
  if (rec != H->recorders) return fail(PAXISIM_EINVAL, "snapshot recorders word %u does not match its sizes (%u)", H->recorders, rec);
  return 0;
}

inline int snap_info(const void* buf, uint64_t bytes, struct paxisim_snapshot_info* out) {
  if (!out) return fail(PAXISIM_EINVAL, "null argument");
  SnapHeader H;
  if (const int rc = snap_parse(buf, bytes, &H)) return rc;
  memset(out, 0, sizeof *out);
  out->version = H.version;
  out->protocol = H.protocol;
  out->n_replicas = H.n_replicas;
  out->step = H.step;
  out->clusters = H.clusters;
  out->cluster_base = H.cluster_base;
  out->mailbox_records = H.mailbox_records;
  out->total_bytes = H.total_bytes;
  out->plan_hash = H.plan_hash;
  out->recorders = H.recorders;
  out->n_faults = H.n_faults;
  for (uint32_t s = 0; s < SNAP_NSEC; s++) out->section_bytes[s] = H.section_bytes[s];
  memcpy(out->build_id, H.build_id, sizeof out->build_id);
  return 0;
}

// Everything paxisim_restore checks before its first device write, but the trace's row table
// (compared by the caller, which holds it): the blob against the library's build id and the
// handle's plan words, recorders and expected section sizes.  *trace_carried: the blob's trace rows
// go into the handle (both have the recorder), else the handle's rows are emptied.
inline int snap_check_restore(const void* buf, uint64_t bytes, const char* build_id, const PlanWords& pw, const Params& P,
                              uint32_t policy, uint32_t n_pools, const SnapRecorders& r, SnapHeader* H, bool* trace_carried) {
  if (const int rc = snap_parse(buf, bytes, H)) return rc;
  if (strncmp(H->build_id, build_id, sizeof H->build_id - 1))
    return fail(PAXISIM_EINVAL, "snapshot was written by build %s, this library is build %s (the image layout belongs to "
                "the build)", H->build_id, build_id);
  if (H->n_plan_words != pw.w.size())
    return fail(PAXISIM_EINVAL, "snapshot plan differs: %u plan words, the handle has %zu", H->n_plan_words, pw.w.size());
  const uint8_t* pb = static_cast<const uint8_t*>(buf) + snap_offset(*H, PAXISIM_SNAP_PLAN);
  for (size_t i = 0; i < pw.w.size(); i++) {
    uint64_t v;
    memcpy(&v, pb + 8 * i, 8);
    if (v != pw.w[i])
      return fail(PAXISIM_EINVAL, "snapshot plan differs: %s (snapshot %llu, handle %llu)", pw.names[i],
                  (unsigned long long)v, (unsigned long long)pw.w[i]);
  }
  if (H->plan_hash != snap_hash_words(pw.w)) return fail(PAXISIM_EINVAL, "snapshot plan differs: plan_hash");
  if (H->lat_bins != r.lat_bins)
    return fail(PAXISIM_EINVAL, "snapshot recorders differ: latency bins (snapshot %u, handle %u)", H->lat_bins, r.lat_bins);
  if (H->ch_cap != r.ch_cap)
    return fail(PAXISIM_EINVAL, "snapshot recorders differ: client history ops_per_worker (snapshot %u, handle %u)",
                H->ch_cap, r.ch_cap);
  if (H->mv_cap != r.mv_cap)
    return fail(PAXISIM_EINVAL, "snapshot recorders differ: multiversion versions_per_key (snapshot %u, handle %u)",
                H->mv_cap, r.mv_cap);
  SnapRecorders rb = r;   // the sizes the blob must have: the handle's, with the blob's own trace
  if (H->tr_cap) {
    if (!r.tr_cap) return fail(PAXISIM_EINVAL, "snapshot recorders differ: the snapshot carries a trace, the handle has none");
    if (H->tr_cap != r.tr_cap || H->tr_from != r.tr_from || H->tr_to != r.tr_to || H->tr_rows != r.tr_rows)
      return fail(PAXISIM_EINVAL, "snapshot recorders differ: trace (snapshot %u rows x %u records, steps [%u, %u); handle %u "
                  "x %u, [%u, %u))", H->tr_rows, H->tr_cap, H->tr_from, H->tr_to, r.tr_rows, r.tr_cap, r.tr_from, r.tr_to);
  } else {
    rb.tr_cap = rb.tr_from = rb.tr_to = rb.tr_rows = 0;
  }
  *trace_carried = H->tr_cap != 0;
  if (H->n_pools != n_pools)
    return fail(PAXISIM_EINVAL, "snapshot plan differs: pools (snapshot %u, handle %u)", H->n_pools, n_pools);
  uint64_t want[SNAP_NSEC];
  snap_sections(P, policy, H->n_plan_words, H->n_faults, n_pools, rb, H->mailbox_records, want);
  for (uint32_t s = 0; s < SNAP_NSEC; s++)
    if (want[s] != H->section_bytes[s])
      return fail(PAXISIM_EINVAL, "snapshot section %s is %llu bytes, the handle's is %llu", snap_section_names()[s],
                  (unsigned long long)H->section_bytes[s], (unsigned long long)want[s]);
  if (H->mailbox_records > (uint64_t)(P.C / LANES) * P.rec_per_block)
    return fail(PAXISIM_EINVAL, "snapshot carries %llu mailbox records, the handle holds %llu at most",
                (unsigned long long)H->mailbox_records, (unsigned long long)((P.C / LANES) * P.rec_per_block));
  return 0;
}

}  // namespace pxs
