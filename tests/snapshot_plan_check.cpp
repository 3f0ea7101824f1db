// Stand-alone check of paxi_amd/csrc/snapshot_plan.h (built and run by tests/test_snapshot_plan.py
// with the HIP compiler in host-only mode and the address and undefined-behaviour sanitizers; no
// GPU).  Over a grid of shapes - every protocol, N 1..16, D 2..16, M over 1..64, recorders on and
// off; what check_config refuses is counted and skipped - it writes a header and parses it back,
// compares every section size and offset with carve_arena's and the recorders' own arithmetic, and
// on whole blobs exercises every refusal: each truncation point, bad magic, bad version, every
// section size off by one, a foreign build id, every fingerprint word changed alone, every
// recorder mismatch.  The list of the recorders' device buffers is checked against the section sizes.
#include <cinttypes>
#include <string>
#include <type_traits>
#include <vector>

#include "snapshot_plan.h"

using namespace pxs;

static int g_fail = 0;
static long g_checks = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    g_checks++;                               \
    if (!(cond)) {                            \
      std::printf("FAIL %s: ", #cond);        \
      std::printf(__VA_ARGS__);               \
      std::printf("\n");                      \
      if (++g_fail > 40) std::exit(1);        \
    }                                         \
  } while (0)

static const char* BUILD = "0123456789abcdef";

struct Shape {
  paxisim_config cfg;
  paxisim_workload wl;
  paxisim_fault_process fp;
  Params P;
  PlanExtra x;
  uint32_t variant;
  bool ok;
};

static Shape shape(uint32_t protocol, uint32_t N, uint32_t max_delay, uint32_t M, uint64_t clusters, uint64_t seed = 7) {
  Shape s;
  memset(&s.cfg, 0, sizeof s.cfg);
  memset(&s.wl, 0, sizeof s.wl);
  memset(&s.fp, 0, sizeof s.fp);
  s.variant = protocol;
  s.cfg.protocol = protocol == PAXISIM_M2PAXOS || protocol == PAXISIM_KPAXOS ? (uint32_t)PAXISIM_WPAXOS : protocol;
  s.cfg.n_zones = N % 3 == 0 ? 3 : 1;
  for (uint32_t z = 0; z < s.cfg.n_zones; z++) s.cfg.npz[z] = N / s.cfg.n_zones;
  s.cfg.window = 8;
  s.cfg.mbox_cap = M;
  s.cfg.max_delay = max_delay;
  s.cfg.keys = 4;
  s.cfg.clusters = clusters;
  s.cfg.seed = seed;
  s.cfg.history = protocol == PAXISIM_ABD ? 8 : 0;
  s.cfg.kv = 1;
  s.cfg.policy_threshold = 2;
  s.cfg.policy_alpha = 0.5;
  s.wl.outstanding = M < 2 ? 1 : 2;
  s.wl.write_ppm = 500000;
  s.fp.slow_ppm = max_delay ? 1000 : 0;
  s.fp.slow_len = 5;
  s.fp.slow_min = max_delay ? 1 : 0;
  s.fp.slow_max = max_delay;
  Knobs kn;
  uint32_t n = 0, zone_of[PAXISIM_MAX_N], node_of[PAXISIM_MAX_N], S = 0;
  s.ok = check_config(&s.cfg, &s.wl, &s.fp, kn, &n) == 0;
  if (!s.ok) return s;
  fill_params(s.P, zone_of, node_of, S, &s.cfg, &s.wl, &s.fp, s.variant, n, kn);
  KernelFacts kf;
  kf.vgprs = 128;
  kf.max_threads = 1024;
  kf.serial = true;
  kf.has_pipe = true;
  s.ok = plan_lds(s.P, kn, kf) == 0;
  if (!s.ok) return s;
  Params Q = s.P;
  const ArenaSize sz = carve_arena(Q, s.cfg.policy, nullptr, false);
  const Schedule sc = plan_schedule(s.P, kn, kf, S, true);
  s.P.compact = sc.compact;
  s.x.arena_zero = sz.zero_bytes;
  s.x.arena_total = sz.total;
  s.x.serial = true;
  s.x.chunk = S;
  s.x.pipe_max = sc.pipe_max;
  s.x.cmp_every = sc.cmp_every;
  s.x.late_until = sc.late_until;
  return s;
}

static PlanWords words(const Shape& s) {
  paxisim_config cfg = s.cfg;
  cfg.protocol = s.variant;
  return plan_words(cfg, s.wl, s.fp, s.P, s.x);
}

// a whole blob of the shape: the header, the plan words, zeroed sections with the counts given
static std::vector<uint8_t> blob_of(const Shape& s, const SnapRecorders& r, uint32_t t, uint32_t n_faults, uint64_t records,
                                    SnapHeader* Hout = nullptr) {
  const PlanWords pw = words(s);
  const SnapHeader H = snap_header(BUILD, pw, s.variant, s.P, s.cfg.policy, t, n_faults, 1, r, records);
  std::vector<uint8_t> b(H.total_bytes, 0);
  memcpy(b.data(), &H, sizeof H);
  memcpy(b.data() + snap_offset(H, PAXISIM_SNAP_PLAN), pw.w.data(), pw.w.size() * 8);
  if (Hout) *Hout = H;
  return b;
}

static bool refused(int rc, const char* what) { return rc == PAXISIM_EINVAL && strstr(g_err, what) != nullptr; }

static void grid() {
  const uint32_t protos[] = {PAXISIM_PAXOS, PAXISIM_WPAXOS, PAXISIM_M2PAXOS, PAXISIM_KPAXOS, PAXISIM_ABD, PAXISIM_EPAXOS};
  const uint32_t Ms[] = {1, 2, 3, 8, 31, 32, 63, 64};
  long shapes = 0, skipped = 0;
  for (const uint32_t pr : protos)
    for (uint32_t N = 1; N <= 16; N++)
      for (uint32_t D = 2; D <= 16; D++)
        for (const uint32_t M : Ms)
          for (uint32_t rec = 0; rec < 2; rec++) {
            Shape s = shape(pr, N, D - 2, M, 70 + N);
            if (!s.ok) {
              skipped++;
              continue;
            }
            shapes++;
            SnapRecorders r;
            if (rec) {
              r.lat_bins = 64; r.ch_cap = 4; r.mv_cap = 3; r.tr_cap = 16; r.tr_from = 5; r.tr_to = 90; r.tr_rows = 6;
            }
            const Params& P = s.P;
            const uint64_t records = (uint64_t)N * D * M + rec;
            const PlanWords pw = words(s);
            const SnapHeader H = snap_header(BUILD, pw, s.variant, P, s.cfg.policy, 37, 2, 1, r, records);
            // the parser reads the header alone: give it the header and the size the header claims
            SnapHeader G;
            CHECK(snap_parse(&H, H.total_bytes, &G) == 0, "%s", g_err);
            CHECK(!memcmp(&G, &H, sizeof H), "round trip");
            struct paxisim_snapshot_info inf;
            CHECK(snap_info(&H, H.total_bytes, &inf) == 0, "%s", g_err);
            CHECK(inf.protocol == pr && inf.n_replicas == N && inf.clusters == 70 + N && inf.step == 37 &&
                  inf.mailbox_records == records && inf.total_bytes == H.total_bytes && inf.n_faults == 2 &&
                  !strcmp(inf.build_id, BUILD) && inf.recorders == (rec ? 15u : 0u), "info of proto %u N %u", pr, N);
            // sections against carve_arena and the recorders' own arithmetic
            Params Q = P;
            char* const base = reinterpret_cast<char*>(uintptr_t(1) << 30);
            const ArenaSize sz = carve_arena(Q, s.cfg.policy, base, true);
            const uint64_t C = P.C, WK = P.WK;
            CHECK(H.section_bytes[PAXISIM_SNAP_ARENA] == sz.zero_bytes, "arena");
            CHECK((uint64_t)(reinterpret_cast<char*>(Q.rec) - base) == sz.zero_bytes, "rec starts where the arena section ends");
            CHECK((uint64_t)(reinterpret_cast<char*>(Q.image) - base) + (C / 64) * P.img.bytes <= sz.zero_bytes, "image inside");
            CHECK(sz.total - sz.zero_bytes >= (C / 64) * (uint64_t)P.rec_per_block * 16, "rec region");
            CHECK(P.rec_per_block == D * N * (N + 1) * M * 64, "rec_per_block");
            CHECK(H.section_bytes[PAXISIM_SNAP_MAILBOX] == 16 * records, "mailbox");
            CHECK(H.section_bytes[PAXISIM_SNAP_PLAN] == 8 * pw.w.size() && pw.w.size() == pw.names.size(), "plan");
            CHECK(H.section_bytes[PAXISIM_SNAP_FAULTS] == 2 * 48 && H.section_bytes[PAXISIM_SNAP_POOLS] == 48, "faults, pools");
            CHECK(H.section_bytes[PAXISIM_SNAP_LAT] == (rec ? 4 * WK * C + 8 * 8 * WK * (64 + 4) : 0), "lat");
            CHECK(H.section_bytes[PAXISIM_SNAP_CHIST] == (rec ? 4 * WK * C + 16 * WK * C * 4 : 0), "chist");
            CHECK(H.section_bytes[PAXISIM_SNAP_MV] == (rec ? 4 * (uint64_t)P.keys * N * C * (1 + 3) : 0), "mv");
            CHECK(H.section_bytes[PAXISIM_SNAP_TRACE] == (rec ? 4 * C + 4 * 6 * N + 32 * 6 * (uint64_t)N * 16 : 0), "trace");
            uint64_t off = PAXISIM_SNAPSHOT_HEADER;
            for (uint32_t k = 0; k < SNAP_NSEC; k++) {
              CHECK(snap_offset(H, k) == off, "offset of section %u", k);
              off += H.section_bytes[k];
            }
            CHECK(off == H.total_bytes, "total");
            // the handle it came from takes it back; header-level refusals
            bool carried = false;
            std::vector<uint8_t> hp(sizeof H + pw.w.size() * 8);
            memcpy(hp.data(), &H, sizeof H);
            memcpy(hp.data() + sizeof H, pw.w.data(), pw.w.size() * 8);
            CHECK(snap_check_restore(hp.data(), H.total_bytes, BUILD, pw, P, s.cfg.policy, 1, r, &G, &carried) == 0, "%s", g_err);
            CHECK(carried == (rec != 0), "trace carried");
            CHECK(refused(snap_parse(&H, H.total_bytes - 1, &G), "truncated"), "%s", g_err);
            CHECK(refused(snap_parse(&H, H.total_bytes + 1, &G), "add up"), "%s", g_err);
            CHECK(refused(snap_check_restore(hp.data(), H.total_bytes, "fedcba9876543210", pw, P, s.cfg.policy, 1, r, &G, &carried),
                          "written by build"), "%s", g_err);
          }
  std::printf("grid: %ld shapes, %ld refused by the create plan\n", shapes, skipped);
  CHECK(shapes > 5000, "the grid is not vacuous");
}

static void refusals() {
  Shape s = shape(PAXISIM_PAXOS, 5, 4, 32, 130);
  CHECK(s.ok, "shape");
  SnapRecorders r;
  r.lat_bins = 64; r.ch_cap = 4; r.mv_cap = 3;
  const PlanWords pw = words(s);
  SnapHeader H, G;
  const std::vector<uint8_t> blob = blob_of(s, r, 37, 1, 0, &H);
  bool carried = false;
  auto restore = [&](const std::vector<uint8_t>& b, const SnapRecorders& rr, const PlanWords& w = PlanWords()) {
    return snap_check_restore(b.data(), b.size(), BUILD, w.w.empty() ? pw : w, s.P, s.cfg.policy, 1, rr, &G, &carried);
  };
  CHECK(restore(blob, r) == 0, "%s", g_err);
  CHECK(snap_parse(nullptr, 10, &G) == PAXISIM_EINVAL, "null");
  // every truncation point
  for (uint64_t n = 0; n < blob.size(); n++) {
    std::vector<uint8_t> cut(blob.begin(), blob.begin() + n);   // its own allocation: a read past n is caught
    const int rc = snap_parse(n ? cut.data() : blob.data(), n, &G);
    if (!refused(rc, "truncated")) CHECK(false, "cut at %" PRIu64 ": %d %s", n, rc, g_err);
    if (n > 4096 && n + 4096 < blob.size()) n += 997;           // dense at both ends, strided in the zeroed middle
  }
  for (int i = 0; i < 8; i++) {
    std::vector<uint8_t> b = blob;
    b[i] ^= 0x20;
    CHECK(refused(restore(b, r), "bad magic"), "%s", g_err);
  }
  for (const uint32_t v : {0u, 2u, 0xFFFFFFFFu}) {
    std::vector<uint8_t> b = blob;
    memcpy(b.data() + 8, &v, 4);
    CHECK(refused(restore(b, r), "version"), "%s", g_err);
  }
  {
    std::vector<uint8_t> b = blob;
    const uint32_t v = 264;
    memcpy(b.data() + 12, &v, 4);
    CHECK(refused(restore(b, r), "header_bytes"), "%s", g_err);
  }
  for (uint32_t k = 0; k < SNAP_NSEC; k++)
    for (const int d : {-1, 1}) {
      if (H.section_bytes[k] == 0 && d < 0) continue;
      std::vector<uint8_t> b = blob;
      const uint64_t v = H.section_bytes[k] + d;
      memcpy(b.data() + 104 + 8 * k, &v, 8);
      CHECK(refused(restore(b, r), "add up"), "section %u %+d: %s", k, d, g_err);
      // ... and with the total moved along, so that the sums agree: the section's own check
      const uint64_t tot = H.total_bytes + d;
      memcpy(b.data() + 56, &tot, 8);
      b.resize(tot);
      CHECK(restore(b, r) == PAXISIM_EINVAL, "section %u %+d with the total adjusted: %s", k, d, g_err);
    }
  {
    std::vector<uint8_t> b = blob;
    b[16] ^= 1;
    CHECK(refused(restore(b, r), "written by build"), "%s", g_err);
  }
  // every fingerprint word changed alone: named
  for (size_t i = 0; i < pw.w.size(); i++) {
    std::vector<uint8_t> b = blob;
    b[snap_offset(H, PAXISIM_SNAP_PLAN) + 8 * i] ^= 1;
    const std::string want = std::string("snapshot plan differs: ") + pw.names[i] + " (";
    CHECK(refused(restore(b, r), want.c_str()), "word %zu %s: %s", i, pw.names[i], g_err);
  }
  // every input field changed alone moves exactly its word (tables: their hash)
#define MUT(stmt, name)                                                              \
  {                                                                                  \
    Shape m = s;                                                                     \
    stmt;                                                                            \
    const PlanWords mw = words(m);                                                   \
    size_t diff = 0, at = 0;                                                         \
    for (size_t i = 0; i < pw.w.size(); i++)                                         \
      if (mw.w[i] != pw.w[i]) { diff++; at = i; }                                    \
    CHECK(diff == 1 && !strcmp(pw.names[at], name), "%s moved %zu words", name, diff); \
    CHECK(refused(restore(blob, r, mw), name), "%s: %s", name, g_err);               \
  }
  MUT(m.cfg.seed++, "config.seed")
  MUT(m.cfg.clusters++, "config.clusters")
  MUT(m.cfg.cluster_base = 64, "config.cluster_base")
  MUT(m.cfg.window = 16, "config.window")
  MUT(m.cfg.npz[3] = 1, "config.npz")
  MUT(m.cfg.thrifty = 1, "config.thrifty")
  MUT(m.cfg.policy_alpha = 0.25, "config.policy_alpha")
  MUT(m.wl.write_ppm++, "workload.write_ppm")
  MUT(m.wl.target[1] = 3, "workload.target")
  MUT(m.wl.key_cdf[5] = 9, "workload.key_cdf")
  MUT(m.wl.start_step[1] = 9, "workload.start_step")
  MUT(m.fp.drop_ppm = 5, "fault_process.drop_ppm")
  MUT(m.fp.slow_len++, "fault_process.slow_len")
  MUT(m.P.G = 2, "plan.G")
  MUT(m.P.C += 64, "plan.C")
  MUT(m.P.rec_per_block++, "plan.rec_per_block")
  MUT(m.P.img.off_cnt += 4, "plan.img.off_cnt")
  MUT(m.P.packed ^= 1, "plan.packed")
  MUT(m.P.wcoloc ^= 1, "plan.wcoloc")
  MUT(m.P.wlds ^= 1, "plan.wlds")
  MUT(m.x.arena_zero += 256, "plan.arena_zero")
  MUT(m.x.arena_total += 256, "plan.arena_total")
  MUT(m.x.serial = false, "plan.serial")
  MUT(m.x.staged = true, "plan.staged")
  MUT(m.x.npools = 2, "plan.npools")
  MUT(m.x.pool1_base = 512, "plan.pool1_base")
  MUT(m.x.pipe_max++, "plan.pipe_max")
  MUT(m.x.cmp_every++, "plan.cmp_every")
  {
    const uint32_t tab[PAXISIM_MAX_KEYS] = {1, 2, 3};
    Shape m = s;
    m.P.move_tables = 1;
    m.x.move_cdf = tab;
    CHECK(refused(restore(blob, r, words(m)), "workload.move_cdf"), "%s", g_err);
  }
  // recorders
  SnapRecorders q = r;
  q.lat_bins = 128;
  CHECK(refused(restore(blob, q), "latency bins (snapshot 64, handle 128)"), "%s", g_err);
  q = r; q.lat_bins = 0; q.ch_cap = 0; q.mv_cap = 0;
  CHECK(refused(restore(blob, q), "latency bins (snapshot 64, handle 0)"), "%s", g_err);
  q = r; q.ch_cap = 8;
  CHECK(refused(restore(blob, q), "client history ops_per_worker"), "%s", g_err);
  q = r; q.mv_cap = 0;
  CHECK(refused(restore(blob, q), "multiversion versions_per_key"), "%s", g_err);
  q = r; q.tr_cap = 16; q.tr_to = 50; q.tr_rows = 2;          // the handle alone traces: rewind and trace
  CHECK(restore(blob, q) == 0 && !carried, "%s", g_err);
  const std::vector<uint8_t> traced = blob_of(s, q, 37, 1, 0);
  CHECK(restore(traced, q) == 0 && carried, "%s", g_err);
  CHECK(refused(restore(traced, r), "the snapshot carries a trace, the handle has none"), "%s", g_err);
  SnapRecorders q2 = q;
  q2.tr_to = 60;
  CHECK(refused(restore(traced, q2), "snapshot recorders differ: trace"), "%s", g_err);
  q2 = q; q2.tr_rows = 3;
  CHECK(refused(restore(traced, q2), "snapshot recorders differ: trace"), "%s", g_err);
  // pools and the record bound
  CHECK(refused(snap_check_restore(blob.data(), blob.size(), BUILD, pw, s.P, s.cfg.policy, 2, r, &G, &carried), "pools"), "%s", g_err);
  {
    const uint64_t cap = (s.P.C / 64) * s.P.rec_per_block;
    const PlanWords w = words(s);
    SnapHeader B = snap_header(BUILD, w, s.variant, s.P, s.cfg.policy, 1, 0, 1, SnapRecorders(), cap + 1);
    std::vector<uint8_t> hp(sizeof B + w.w.size() * 8);
    memcpy(hp.data(), &B, sizeof B);
    memcpy(hp.data() + sizeof B, w.w.data(), w.w.size() * 8);
    CHECK(refused(snap_check_restore(hp.data(), B.total_bytes, BUILD, w, s.P, s.cfg.policy, 1, SnapRecorders(), &G, &carried),
                  "at most"), "%s", g_err);
  }
}

// snap_recorder_bufs, the list snapshot / restore / fork / destroy walk, against snap_sections: every
// recorder on and off, alone and together, at two shapes.  The pointers are made up; nothing reads them.
static void recorder_table() {
  for (const uint32_t N : {3u, 9u}) {
    const Shape s = shape(PAXISIM_PAXOS, N, 4, 16, 130);
    CHECK(s.ok, "shape N %u", N);
    for (uint32_t on = 0; on < 16; on++) {
      Params P = s.P;
      const uint32_t tr_rows = 2;
      uintptr_t next = 0x1000;
      auto fake = [&](auto*& p) { p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(next += 0x1000); };
      if (on & 1) { P.lat_bins = 16; fake(P.lat_stamp); fake(P.lat_acc); }
      if (on & 2) { P.ch_cap = 8; fake(P.ch_cnt); fake(P.ch_ops); }
      if (on & 4) { P.mv_cap = 4; fake(P.mv_cnt); fake(P.mv_val); }
      if (on & 8) { P.tr_cap = 32; P.tr_from = 0; P.tr_to = 96; fake(P.tr_cnt); fake(P.tr_rec); }
      uint64_t sec[SNAP_NSEC];
      snap_sections(P, s.cfg.policy, 90, 0, 1, snap_recorders(P, tr_rows), 0, sec);
      const auto bufs = snap_recorder_bufs(P, tr_rows);
      const void* const want[SNAP_NBUF] = {P.lat_stamp, P.lat_acc, P.ch_cnt, P.ch_ops, P.mv_cnt, P.mv_val, P.tr_cnt, P.tr_rec};
      const uint32_t section[SNAP_NBUF] = {PAXISIM_SNAP_LAT, PAXISIM_SNAP_LAT, PAXISIM_SNAP_CHIST, PAXISIM_SNAP_CHIST,
                                           PAXISIM_SNAP_MV, PAXISIM_SNAP_MV, PAXISIM_SNAP_TRACE, PAXISIM_SNAP_TRACE};
      uint64_t sum[SNAP_NSEC] = {0};
      for (uint32_t i = 0; i < SNAP_NBUF; i++) {
        const SnapBuf& b = bufs[i];
        const bool present = (on >> (i / 2)) & 1u;
        const uint64_t lead = b.section == PAXISIM_SNAP_TRACE ? snap_tr_row_bytes(P) : 0;   // the host-side tr_row table
        CHECK(b.section == section[i] && b.ptr == want[i], "N %u on %u: entry %u is section %u", N, on, i, b.section);
        CHECK(b.present == present && (b.ptr != nullptr) == present && (b.bytes != 0) == present,
              "N %u on %u: entry %u present %d, %zu bytes", N, on, i, (int)b.present, b.bytes);
        CHECK(b.offset == lead + sum[b.section], "N %u on %u: entry %u at offset %zu", N, on, i, b.offset);
        sum[b.section] += b.bytes;
      }
      for (const uint32_t k : {(uint32_t)PAXISIM_SNAP_LAT, (uint32_t)PAXISIM_SNAP_CHIST, (uint32_t)PAXISIM_SNAP_MV})
        CHECK(sum[k] == sec[k], "N %u on %u: section %u is %" PRIu64 " bytes, the table's buffers %" PRIu64, N, on, k, sec[k], sum[k]);
      const uint64_t lead = (on & 8) ? snap_tr_row_bytes(P) : 0;
      CHECK(sum[PAXISIM_SNAP_TRACE] == sec[PAXISIM_SNAP_TRACE] - lead,
            "N %u on %u: trace section %" PRIu64 " bytes, tr_row %" PRIu64 ", the table's buffers %" PRIu64, N, on,
            sec[PAXISIM_SNAP_TRACE], lead, sum[PAXISIM_SNAP_TRACE]);
    }
  }
}

int main() {
  grid();
  refusals();
  recorder_table();
  if (g_fail) {
    std::printf("%d failures in %ld checks\n", g_fail, g_checks);
    return 1;
  }
  std::printf("snapshot_plan OK: %ld checks\n", g_checks);
  return 0;
}
