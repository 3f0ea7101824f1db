// Stand-alone check of paxi_amd/csrc/create_plan.h (built and run by tests/test_create_plan.py with
// the HIP compiler in host-only mode and the address and undefined-behaviour sanitizers; no GPU).
//   create_plan_check <tests/golden/create_plan.txt>
// For every case of the fixture - recorded from the library before paxisim_create was split - it runs
// the plan on the recorded inputs, knobs and kernel facts and compares every recorded output, or
// the refusal's code and message.  It then checks invariants of the plan on those cases and on a
// denser grid of shapes with made-up kernel facts.
#include <algorithm>
#include <cinttypes>
#include <map>
#include <string>
#include <vector>

#include "create_plan.h"

using namespace pxs;

static int g_fail = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      std::printf("FAIL %s: ", #cond);        \
      std::printf(__VA_ARGS__);               \
      std::printf("\n");                      \
      if (++g_fail > 40) std::exit(1);        \
    }                                         \
  } while (0)

// the fixture's field lists (tools/variants/create_plan_dump.patch writes the same ones)
#define DUMP_CFG(S, A) S(protocol) S(n_zones) A(npz) S(q1) S(q2) S(fz) S(thrifty) S(ephemeral_leader) \
  S(reply_when_commit) S(adaptive) S(policy_threshold) S(window) S(mbox_cap) S(max_delay) S(keys) \
  S(steps_per_launch) S(history) S(clusters) S(cluster_base) S(seed) S(policy) S(policy_interval) S(agree_ring) S(kv)
#define DUMP_WL(S, A) S(outstanding) S(max_requests) S(write_ppm) S(locality_ppm) A(target) S(distribution) \
  S(conflicts) A(key_cdf) A(start_step) S(key_min) S(key_space) S(key_tail) S(move_every) S(move_tables) S(move_loop)
#define DUMP_FP(S, A) S(drop_ppm) S(drop_len) S(slow_ppm) S(slow_len) S(slow_min) S(slow_max)
#define DUMP_P(S, A) S(protocol) S(N) S(Z) S(W) S(M) S(D) S(NS) S(WK) S(max_requests) S(keys) S(write_ppm) \
  S(locality_ppm) S(H) S(OW) S(dist) S(conflicts) A(key_cdf) S(NK) S(NI) S(adaptive) S(policy_thr) S(policy) \
  S(policy_interval) S(wk_magic) S(C) S(clusters) S(cluster_base) S(seed) S(q1) S(q2) S(fz) S(thrifty) \
  S(ephemeral) S(rwc) S(max_delay) S(nfaults) S(drop_ppm) S(drop_len) S(slow_ppm) S(slow_len) S(slow_min) \
  S(slow_max) A(npz) A(zmask) A(zone_of) A(target) A(start_step) S(late_workers) A(wzone) A(wnk) A(wnk_magic) \
  S(keys_magic) S(img.off_a) S(img.off_b) S(img.off_c) S(img.off_wcur) S(img.off_wiss) S(img.off_poison) \
  S(img.off_cnt) S(img.bytes) S(J) S(off_stage) S(lds_bytes) S(lds_tail) S(off_wscr) S(G) S(rec_per_block) \
  S(wst_str) S(wlog_str) S(wlds) S(wcoloc) S(AR) S(off_agn) S(packed) S(compact) S(phase_sort) S(phase_period) \
  S(ph_rel) S(variant) A(zfirst) S(key_min) S(kspace) S(kspace_magic) S(conflict_key) S(key_tail) S(move_every) \
  S(move_tables) S(move_loop) S(kv) S(lat_bins) S(ch_cap) S(mv_cap) S(tr_cap) S(tr_from) S(tr_to)
#define DUMP_PTR(O) O(ballot) O(slot) O(execute) O(meta) O(flags) O(npend) O(nfwd) O(digest) O(kc) O(pend) O(fwd) \
  O(link_drop) O(link_slow) O(ck_e) O(ck_d) O(gst) O(wst) O(wdig) O(wlog) O(wpend) O(wpx) O(stats) O(agr) O(agq) \
  O(reqx) O(plog) O(hist) O(image) O(rec) O(slot_of) O(cl_of) O(frz) O(qf) O(phase) O(ep_inst) O(ep_sce) O(ep_cf) \
  O(ep_max) O(kv_val) O(kv_ver) O(wrep)
static const char* const KNOBS[] = {
    "PAXISIM_SERIAL", "PAXISIM_WLDS", "PAXISIM_WCOLOC", "PAXISIM_GROUPS", "PAXISIM_STAGE", "PAXISIM_COMPACT",
    "PAXISIM_PHASE_SORT", "PAXISIM_PHASE_PERIOD", "PAXISIM_PIPE", "PAXISIM_PIPE_SPIN", "PAXISIM_PIPE_SLOTS",
    "PAXISIM_COMPACT_EVERY", "PAXISIM_POOLS", "PAXISIM_ARENA_PAD_MB", "PAXISIM_ARENA_CONTIG"};

typedef std::map<std::string, std::string> Map;

static std::string num(unsigned long long v) { return std::to_string(v); }
static std::string real(double v) {
  char b[64];
  snprintf(b, sizeof b, "%.17g", v);
  return b;
}
template <typename T, size_t n>
static std::string list(const T (&a)[n]) {
  std::string s;
  for (size_t i = 0; i < n; i++) s += (i ? "," : "") + num(a[i]);
  return s;
}
template <typename T, size_t n>
static void parse_list(const std::string& v, T (&a)[n]) {
  size_t i = 0;
  for (const char* p = v.c_str(); *p && i < n; i++) {
    char* end;
    a[i] = (T)strtoull(p, &end, 10);
    p = *end == ',' ? end + 1 : end;
  }
}

struct Inputs {
  paxisim_config cfg;
  paxisim_workload wl;
  paxisim_fault_process fp;
  std::vector<uint32_t> move_cdf;
  KernelFacts kf;
  bool probe_ok = true;
  uint32_t resident_slots = 0;
};

static Inputs inputs_of(const Map& m) {
  Inputs in;
  memset(&in.cfg, 0, sizeof in.cfg);
  memset(&in.wl, 0, sizeof in.wl);
  memset(&in.fp, 0, sizeof in.fp);
  auto get = [&](const std::string& k) {
    auto it = m.find(k);
    return it == m.end() ? std::string("0") : it->second;
  };
#define IN_S(x) v.x = (decltype(v.x))strtoull(get(pre + #x).c_str(), nullptr, 10);
#define IN_A(x) parse_list(get(pre + #x), v.x);
  std::string pre = "in.cfg.";
  { paxisim_config& v = in.cfg; DUMP_CFG(IN_S, IN_A) v.policy_alpha = atof(get("in.cfg.policy_alpha").c_str()); }
  pre = "in.wl.";
  { paxisim_workload& v = in.wl; DUMP_WL(IN_S, IN_A) }
  pre = "in.fp.";
  { paxisim_fault_process& v = in.fp; DUMP_FP(IN_S, IN_A) }
  if (m.count("in.wl.move_cdf")) {
    in.move_cdf.resize((size_t)in.wl.move_tables * PAXISIM_MAX_KEYS);
    size_t i = 0;
    for (const char* p = m.at("in.wl.move_cdf").c_str(); *p && i < in.move_cdf.size(); i++) {
      char* end;
      in.move_cdf[i] = (uint32_t)strtoul(p, &end, 10);
      p = *end == ',' ? end + 1 : end;
    }
    in.wl.move_cdf = in.move_cdf.data();
  }
  in.kf.vgprs = atoi(get("fact.vgprs").c_str());
  in.kf.max_threads = atoi(get("fact.max_threads").c_str());
  in.kf.staged = atoi(get("fact.staged").c_str()) != 0;
  in.kf.serial = atoi(get("fact.serial").c_str()) != 0;
  in.kf.has_pipe = atoi(get("fact.has_pipe").c_str()) != 0;
  in.probe_ok = atoi(get("fact.probe_ok").c_str()) != 0;
  in.resident_slots = (uint32_t)atoi(get("fact.resident_slots").c_str());
  return in;
}

// What one run of the plan decides, in paxisim_create's order.
struct Plan {
  int rc = 0;
  Params P;
  uint32_t zone_of[PAXISIM_MAX_N] = {0}, node_of[PAXISIM_MAX_N] = {0};
  uint32_t S = 0;
  ArenaSize sized{0, 0}, bound{0, 0};
  Schedule sc{false, 0, 0, 0};
  uint32_t npools = 1, pool0_end = 0, pool1_base = 0, pool1_last_cmp = 0;
  bool config_ok = false;   // check_config passed
};
static char* const BASE = reinterpret_cast<char*>(uintptr_t(1) << 40);   // an arena nobody dereferences

static Plan run_plan(const Inputs& in, const Knobs& kn) {
  Plan pl;
  memset(&pl.P, 0, sizeof pl.P);
  paxisim_config cfg = in.cfg;
  const uint32_t variant = cfg.protocol;
  if (variant == PAXISIM_M2PAXOS || variant == PAXISIM_KPAXOS) cfg.protocol = PAXISIM_WPAXOS;
  uint32_t N = 0;
  if ((pl.rc = check_config(&cfg, &in.wl, &in.fp, kn, &N))) return pl;
  pl.config_ok = true;
  Params& P = pl.P;
  fill_params(P, pl.zone_of, pl.node_of, pl.S, &cfg, &in.wl, &in.fp, variant, N, kn);
  if ((pl.rc = plan_lds(P, kn, in.kf))) return pl;
  pl.sized = carve_arena(P, cfg.policy, nullptr, false);
  pl.bound = carve_arena(P, cfg.policy, BASE, true);
  pl.sc = plan_schedule(P, kn, in.kf, pl.S, in.probe_ok);
  P.compact = pl.sc.compact;
  pl.pool0_end = (uint32_t)P.C;
  if (kn.pools < 0) {
    pl.rc = fail(PAXISIM_EINVAL, "PAXISIM_POOLS must be 1 or 2");
    return pl;
  }
  const bool can = P.compact && pl.sc.pipe_max > 1;
  const uint32_t tiles = (uint32_t)(P.C / LANES);
  CHECK(pool_want(kn.pools, false, P.N, tiles, in.resident_slots) == 1, "pool_want without `can`");
  if (pool_want(kn.pools, can, P.N, tiles, in.resident_slots) > 1)
    if (const uint32_t split = pool_split_tile(tiles, cfg.clusters)) {
      pl.npools = 2;
      pl.pool0_end = pl.pool1_base = split * LANES;
      pl.pool1_last_cmp = pool_first_cmp(1, pl.S);
    }
  return pl;
}

static Map outputs_of(const Plan& pl) {
  Map o;
  if (pl.rc) {
    o["err.code"] = std::to_string(pl.rc);
    o["err.msg"] = g_err;
    return o;
  }
  const Params& v = pl.P;
#define OUT_S(x) o["out.P." #x] = num(v.x);
#define OUT_A(x) o["out.P." #x] = list(v.x);
#define OUT_O(x) o["out.P." #x] = v.x ? std::to_string((long long)((const char*)v.x - BASE)) : std::string("-1");
  DUMP_P(OUT_S, OUT_A)
  o["out.P.policy_alpha"] = real(v.policy_alpha);
  DUMP_PTR(OUT_O)
  o["out.zero_bytes"] = num(pl.bound.zero_bytes);
  o["out.total"] = num(pl.bound.total);
  o["out.S"] = num(pl.S);
  o["out.pipe_max"] = num(pl.sc.pipe_max);
  o["out.cmp_every"] = num(pl.sc.cmp_every);
  o["out.late_until"] = num(pl.sc.late_until);
  o["out.npools"] = num(pl.npools);
  o["out.pool0_end"] = num(pl.pool0_end);
  o["out.pool1_base"] = num(pl.pool1_base);
  o["out.pool1_last_cmp"] = num(pl.pool1_last_cmp);
  o["out.zone_of"] = list(pl.zone_of);
  o["out.node_of"] = list(pl.node_of);
  return o;
}

// Invariants of any accepted plan.  The region sizes restate the shapes in Params' comments
// (paxisim_dev.h), not the carve.
static void invariants(const char* name, const Plan& pl, uint32_t policy) {
  const Params& P = pl.P;
  CHECK(pl.sized.zero_bytes == pl.bound.zero_bytes && pl.sized.total == pl.bound.total,
        "%s: sizing pass (%zu, %zu) vs binding pass (%zu, %zu)", name, pl.sized.zero_bytes, pl.sized.total,
        pl.bound.zero_bytes, pl.bound.total);
  CHECK(P.lds_bytes % 16 == 0 && (uint64_t)P.G * P.lds_bytes <= LDS_MAX, "%s: G=%u lds_bytes=%u", name, P.G, P.lds_bytes);
  CHECK(P.G >= 1 && P.C % (64 * P.G) == 0 && P.C >= P.clusters && P.C < P.clusters + 64 * P.G, "%s: C=%" PRIu64 " G=%u clusters=%" PRIu64,
        name, P.C, P.G, P.clusters);
  const size_t C = P.C, N = P.N, NC = N * C, NIC = (size_t)P.NI * C, blocks = C / LANES;
  const bool wp = P.protocol == PAXISIM_WPAXOS, ep = P.protocol == PAXISIM_EPAXOS;
  const bool coloc = wp && !P.wlds && P.wcoloc;
  struct Reg {
    const char* name;
    const void* p;
    size_t bytes;
  };
  const Reg regs[] = {
      {"ballot..nfwd", P.ballot, NC * 7 * 4}, {"digest", P.digest, NC * 8}, {"kc", P.kc, C * 4},
      {"pend", P.pend, wp ? 0 : NC * PMAX * 4}, {"fwd", P.fwd, NC * FMAX * 4}, {"link_drop/slow", P.link_drop, NC * N * 2 * 4},
      {"ck_e", P.ck_e, NIC * CKR * 4}, {"ck_d", P.ck_d, NIC * CKR * 8}, {"gst", P.gst, NIC * GMAX * 16},
      {"stats", P.stats, NC * NSTAT * 4}, {"reqx", P.reqx, wp || P.packed ? 0 : NC * P.W * 4},
      {"plog", P.plog, P.packed ? NC * P.W * 16 : 0},
      {"wst", P.wst, coloc ? NIC * P.wst_str * 16 : wp && !P.wlds ? NIC * 32 : 0},
      {"wdig", P.wdig, wp && P.wlds ? NIC * 8 : 0}, {"wlog", P.wlog, wp && !coloc ? NIC * P.W * 16 : 0},
      {"wpend", P.wpend, wp ? NIC * PMAX * 4 : 0},
      {"wpx", P.wpx, wp && policy != PAXISIM_POLICY_CONSECUTIVE ? NIC * 48 : 0}, {"hist", P.hist, NC * P.H * 16},
      {"slot_of..qf", P.slot_of, C * 4 * 4}, {"phase", P.phase, C * 4}, {"agr", P.agr, (size_t)P.AR * P.NK * C * 8},
      {"agq", P.agq, P.AR ? 2 * AGMAX * NC * 16 : 0}, {"ep_inst", P.ep_inst, ep ? N * N * P.W * C * 64 : 0},
      {"ep_sce", P.ep_sce, ep ? 3 * N * NC * 4 : 0}, {"ep_cf", P.ep_cf, ep ? 2 * N * P.keys * NC * 4 : 0},
      {"ep_max", P.ep_max, ep ? P.keys * NC * 4 : 0}, {"kv_val", P.kv_val, P.kv ? P.keys * NC * 4 : 0},
      {"kv_ver", P.kv_ver, P.kv ? NC * 4 : 0}, {"wrep", P.wrep, (size_t)P.WK * C * 4},
      {"image", P.image, blocks * P.img.bytes}, {"rec", P.rec, blocks * P.rec_per_block * 16}};
  std::vector<std::pair<size_t, size_t>> live;   // [offset, end) of the regions that hold anything
  for (const Reg& r : regs) {
    CHECK(r.p != nullptr, "%s: %s is not bound", name, r.name);
    const size_t off = (size_t)((const char*)r.p - BASE);
    const bool in_block = coloc && r.p == (const void*)P.wlog;
    CHECK(off % 256 == (in_block ? 32u : 0u) && off + r.bytes <= pl.bound.total, "%s: %s at %zu + %zu of %zu", name, r.name, off,
          r.bytes, pl.bound.total);
    if (r.bytes) live.emplace_back(off, off + r.bytes);
  }
  std::sort(live.begin(), live.end());
  for (size_t i = 1; i < live.size(); i++)
    CHECK(live[i - 1].second <= live[i].first, "%s: regions [%zu,%zu) and [%zu,%zu) overlap", name, live[i - 1].first,
          live[i - 1].second, live[i].first, live[i].second);
  CHECK((size_t)((const char*)P.rec - BASE) == pl.bound.zero_bytes, "%s: rec does not begin at zero_bytes", name);
  CHECK(live.back().first == pl.bound.zero_bytes, "%s: rec is not the last region", name);
  // the pointers that share a carved region
  CHECK(P.slot == P.ballot + NC && P.execute == P.ballot + 2 * NC && P.meta == P.ballot + 3 * NC &&
            P.flags == P.ballot + 4 * NC && P.npend == P.ballot + 5 * NC && P.nfwd == P.ballot + 6 * NC,
        "%s: the seven replica scalars", name);
  CHECK(P.link_slow == P.link_drop + NC * N, "%s: link_slow", name);
  CHECK(P.cl_of == P.slot_of + C && P.frz == P.slot_of + 2 * C && P.qf == P.slot_of + 3 * C, "%s: slot maps", name);
  if (coloc) {
    CHECK((const char*)P.wlog == (const char*)P.wst + 32, "%s: wcoloc window is not 32 B into the block", name);
    CHECK((size_t)P.wst_str * 16 == (size_t)P.wlog_str * 4 && (size_t)P.wst_str * 16 >= 32 + 16 * (size_t)P.W &&
              P.wst_str * 16 % 128 == 0,
          "%s: wcoloc strides %u x 16 B, %u x 4 B", name, P.wst_str, P.wlog_str);
  } else {
    CHECK(P.wst_str == 2 && P.wlog_str == P.W * 4, "%s: strides %u, %u", name, P.wst_str, P.wlog_str);
  }
}

static void set_knobs(const Map& m) {
  for (const char* k : KNOBS) {
    auto it = m.find(std::string("knob.") + k);
    if (it == m.end()) unsetenv(k);
    else setenv(k, it->second.c_str(), 1);
  }
}

static int run_fixture(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) {
    std::printf("cannot open %s\n", path);
    return -1;
  }
  std::vector<std::pair<std::string, Map>> cases;
  std::string line;
  for (int c; (c = fgetc(f)) != EOF || !line.empty();) {
    if (c != '\n' && c != EOF) {
      line += (char)c;
      continue;
    }
    if (!line.empty() && line[0] == '[') cases.emplace_back(line.substr(1, line.size() - 2), Map());
    else if (!line.empty() && line[0] != '#' && !cases.empty()) {
      const size_t eq = line.find('=');
      if (eq != std::string::npos) cases.back().second[line.substr(0, eq)] = line.substr(eq + 1);
    }
    line.clear();
    if (c == EOF) break;
  }
  fclose(f);
  int refused = 0;
  for (const auto& cs : cases) {
    const char* name = cs.first.c_str();
    const Map& m = cs.second;
    set_knobs(m);
    const Inputs in = inputs_of(m);
    const Plan pl = run_plan(in, knobs_from_env());
    const Map got = outputs_of(pl);
    size_t want_n = 0;
    for (const auto& kv : m) {
      if (kv.first.compare(0, 4, "out.") && kv.first.compare(0, 4, "err.")) continue;
      want_n++;
      auto it = got.find(kv.first);
      CHECK(it != got.end() && it->second == kv.second, "%s: %s = %s, recorded %s", name, kv.first.c_str(),
            it == got.end() ? "(absent)" : it->second.c_str(), kv.second.c_str());
    }
    CHECK(want_n == got.size() && want_n > 0, "%s: %zu recorded outputs, the plan gives %zu", name, want_n, got.size());
    if (pl.rc) refused++;
    else invariants(name, pl, in.cfg.policy);
  }
  set_knobs(Map());
  std::printf("fixture: %zu cases, %d refusals\n", cases.size(), refused);
  CHECK(cases.size() >= 50 && refused >= 6, "the fixture has lost cases");
  return 0;
}

// Invariants over N x window x max_delay x protocol x kernel, with made-up kernel facts.
static void run_grid() {
  const uint32_t protos[] = {PAXISIM_PAXOS, PAXISIM_ABD, PAXISIM_WPAXOS, PAXISIM_EPAXOS};
  const uint32_t windows[] = {8, 16, 32, 64}, delays[] = {0, 4, 14};
  const int vgprs[] = {64, 128, 256, 512};
  unsigned total = 0, refused = 0;
  for (uint32_t proto : protos)
    for (uint32_t N = 1; N <= 16; N++)
      for (uint32_t W : windows)
        for (uint32_t delay : delays)
          for (int serial = 0; serial < 2; serial++) {
            Inputs in;
            memset(&in.cfg, 0, sizeof in.cfg);
            memset(&in.wl, 0, sizeof in.wl);
            memset(&in.fp, 0, sizeof in.fp);
            paxisim_config& c = in.cfg;
            c.protocol = proto;
            if (proto == PAXISIM_WPAXOS && N % 3 == 0) {
              c.n_zones = 3;
              c.npz[0] = c.npz[1] = c.npz[2] = N / 3;
            } else {
              c.n_zones = 1;
              c.npz[0] = N;
            }
            c.window = W; c.mbox_cap = 16; c.max_delay = delay; c.keys = 8; c.clusters = 130 + N; c.seed = 1;
            c.adaptive = 1; c.policy_threshold = 3; c.kv = N & 1; c.history = proto == PAXISIM_ABD ? N : 0;
            c.policy = N % 3;
            c.policy_interval = 5;
            c.policy_alpha = 0.5;
            in.wl.outstanding = 4;
            Knobs kn;
            kn.serial = serial != 0;
            total++;
            bool ok = true;
            for (int v : vgprs) {
              in.kf.vgprs = v;
              in.kf.max_threads = 1024;
              in.kf.serial = kn.serial;
              in.kf.staged = !kn.serial;
              in.kf.has_pipe = kn.serial;
              const Plan pl = run_plan(in, kn);
              if (pl.rc) {
                ok = false;
                break;
              }
              char name[96];
              snprintf(name, sizeof name, "grid proto=%u N=%u W=%u delay=%u serial=%d vgprs=%d", proto, N, W, delay, serial, v);
              invariants(name, pl, c.policy);
              CHECK(kn.serial ? pl.P.G == 1 && pl.P.J == 0 : pl.P.G <= 4 && pl.P.J <= 16, "%s: G=%u J=%u", name, pl.P.G, pl.P.J);
            }
            refused += !ok;
          }
  std::printf("grid: %u of %u shapes refused (%.1f%%)\n", refused, total, 100.0 * refused / total);
  CHECK(2 * refused < total, "more than half of the grid is refused: the grid checks too little");
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: %s tests/golden/create_plan.txt\n", argv[0]);
    return 2;
  }
  if (run_fixture(argv[1])) return 1;
  run_grid();
  if (g_fail) return 1;
  std::printf("create_plan OK\n");
  return 0;
}
