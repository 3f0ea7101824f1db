// shape_plan_check.cpp — a stand-alone program around paxi_amd/csrc/shape_plan.h (host only), built
// by tests/test_shape_plan.py with the address and undefined-behaviour sanitizers: the headline's
// exact config fits the fixed shape, every single departure from it - one case per pinned field -
// does not and names that field alone, and the PAXISIM_SHAPE knob reads 1 / 0 / refused.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>

#include "create_plan.h"
#include "shape_plan.h"

using namespace pxs;

namespace {
int failures = 0;

struct Case {
  paxisim_config cfg;
  paxisim_workload wl;
  paxisim_fault_process fp;
  uint32_t n_faults;
  Knobs kn;
};

// BASELINE config 2 as bench.py builds it: Multi-Paxos, 5 replicas in one zone, window 16, mailbox
// 32, max_delay 4, a Database, 8 workers on replica 0, uniform keys, Drop/Slow at 1e-3
Case headline() {
  Case c;
  memset(&c.cfg, 0, sizeof c.cfg);
  memset(&c.wl, 0, sizeof c.wl);
  memset(&c.fp, 0, sizeof c.fp);
  c.cfg.protocol = PAXISIM_PAXOS;
  c.cfg.n_zones = 1;
  c.cfg.npz[0] = 5;
  c.cfg.q1 = c.cfg.q2 = PAXISIM_Q_MAJORITY;
  c.cfg.window = 16;
  c.cfg.mbox_cap = 32;
  c.cfg.max_delay = 4;
  c.cfg.clusters = 1u << 20;
  c.cfg.seed = 42;
  c.cfg.steps_per_launch = 20;
  c.cfg.kv = 1;
  c.wl.outstanding = 8;
  c.wl.distribution = PAXISIM_DIST_UNIFORM;
  c.fp.drop_ppm = 1000;
  c.fp.drop_len = 50;
  c.fp.slow_ppm = 1000;
  c.fp.slow_len = 50;
  c.fp.slow_min = 1;
  c.fp.slow_max = 4;
  c.n_faults = 0;
  c.kn = Knobs{};
  return c;
}

uint32_t misfit(const Case& c) {
  uint32_t N = 0;
  for (uint32_t z = 0; z < c.cfg.n_zones; z++) N += c.cfg.npz[z];
  return shape_misfit(&c.cfg, &c.wl, c.n_faults, ShapeKnobs{c.kn.serial, c.kn.shape},
                      c.kn.serial && c.cfg.protocol == PAXISIM_PAXOS && paxos_packed(N));
}

// what fill_params writes for the case, against the constants of shape.h
bool params_fit(const Case& c) {
  uint32_t N = 0;
  if (check_config(&c.cfg, &c.wl, &c.fp, c.kn, &N)) {
    printf("  check_config refused: %s\n", g_err);
    return false;
  }
  Params P;
  uint32_t zone_of[PAXISIM_MAX_N], node_of[PAXISIM_MAX_N], S = 0;
  fill_params(P, zone_of, node_of, S, &c.cfg, &c.wl, &c.fp, c.cfg.protocol, N, c.kn);
  P.nfaults = c.n_faults;
  return shape_fields_fit(ShapeFields{P.N, P.NS, P.NI, P.NK, P.Z, P.W, P.q1, P.q2, P.kv, P.dist, P.rwc, P.thrifty,
                                      P.ephemeral, P.nfaults, P.late_workers, P.max_requests, P.locality_ppm,
                                      P.move_every, P.key_tail});
}

void expect(const char* what, const std::function<void(Case&)>& change, uint32_t want, bool params_leave = true) {
  Case c = headline();
  change(c);
  const uint32_t got = misfit(c);
  bool ok = got == want;
  // the filled Params agree with the decision: a departure in a config field shows in Params too
  // (the two knob departures do not: they choose the kernel, not a field)
  if (ok && want && params_leave && params_fit(c)) ok = false;
  printf("%-34s misfit %05x (%s) want %05x%s\n", what, got, got && !(got & (got - 1u)) ? shape_misfit_name(got) : "-",
         want, ok ? "" : "   FAILED");
  if (!ok) failures++;
}
}  // namespace

int main() {
  {
    Case c = headline();
    const bool ok = misfit(c) == 0 && params_fit(c);
    printf("%-34s misfit %05x, params %s%s\n", "headline (config 2)", misfit(c), params_fit(c) ? "fit" : "do not fit",
           ok ? "" : "   FAILED");
    if (!ok) failures++;
    // the random fault process is not pinned: none at all still fits
    memset(&c.fp, 0, sizeof c.fp);
    c.cfg.mbox_cap = 16;
    c.cfg.max_delay = 2;
    c.wl.outstanding = 4;
    if (misfit(c) != 0 || !params_fit(c)) {
      printf("headline without faults, M=16, D=4, WK=4   FAILED\n");
      failures++;
    }
  }
  expect("N=3", [](Case& c) { c.cfg.npz[0] = 3; }, SHAPE_N);
  expect("N=9", [](Case& c) { c.cfg.npz[0] = 9; }, SHAPE_N | SHAPE_KERNEL);   // 9 replicas: plane windows too
  expect("N=5 in two zones", [](Case& c) { c.cfg.n_zones = 2; c.cfg.npz[0] = 2; c.cfg.npz[1] = 3; }, SHAPE_Z);
  expect("window 8", [](Case& c) { c.cfg.window = 8; }, SHAPE_W);
  expect("window 32", [](Case& c) { c.cfg.window = 32; }, SHAPE_W);
  for (uint32_t q = PAXISIM_Q_ALL; q <= PAXISIM_Q_FGRID_Q2; q++) {
    char name[32];
    snprintf(name, sizeof name, "q2 kind %u", q);
    expect(name, [q](Case& c) { c.cfg.q2 = q; }, SHAPE_Q2);
    snprintf(name, sizeof name, "q1 kind %u", q);
    expect(name, [q](Case& c) { c.cfg.q1 = q; }, SHAPE_Q1);
  }
  expect("thrifty", [](Case& c) { c.cfg.thrifty = 1; }, SHAPE_THRIFTY);
  expect("ephemeral_leader", [](Case& c) { c.cfg.ephemeral_leader = 1; }, SHAPE_EPHEMERAL);
  expect("reply_when_commit", [](Case& c) { c.cfg.reply_when_commit = 1; }, SHAPE_RWC);
  expect("kv=0", [](Case& c) { c.cfg.kv = 0; }, SHAPE_KV);
  expect("one scripted fault", [](Case& c) { c.n_faults = 1; }, SHAPE_NFAULTS);
  expect("one late worker", [](Case& c) { c.wl.start_step[7] = 100; }, SHAPE_LATE_WORKERS);
  expect("max_requests=1000", [](Case& c) { c.wl.max_requests = 1000; }, SHAPE_MAX_REQUESTS);
  expect("distribution order", [](Case& c) { c.wl.distribution = PAXISIM_DIST_ORDER; }, SHAPE_DIST);
  expect("distribution conflict", [](Case& c) { c.wl.distribution = PAXISIM_DIST_CONFLICT; c.wl.conflicts = 50; },
         SHAPE_DIST);
  expect("distribution table", [](Case& c) { c.wl.distribution = PAXISIM_DIST_TABLE; }, SHAPE_DIST);
  expect("locality_ppm=1", [](Case& c) { c.wl.locality_ppm = 1; }, SHAPE_LOCALITY);
  {
    static uint32_t tables[2 * PAXISIM_MAX_KEYS];
    expect("moving keys", [](Case& c) {
      c.wl.distribution = PAXISIM_DIST_TABLE;
      c.wl.move_every = 100;
      c.wl.move_tables = 2;
      c.wl.move_cdf = tables;
    }, SHAPE_DIST | SHAPE_MOVE);   // moving keys need a table distribution (check_keys)
  }
  expect("protocol WPaxos", [](Case& c) { c.cfg.protocol = PAXISIM_WPAXOS; c.cfg.keys = 8; c.cfg.npz[0] = 5; },
         SHAPE_PROTOCOL | SHAPE_KERNEL);
  expect("PAXISIM_SERIAL=0", [](Case& c) { c.kn.serial = false; }, SHAPE_KERNEL, false);
  expect("PAXISIM_SHAPE=0", [](Case& c) { c.kn.shape = 0; }, SHAPE_OFF, false);

  // the knob as the library reads it: unset and "1" are on, "0" is off, anything else is refused
  struct { const char* v; int shape; bool refused; } knob[] = {
      {nullptr, 1, false}, {"1", 1, false}, {"0", 0, false}, {"2", -1, true}, {"", -1, true}, {"yes", -1, true}};
  for (const auto& k : knob) {
    if (k.v) setenv("PAXISIM_SHAPE", k.v, 1);
    else unsetenv("PAXISIM_SHAPE");
    Case c = headline();
    c.kn = knobs_from_env();
    uint32_t N = 0;
    const int rc = check_config(&c.cfg, &c.wl, &c.fp, c.kn, &N);
    const bool ok = c.kn.shape == k.shape && (rc != 0) == k.refused && (!k.refused || rc == PAXISIM_EINVAL) &&
                    (k.refused || (misfit(c) == 0) == (k.shape == 1));
    printf("PAXISIM_SHAPE=%-8s shape %d, check_config %d%s\n", k.v ? k.v : "(unset)", c.kn.shape, rc, ok ? "" : "   FAILED");
    if (!ok) failures++;
  }
  unsetenv("PAXISIM_SHAPE");
  if (failures) {
    printf("shape_plan: %d FAILED\n", failures);
    return 1;
  }
  printf("shape_plan OK\n");
  return 0;
}
