// create_plan.h — what paxisim_create decides before it touches the device (host only, no HIP
// runtime calls): the create-time knobs, the config checks, every Params field that needs neither
// the kernel nor a device pointer, the LDS plan, the arena carve and the launch schedule.
// paxisim_create (paxisim.hip) runs these in order between its device calls;
// tests/create_plan_check.cpp runs them without a GPU against tests/golden/create_plan.txt.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "paxisim_dev.h"
#include "pool_plan.h"

namespace pxs {

inline thread_local char g_err[512];
inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}

constexpr uint32_t PLAN_EP_NMAX = 10;   // = EP_NMAX (epaxos_kernel.h; paxisim.hip asserts it)

// The create-time knobs (the table).  A default-constructed Knobs is the empty
// environment; knobs_from_env is the library's only getenv of them.
struct Knobs {
  // PAXISIM_SERIAL: the serial kernel (one wave per tile plays every replica, sim_core.h sim_serial)
  // or, 0, the replica-per-wave one (A/B).  Any value but 0 and 1 is refused (serial_ok), so an A/B
  // arm cannot silently measure the default kernel.
  bool serial = true, serial_ok = true;
  int wlds = -1, wcoloc = -1;     // PAXISIM_WLDS, PAXISIM_WCOLOC: -1 unset, else 0 / 1
  uint32_t groups = 4;            // PAXISIM_GROUPS: cluster groups per workgroup at most (tuning)
  uint32_t stage = 16;            // PAXISIM_STAGE: staged picks per replica at most (tuning)
  bool compact = true;            // PAXISIM_COMPACT=0 turns compaction off (A/B)
  bool phase_sort = true;   // PAXISIM_PHASE_SORT (A/B r4h, config 2: 12.87-13.17 -> 16.05-16.33 G msgs/s)
  uint32_t phase_period = 3;      // PAXISIM_PHASE_PERIOD
  uint32_t pipe = 4;              // PAXISIM_PIPE: chunks per launch at most (1: off)
  bool has_pipe_spin = false;     // PAXISIM_PIPE_SPIN: the poll limit of a chunk wait (tests)
  uint32_t pipe_spin = 0;
  uint32_t pipe_slots = 0;        // PAXISIM_PIPE_SLOTS: cap on the persistent grid (0: none)
  uint32_t compact_every = 0;     // PAXISIM_COMPACT_EVERY: steps between compactions (0: unset)
  int pools = 0;                  // PAXISIM_POOLS: 0 unset, 1 or 2, -1 anything else (refused)
  // PAXISIM_SHAPE: 1 (the default) lets a handle of the fixed shape run the unit compiled for it
  // (shape_plan.h), 0 keeps every handle on the generic units (A/B); -1: anything else (refused)
  int shape = 1;
  long long arena_pad_mb = 0;     // PAXISIM_ARENA_PAD_MB, PAXISIM_ARENA_CONTIG: arena placement
  bool arena_contig = false;      // experiments (the two run modes)
};

inline Knobs knobs_from_env() {
  Knobs k;
  auto at_least_1 = [](const char* e) { return (uint32_t)atoi(e) ? (uint32_t)atoi(e) : 1u; };
  if (const char* e = getenv("PAXISIM_SERIAL")) {
    k.serial_ok = !strcmp(e, "0") || !strcmp(e, "1");
    k.serial = strcmp(e, "0") != 0;
  }
  if (const char* e = getenv("PAXISIM_WLDS")) k.wlds = atoi(e) != 0;
  if (const char* e = getenv("PAXISIM_WCOLOC")) k.wcoloc = atoi(e) != 0;
  if (const char* e = getenv("PAXISIM_GROUPS")) k.groups = at_least_1(e);
  if (const char* e = getenv("PAXISIM_STAGE")) k.stage = (uint32_t)atoi(e);
  if (const char* e = getenv("PAXISIM_COMPACT")) k.compact = atoi(e) != 0;
  if (const char* e = getenv("PAXISIM_PHASE_SORT")) k.phase_sort = atoi(e) != 0;
  if (const char* e = getenv("PAXISIM_PHASE_PERIOD")) k.phase_period = (uint32_t)atoi(e);
  if (const char* e = getenv("PAXISIM_PIPE")) k.pipe = at_least_1(e);
  if (const char* e = getenv("PAXISIM_PIPE_SPIN")) {
    k.has_pipe_spin = true;
    k.pipe_spin = (uint32_t)strtoul(e, nullptr, 0);
  }
  if (const char* e = getenv("PAXISIM_PIPE_SLOTS")) k.pipe_slots = (uint32_t)strtoul(e, nullptr, 0);
  if (const char* e = getenv("PAXISIM_COMPACT_EVERY")) k.compact_every = at_least_1(e);
  if (const char* e = getenv("PAXISIM_POOLS")) k.pools = !strcmp(e, "1") ? 1 : !strcmp(e, "2") ? 2 : -1;
  if (const char* e = getenv("PAXISIM_SHAPE")) k.shape = !strcmp(e, "1") ? 1 : !strcmp(e, "0") ? 0 : -1;
  if (const char* e = getenv("PAXISIM_ARENA_PAD_MB")) k.arena_pad_mb = atoll(e);
  if (const char* e = getenv("PAXISIM_ARENA_CONTIG")) k.arena_contig = atoi(e) != 0;
  return k;
}

// Everything paxisim_create takes from the step kernel's StepOps (step_ops.h).
struct KernelFacts {
  int vgprs = 0, max_threads = 0;   // hipFuncGetAttributes; <= 0: unknown
  bool staged = false;              // the instance carries the LDS-staged merge loop
  bool serial = false;              // the serial kernel
  bool has_pipe = false;            // it has pipelined launches (StepOps::launch_pipe)
};

inline Image proto_image(uint32_t protocol, uint32_t N, uint32_t W, uint32_t K, uint32_t WK, uint32_t D,
                         uint32_t wlds, bool packed) {
  if (protocol == PAXISIM_ABD) {
    const uint32_t kv = N * K * LANES * 4u;
    return image_layout(kv, kv, N * abd_ow(WK) * ABD_OPF * LANES * 4u, N, WK, D);
  }
  if (protocol == PAXISIM_WPAXOS)   // instance scalars in the image (wlds), or all in HBM
    return image_layout(wlds ? K * N * WP_WORDS * LANES * 4u : 0u, 0, 0, N, WK, D);
  if (protocol == PAXISIM_EPAXOS) return image_layout(0, 0, 0, N, WK, D);   // state in HBM
  // Multi-Paxos: the window's three planes, or none - the packed serial units keep their entries
  // outside the image (Params::plog)
  const uint32_t logb = packed ? 0u : N * W * LANES * 4u;
  return image_layout(logb, logb, logb, N, WK, D);
}

// LDS bytes of the agreement-ring arrival counts [2][N][lane] u8, after the image (either kernel)
inline uint32_t arrival_bytes(bool ring, uint32_t N) { return ring ? (2u * N * LANES + 15u) & ~15u : 0u; }

// The workload's key space (paxisim.h): ORDER / UNIFORM / CONFLICT range over
// key_space indices; CONFLICT's literal key 0 is its own index when key_min != 0.
inline uint32_t key_space_of(const paxisim_config* cfg, const paxisim_workload* wl) {
  const uint32_t keys = cfg->keys ? cfg->keys : 1u;
  return wl->key_space ? wl->key_space : keys;
}
inline int check_keys(const paxisim_config* cfg, const paxisim_workload* wl) {
  const uint32_t keys = cfg->keys ? cfg->keys : 1u;
  const uint32_t ks = key_space_of(cfg, wl);
  if (ks > keys) return fail(PAXISIM_EINVAL, "key_space %u exceeds keys %u", ks, keys);
  if (wl->distribution == PAXISIM_DIST_CONFLICT && wl->key_min && ks >= keys)
    return fail(PAXISIM_EINVAL, "conflict with key_min != 0 needs key_space < keys (literal key 0 has its own index)");
  if (wl->distribution == PAXISIM_DIST_TABLE) {
    for (uint32_t k = 1; k + 1u < keys; k++)
      if (wl->key_cdf[k] < wl->key_cdf[k - 1]) return fail(PAXISIM_EINVAL, "key_cdf must be non-decreasing");
    if (wl->key_tail && keys >= 2 && wl->key_tail < wl->key_cdf[keys - 2])
      return fail(PAXISIM_EINVAL, "key_tail below the last key_cdf threshold");
  } else if (wl->key_tail) {
    return fail(PAXISIM_EINVAL, "key_tail needs a table distribution");
  }
  if (wl->move_every) {
    if (wl->distribution != PAXISIM_DIST_TABLE) return fail(PAXISIM_EINVAL, "move_every needs a table distribution");
    if (!wl->move_cdf || wl->move_tables < 1 || wl->move_loop >= wl->move_tables)
      return fail(PAXISIM_EINVAL, "move_cdf / move_tables / move_loop");
    for (uint32_t e = 0; e < wl->move_tables; e++)
      for (uint32_t k = 1; k + 1u < keys; k++)
        if (wl->move_cdf[e * PAXISIM_MAX_KEYS + k] < wl->move_cdf[e * PAXISIM_MAX_KEYS + k - 1])
          return fail(PAXISIM_EINVAL, "move_cdf table %u must be non-decreasing", e);
  }
  return 0;
}

inline int check_config(const paxisim_config* cfg, const paxisim_workload* wl, const paxisim_fault_process* fp,
                        const Knobs& kn, uint32_t* N_out) {
  uint32_t N = 0;
  if (cfg->protocol > PAXISIM_EPAXOS || cfg->protocol == PAXISIM_M2PAXOS || cfg->protocol == PAXISIM_KPAXOS)
    return fail(PAXISIM_EUNSUPP, "protocol %u not built", cfg->protocol);
  if (cfg->protocol == PAXISIM_EPAXOS && (cfg->keys < 1 || cfg->keys > 32))
    return fail(PAXISIM_EINVAL, "EPaxos keys must be in [1,32]");
  if (cfg->protocol == PAXISIM_ABD && (cfg->keys < 1 || cfg->keys > 64)) return fail(PAXISIM_EINVAL, "keys");
  if (cfg->protocol == PAXISIM_WPAXOS && (cfg->keys < 1 || cfg->keys > 32))
    return fail(PAXISIM_EINVAL, "WPaxos keys must be in [1,32]");
  if (cfg->policy_threshold > 255) return fail(PAXISIM_EINVAL, "policy_threshold");
  if (cfg->policy > PAXISIM_POLICY_EMA) return fail(PAXISIM_EINVAL, "policy %u", cfg->policy);
  if (cfg->policy == PAXISIM_POLICY_MAJORITY && cfg->policy_interval < 1) return fail(PAXISIM_EINVAL, "policy_interval");
  if (cfg->policy == PAXISIM_POLICY_EMA && !(cfg->policy_alpha > 0.0 && cfg->policy_alpha <= 1.0))
    return fail(PAXISIM_EINVAL, "policy_alpha must be in (0, 1]");
  if (cfg->n_zones < 1 || cfg->n_zones > PAXISIM_MAX_ZONES) return fail(PAXISIM_EINVAL, "n_zones");
  for (uint32_t z = 0; z < cfg->n_zones; z++) {
    if (cfg->npz[z] < 1) return fail(PAXISIM_EINVAL, "npz[%u] must be >= 1", z);
    N += cfg->npz[z];
  }
  if (N < 1 || N > PAXISIM_MAX_N) return fail(PAXISIM_EINVAL, "N=%u out of range", N);
  if (cfg->protocol == PAXISIM_ABD && N > 15) return fail(PAXISIM_EINVAL, "ABD supports N <= 15");
  if (cfg->protocol == PAXISIM_EPAXOS && N > PLAN_EP_NMAX)
    return fail(PAXISIM_EINVAL, "EPaxos supports N <= %u", PLAN_EP_NMAX);
  if (cfg->window < 8 || cfg->window > PAXISIM_MAX_WINDOW || (cfg->window & (cfg->window - 1)))
    return fail(PAXISIM_EINVAL, "window must be a power of 2 in [8,64]");
  if (cfg->mbox_cap < 2 || cfg->mbox_cap > PAXISIM_MAX_MBOX) return fail(PAXISIM_EINVAL, "mbox_cap");
  if (cfg->max_delay > PAXISIM_MAX_DELAY) return fail(PAXISIM_EINVAL, "max_delay");
  if (cfg->q1 > PAXISIM_Q_FGRID_Q2 || cfg->q2 > PAXISIM_Q_FGRID_Q2) return fail(PAXISIM_EINVAL, "quorum kind");
  if (cfg->clusters < 1) return fail(PAXISIM_EINVAL, "clusters");
  if (cfg->agree_ring > 65536) return fail(PAXISIM_EINVAL, "agree_ring > 65536");
  if (wl->outstanding < 1 || wl->outstanding > PAXISIM_MAX_WORKERS) return fail(PAXISIM_EINVAL, "outstanding");
  if (wl->outstanding > cfg->mbox_cap) return fail(PAXISIM_EINVAL, "outstanding exceeds mbox_cap");
  if (wl->distribution > PAXISIM_DIST_TABLE) return fail(PAXISIM_EINVAL, "distribution %u", wl->distribution);
  if (wl->distribution == PAXISIM_DIST_CONFLICT && wl->conflicts > 100) return fail(PAXISIM_EINVAL, "conflicts > 100");
  if (int rc = check_keys(cfg, wl)) return rc;
  if (!kn.serial_ok) return fail(PAXISIM_EINVAL, "PAXISIM_SERIAL must be 0 or 1");
  if (kn.shape < 0) return fail(PAXISIM_EINVAL, "PAXISIM_SHAPE must be 0 or 1");
  for (uint32_t w = 0; w < wl->outstanding; w++)
    if (wl->target[w] >= N) return fail(PAXISIM_EINVAL, "target[%u]", w);
  if (fp->slow_ppm && (fp->slow_min > fp->slow_max || fp->slow_max > cfg->max_delay))
    return fail(PAXISIM_EINVAL, "slow delay range exceeds max_delay");
  const bool serial = kn.serial;
  const Image img = proto_image(cfg->protocol, N, cfg->window, cfg->keys, wl->outstanding, cfg->max_delay + 2u, 0,
                                serial && cfg->protocol == PAXISIM_PAXOS && paxos_packed(N));
  // the serial kernel keeps only the image's tail (client tables on) in LDS;
  // either kernel adds the agreement-ring arrival counts after the image
  const uint32_t agn = arrival_bytes(cfg->protocol != PAXISIM_ABD && cfg->protocol != PAXISIM_EPAXOS, N);
  const uint32_t need = (serial ? img.bytes - img.off_wcur : img.bytes) + agn;
  if (need > LDS_MAX)
    return fail(PAXISIM_EUNSUPP, "%s %u B exceeds LDS (%u B): reduce %smax_delay/replicas",
                serial ? "serial LDS (image tail and arrival counts)" : "workgroup image and arrival counts", need,
                LDS_MAX, serial ? "" : "window/");
  *N_out = N;
  return 0;
}

// Every Params field that depends neither on the kernel nor on a device pointer, the handle's
// 1-based "z.n" ids and its steps per launch.  cfg: checked, with M2Paxos / KPaxos already
// normalised to the WPaxos kernel; variant: the protocol the caller asked for.
inline void fill_params(Params& P, uint32_t* zone_of, uint32_t* node_of, uint32_t& S, const paxisim_config* cfg,
                        const paxisim_workload* wl, const paxisim_fault_process* fp, uint32_t variant, uint32_t N,
                        const Knobs& kn) {
  S = cfg->steps_per_launch ? cfg->steps_per_launch : 32;
  {   // per-type delivered counts are 16-bit in the kernel: at most NS*M messages per replica-step
    const uint32_t smax = 65535u / ((N + 1u) * cfg->mbox_cap);
    if (S > smax) S = smax;
  }
  memset(&P, 0, sizeof P);
  P.protocol = cfg->protocol;
  P.N = N;
  P.Z = cfg->n_zones;
  P.keys = cfg->keys ? cfg->keys : 1;
  P.write_ppm = wl->write_ppm;
  P.locality_ppm = wl->locality_ppm;
  P.dist = wl->distribution;
  P.conflicts = wl->conflicts;
  memcpy(P.key_cdf, wl->key_cdf, sizeof P.key_cdf);
  P.NK = cfg->protocol == PAXISIM_WPAXOS ? P.keys : 1u;
  P.NI = P.NK * N;
  P.adaptive = cfg->adaptive;
  P.policy_thr = cfg->policy_threshold;
  P.policy = cfg->policy;
  P.policy_interval = cfg->policy_interval;
  P.policy_alpha = cfg->policy_alpha;
  P.H = cfg->protocol == PAXISIM_ABD ? cfg->history : 0;
  P.AR = (cfg->protocol == PAXISIM_ABD || cfg->protocol == PAXISIM_EPAXOS) ? 0u
         : cfg->agree_ring ? cfg->agree_ring : (cfg->protocol == PAXISIM_WPAXOS ? 128u : 1024u);
  P.OW = abd_ow(wl->outstanding);
  P.W = cfg->window;
  P.M = cfg->mbox_cap;
  P.D = cfg->max_delay + 2u;
  P.NS = N + 1u;
  P.WK = wl->outstanding;
  P.wk_magic = 0xFFFFFFFFu / P.WK;
  P.max_requests = wl->max_requests;
  P.clusters = cfg->clusters;
  P.cluster_base = cfg->cluster_base;
  P.seed = cfg->seed;
  P.q1 = cfg->q1;
  P.q2 = cfg->q2;
  P.fz = cfg->fz;
  P.thrifty = cfg->thrifty;
  P.ephemeral = cfg->ephemeral_leader;
  P.rwc = cfg->reply_when_commit;
  if (cfg->protocol == PAXISIM_WPAXOS) {
    // kpaxos: Q1/Q2 from fz (wpaxos/kpaxos.go:15-27); no ReplyWhenCommit option
    // (kpaxos.go:35-39); the Paxos replica's -ephemeral_leader is not consulted
    P.q1 = cfg->fz ? PAXISIM_Q_FGRID_Q1 : PAXISIM_Q_GRID_ROW;
    P.q2 = cfg->fz ? PAXISIM_Q_FGRID_Q2 : PAXISIM_Q_GRID_COLUMN;
    P.rwc = 0;
    P.ephemeral = 0;
  }
  P.variant = cfg->protocol == PAXISIM_WPAXOS ? variant : cfg->protocol;
  if (P.variant == PAXISIM_M2PAXOS || P.variant == PAXISIM_KPAXOS) {   // m2paxos/kpaxos.go:15-21; paxos.NewPaxos default
    P.q1 = PAXISIM_Q_MAJORITY;
    P.q2 = PAXISIM_Q_MAJORITY;
  }
  if (P.variant == PAXISIM_M2PAXOS) P.adaptive = 1;
  P.key_min = wl->key_min;
  P.kspace = key_space_of(cfg, wl);
  P.kspace_magic = 0xFFFFFFFFu / P.kspace;
  P.conflict_key = wl->key_min ? P.kspace : 0u;
  P.key_tail = wl->distribution == PAXISIM_DIST_TABLE ? wl->key_tail : 0u;
  P.move_every = wl->move_every;
  P.move_tables = wl->move_every ? wl->move_tables : 0u;
  P.move_loop = wl->move_every ? wl->move_loop : 0u;
  P.kv = cfg->protocol != PAXISIM_ABD && cfg->kv ? 1u : 0u;   // m2paxos/replica.go:34-52 has no -adaptive switch
  P.max_delay = cfg->max_delay;
  P.drop_ppm = fp->drop_ppm;
  P.drop_len = fp->drop_len;
  P.slow_ppm = fp->slow_ppm;
  P.slow_len = fp->slow_len;
  P.slow_min = fp->slow_min;
  P.slow_max = fp->slow_max;
  uint32_t r = 0;
  for (uint32_t z = 0; z < P.Z; z++) {
    P.npz[z] = cfg->npz[z];
    P.zmask[z] = ((1u << cfg->npz[z]) - 1u) << r;
    for (uint32_t k = 0; k < cfg->npz[z]; k++, r++) {
      P.zone_of[r] = z;
      zone_of[r] = z + 1;
      node_of[r] = k + 1;
    }
    P.zfirst[z] = r - cfg->npz[z];
  }
  for (uint32_t w = 0; w < PAXISIM_MAX_WORKERS; w++) {
    P.target[w] = wl->target[w];
    P.start_step[w] = w < wl->outstanding ? wl->start_step[w] : 0u;
    if (P.start_step[w]) P.late_workers |= 1u << w;
  }

  P.keys_magic = 0xFFFFFFFFu / P.keys;
  for (uint32_t w = 0; w < PAXISIM_MAX_WORKERS; w++) {
    const uint32_t z = w < P.WK ? P.zone_of[P.target[w] < N ? P.target[w] : 0u] : 0u;
    P.wzone[w] = z;
    P.wnk[w] = z < P.keys ? (P.keys - z + P.Z - 1u) / P.Z : 0u;
    P.wnk_magic[w] = P.wnk[w] ? 0xFFFFFFFFu / P.wnk[w] : 0u;
  }
  // WPaxos: the instance scalars move into the tile image when one tile's
  // image (and the agreement counts) fits the LDS; PAXISIM_WLDS=0 keeps them in HBM (A/B)
  if (P.protocol == PAXISIM_WPAXOS) {
    // The serial kernel keeps the image in HBM, where the packed 32-B table
    // (wst, one line per bind) moves 0.67x the bytes of the image's word
    // planes at the same speed (A/B r4, config 5: 267 vs 400 GB per launch,
    // profiles/r4/config5_layout.json); PAXISIM_WLDS=0/1 overrides (A/B).
    P.wlds = (kn.wlds >= 0 ? kn.wlds != 0 : !kn.serial) &&
             (kn.serial || proto_image(P.protocol, N, P.W, P.keys, P.WK, P.D, 1, false).bytes +
                               arrival_bytes(P.AR != 0, N) <= LDS_MAX);
    // Each instance's 32-B scalars and its window in one block of whole lines: a
    // layout only, the kernels address both through wst_str / wlog_str.  On by default at W = 8, where
    // six of the eight entries share the line the bind loads (mirrored A/B r6g2, config 5: +4.2% over
    // the packed table at W = 8); at W = 16 it is 6% slower (r6g1).  PAXISIM_WCOLOC=0/1 overrides.
    P.wcoloc = !P.wlds && (kn.wcoloc >= 0 ? kn.wcoloc != 0 : P.W == 8u);
  }
  // Multi-Paxos: the window layout goes with the kernel - 16-B entries in plog for the serial units
  // that take them (paxos_packed), else the image's planes (paxos_kernel.h)
  P.packed = P.protocol == PAXISIM_PAXOS && kn.serial && paxos_packed(N);
  P.img = proto_image(P.protocol, N, P.W, P.keys, P.WK, P.D, P.wlds, P.packed != 0);
}

// The LDS of one cluster group and what hangs on it: groups per workgroup G, staged picks J, the
// offsets after the image, phase binning, the allocated lanes C and the records per block.
inline int plan_lds(Params& P, const Knobs& kn, const KernelFacts& f) {
  const uint32_t N = P.N;
  // Cluster groups per workgroup (sim_core.h): as many 64-cluster tiles as
  // the step kernel's registers leave wave slots for on every SIMD
  // (ceil(G*N/4) <= waves per SIMD) and the LDS holds, at most 4.
  const uint32_t vgprs = f.vgprs > 0 ? (uint32_t)f.vgprs : 512u;
  const uint32_t maxthr = f.max_threads > 0 ? (uint32_t)f.max_threads : N * LANES;
  const uint32_t alloc = (vgprs + 7u) / 8u * 8u;
  const uint32_t wps = alloc >= 512u ? 1u : (512u / alloc < 8u ? 512u / alloc : 8u);
  // per tile: the image, the agreement-ring arrival counts (not persisted:
  // drained every step), then the stage
  const uint32_t base = P.img.bytes + arrival_bytes(P.AR != 0, N);
  uint32_t G = 1;
  for (uint32_t g = 2; g <= kn.groups; g++)
    if ((g * N + 3u) / 4u <= wps && g * N * LANES <= maxthr && g * base <= LDS_MAX) G = g;
  P.G = G;
  // LDS stage for the first J picks of every replica's step, from what the groups leave
  const uint32_t room = LDS_MAX / G > base ? (LDS_MAX / G - base) / (N * LANES * 16u) : 0u;
  P.J = room < kn.stage ? room : kn.stage;
  if (!f.staged) P.J = 0;   // that instance has no staged loop
  P.off_agn = P.img.bytes;
  P.off_stage = base;
  P.lds_bytes = base + P.J * N * LANES * 16u;
  if (f.serial) {   // one tile per workgroup; LDS: the image tail and the arrival counts
    P.G = 1;
    P.J = 0;
    P.lds_tail = P.img.off_wcur;
    P.lds_bytes = base - P.lds_tail;
    // phase binning (Paxos, with compaction): per-residue record counts after the rest
    if (P.protocol == PAXISIM_PAXOS && kn.compact && kn.phase_sort) {
      P.phase_period = kn.phase_period;
      if (P.phase_period < 2u || P.phase_period > 7u) return fail(PAXISIM_EINVAL, "PAXISIM_PHASE_PERIOD in [2,7]");
      P.ph_rel = P.lds_tail + P.lds_bytes - P.img.off_cnt;
      P.lds_bytes += P.phase_period * LANES * 4u;
      P.phase_sort = 1;
    }
    // check_config bounds the image tail and the arrival counts; the phase
    // counts come on top of them: refuse here, not at the first launch
    if (P.lds_bytes > LDS_MAX)
      return fail(PAXISIM_EUNSUPP, "serial LDS %u B (image tail, arrival and phase counts) exceeds LDS (%u B): "
                  "reduce window/max_delay/replicas or set PAXISIM_PHASE_SORT=0", P.lds_bytes, LDS_MAX);
  }
  P.C = (P.clusters + LANES * P.G - 1) / (LANES * P.G) * (LANES * P.G);
  P.rec_per_block = P.D * N * P.NS * P.M * LANES;
  return 0;
}

template <typename T>
inline T* carve(uintptr_t& p, size_t count) {
  T* out = reinterpret_cast<T*>(p);
  p += (count * sizeof(T) + 255) & ~size_t(255);
  return out;
}

struct ArenaSize {
  size_t zero_bytes, total;   // the arena is zeroed up to zero_bytes: all of it but rec
};

// The arena: every per-cluster array of Params, each region rounded to 256 B, in this order; rec
// last, the only region not zeroed.  Sizes with a null base; `assign` binds P's pointers.
inline ArenaSize carve_arena(Params& P, uint32_t policy, char* base, bool assign) {
  const uint32_t N = P.N;
  const size_t C = P.C, NC = (size_t)N * C, NIC = (size_t)P.NI * C, blocks = C / LANES;
  const bool wp = P.protocol == PAXISIM_WPAXOS;
  uintptr_t p = reinterpret_cast<uintptr_t>(base);
  uint32_t* s7 = carve<uint32_t>(p, NC * 7);
  uint64_t* dg = carve<uint64_t>(p, NC);
  uint32_t* kc = carve<uint32_t>(p, C);
  uint32_t* pend = carve<uint32_t>(p, wp ? 0 : NC * PMAX);
  uint32_t* fwd = carve<uint32_t>(p, NC * FMAX);
  uint32_t* links = carve<uint32_t>(p, NC * N * 2);
  uint32_t* cke = carve<uint32_t>(p, NIC * CKR);
  uint64_t* ckd = carve<uint64_t>(p, NIC * CKR);
  uint4* gst = carve<uint4>(p, NIC * GMAX);
  uint32_t* st = carve<uint32_t>(p, NC * NSTAT);
  uint32_t* reqx = carve<uint32_t>(p, wp || P.packed ? 0 : NC * P.W);
  uint4* plog = carve<uint4>(p, P.packed ? NC * P.W : 0);
  // WPaxos instances: the scalars table and the windows apart, or (wcoloc) one block per instance
  // holding both - 32 B of scalars, then the window - padded to whole 128-B lines, so the entries
  // at the window's head share the line the bind loads
  const bool coloc = wp && !P.wlds && P.wcoloc;
  const size_t wblk_b = ((32u + 16u * P.W) + 127u) & ~size_t(127);
  uint4* wblk = carve<uint4>(p, coloc ? NIC * (wblk_b / 16u) : 0);
  uint4* wst = carve<uint4>(p, wp && !P.wlds && !coloc ? NIC * 2 : 0);
  uint64_t* wdig = carve<uint64_t>(p, wp && P.wlds ? NIC : 0);
  uint32_t* wlog = carve<uint32_t>(p, wp && !coloc ? NIC * P.W * 4 : 0);
  uint32_t* wpend = carve<uint32_t>(p, wp ? NIC * PMAX : 0);
  uint4* wpx = carve<uint4>(p, wp && policy != PAXISIM_POLICY_CONSECUTIVE ? NIC * 3 : 0);
  uint4* hist = carve<uint4>(p, NC * P.H);
  uint32_t* maps = carve<uint32_t>(p, C * 4);
  uint32_t* phs = carve<uint32_t>(p, C);
  unsigned long long* agr = carve<unsigned long long>(p, (size_t)P.AR * P.NK * C);
  uint4* agq = carve<uint4>(p, P.AR ? (size_t)2 * AGMAX * N * C : 0);
  const bool ep = P.protocol == PAXISIM_EPAXOS;
  uint4* ep_inst = carve<uint4>(p, ep ? (size_t)N * N * P.W * C * 4 : 0);
  uint32_t* ep_sce = carve<uint32_t>(p, ep ? (size_t)3 * N * N * C : 0);
  uint32_t* ep_cf = carve<uint32_t>(p, ep ? (size_t)2 * N * P.keys * N * C : 0);
  uint32_t* ep_max = carve<uint32_t>(p, ep ? (size_t)P.keys * N * C : 0);
  uint32_t* kv_val = carve<uint32_t>(p, P.kv ? (size_t)P.keys * N * C : 0);
  uint32_t* kv_ver = carve<uint32_t>(p, P.kv ? (size_t)N * C : 0);
  uint32_t* wrep = carve<uint32_t>(p, (size_t)P.WK * C);
  uint8_t* image = carve<uint8_t>(p, blocks * P.img.bytes);
  const uintptr_t zend = p;
  uint4* rec = carve<uint4>(p, blocks * P.rec_per_block);
  if (assign) {
    if (coloc) {
      wst = wblk;
      wlog = reinterpret_cast<uint32_t*>(wblk) + 8;
    }
    P.ballot = s7; P.slot = s7 + NC; P.execute = s7 + 2 * NC; P.meta = s7 + 3 * NC;
    P.flags = s7 + 4 * NC; P.npend = s7 + 5 * NC; P.nfwd = s7 + 6 * NC;
    P.digest = dg; P.kc = kc; P.pend = pend; P.fwd = fwd;
    P.link_drop = links; P.link_slow = links + NC * N;
    P.ck_e = cke; P.ck_d = ckd; P.stats = st; P.reqx = reqx; P.plog = plog; P.hist = hist; P.image = image; P.rec = rec;
    P.wst = wst; P.wdig = wdig; P.wlog = wlog; P.wpend = wpend; P.gst = gst; P.wpx = wpx;
    P.wst_str = coloc ? (uint32_t)(wblk_b / 16u) : 2u;
    P.wlog_str = coloc ? (uint32_t)(wblk_b / 4u) : P.W * 4u;
    P.slot_of = maps; P.cl_of = maps + C; P.frz = maps + 2 * C; P.qf = maps + 3 * C;
    P.phase = phs;
    P.agr = agr;
    P.agq = agq;
    P.ep_inst = ep_inst; P.ep_sce = ep_sce; P.ep_cf = ep_cf; P.ep_max = ep_max;
    P.kv_val = kv_val; P.kv_ver = kv_ver; P.wrep = wrep;
  }
  const uintptr_t b0 = reinterpret_cast<uintptr_t>(base);
  return ArenaSize{(size_t)(zend - b0), (size_t)(p - b0)};
}

// The launch schedule.  PAXISIM_PIPE applies before the XCD probe (plan_pipe: the chunks per launch
// to probe for, 1 = not pipelined, no probe); the rest follows the probe's outcome.
struct Schedule {
  bool compact;          // Paxos (the swap covers its arrays), unless PAXISIM_COMPACT=0
  uint32_t late_until;   // no compaction before every late worker has started
  uint32_t pipe_max;     // chunks of S steps per launch at most
  uint32_t cmp_every;    // steps between compactions
};
inline uint32_t plan_pipe(const Knobs& kn, const KernelFacts& f) {
  return kn.pipe > 1 && f.serial && f.has_pipe ? kn.pipe : 1u;
}
inline Schedule plan_schedule(const Params& P, const Knobs& kn, const KernelFacts& f, uint32_t S, bool probe_ok) {
  Schedule s;
  s.compact = P.protocol == PAXISIM_PAXOS && kn.compact;
  s.late_until = 0;
  for (uint32_t w = 0; w < P.WK; w++)
    if (P.start_step[w] + 1u > s.late_until) s.late_until = P.start_step[w] + 1u;
  s.pipe_max = probe_ok ? plan_pipe(kn, f) : 1u;
  // pipelined (PAXISIM_PIPE > 1, the default): compaction every three chunks (at most pipe_max), so
  // they fuse (A/B r5v / r5x, config 2: 50-step chunks with compaction every 100 +2.0% against every
  // 50 unpipelined, every 200 with four chunks +0.0%; 25-step chunks every 75 another +0.9 / +2.2%
  // in the two run modes, every 50 +0.5 / +1.1%)
  s.cmp_every = s.pipe_max > 1 ? (s.pipe_max < 3u ? s.pipe_max : 3u) * S : 50u;
  if (kn.compact_every) s.cmp_every = kn.compact_every;
  return s;
}

}  // namespace pxs
