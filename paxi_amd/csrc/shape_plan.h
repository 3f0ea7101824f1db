// shape_plan.h — does a handle have the fixed shape k_paxos5f.hip is compiled for?  (host only: the
// C ABI's structs and nothing of HIP, as pool_plan.h)
//
// shape.h pins nineteen Params fields of the step kernels to constants in that unit.  shape_misfit
// restates, field by field, what fill_params (create_plan.h) makes of the config, the workload, the
// scripted faults and the knobs, and answers with one bit per pinned field that departs from its
// constant: 0 means the handle may run the fixed-shape unit.  paxisim_create asks it after its plan
// steps (and checks the filled Params against the same constants, shape_fields_fit); the only
// pinned field that can change after create is the number of scripted faults, so paxisim_fault_add,
// paxisim_restore and paxisim_fork ask again with the new count and switch the handle's unit.
// tests/shape_plan_check.cpp runs it without a GPU.
#pragma once
#include <stdint.h>

#include "../../include/paxisim.h"

namespace pxs {

enum ShapeMisfit : uint32_t {
  SHAPE_OFF = 1u << 0,            // PAXISIM_SHAPE=0
  SHAPE_KERNEL = 1u << 1,         // not the serial kernel with packed windows (PAXISIM_SERIAL=0)
  SHAPE_PROTOCOL = 1u << 2,       // not Multi-Paxos: NK = 1, NI = N
  SHAPE_N = 1u << 3,              // N = 5 (NS = 6, NI = 5)
  SHAPE_Z = 1u << 4,              // Z = 1
  SHAPE_W = 1u << 5,              // W = 16
  SHAPE_Q1 = 1u << 6,             // q1 = MAJORITY
  SHAPE_Q2 = 1u << 7,             // q2 = MAJORITY
  SHAPE_KV = 1u << 8,             // kv = 1
  SHAPE_DIST = 1u << 9,           // dist = UNIFORM (key_tail = 0: only a table has a tail)
  SHAPE_RWC = 1u << 10,           // rwc = 0
  SHAPE_THRIFTY = 1u << 11,       // thrifty = 0
  SHAPE_EPHEMERAL = 1u << 12,     // ephemeral = 0
  SHAPE_NFAULTS = 1u << 13,       // nfaults = 0
  SHAPE_LATE_WORKERS = 1u << 14,  // late_workers = 0
  SHAPE_MAX_REQUESTS = 1u << 15,  // max_requests = 0
  SHAPE_LOCALITY = 1u << 16,      // locality_ppm = 0
  SHAPE_MOVE = 1u << 17,          // move_every = 0
  SHAPE_NBITS = 18
};

inline const char* shape_misfit_name(uint32_t bit) {
  static const char* const names[SHAPE_NBITS] = {
      "PAXISIM_SHAPE=0", "kernel", "protocol", "N", "Z", "W", "q1", "q2", "kv", "dist", "rwc", "thrifty",
      "ephemeral", "nfaults", "late_workers", "max_requests", "locality_ppm", "move_every"};
  for (uint32_t i = 0; i < SHAPE_NBITS; i++)
    if (bit == (1u << i)) return names[i];
  return "?";
}

// The knobs the decision reads (create_plan.h Knobs), and whether the Multi-Paxos windows of this
// replica count are packed (paxisim_dev.h paxos_packed).
struct ShapeKnobs {
  bool serial;   // PAXISIM_SERIAL is not 0
  int shape;     // PAXISIM_SHAPE: 1, 0, or -1 (refused by check_config before anything asks)
};

// cfg: checked, with M2Paxos / KPaxos already normalised to the WPaxos kernel, as fill_params takes it
inline uint32_t shape_misfit(const paxisim_config* cfg, const paxisim_workload* wl, uint32_t n_faults,
                             const ShapeKnobs& kn, bool packed) {
  uint32_t m = 0;
  if (kn.shape != 1) m |= SHAPE_OFF;
  if (!kn.serial || !packed) m |= SHAPE_KERNEL;
  if (cfg->protocol != PAXISIM_PAXOS) m |= SHAPE_PROTOCOL;
  uint32_t N = 0;
  for (uint32_t z = 0; z < cfg->n_zones && z < PAXISIM_MAX_ZONES; z++) N += cfg->npz[z];
  if (N != 5u) m |= SHAPE_N;
  if (cfg->n_zones != 1u) m |= SHAPE_Z;
  if (cfg->window != 16u) m |= SHAPE_W;
  if (cfg->q1 != PAXISIM_Q_MAJORITY) m |= SHAPE_Q1;
  if (cfg->q2 != PAXISIM_Q_MAJORITY) m |= SHAPE_Q2;
  if (!cfg->kv) m |= SHAPE_KV;
  if (wl->distribution != PAXISIM_DIST_UNIFORM) m |= SHAPE_DIST;
  if (cfg->reply_when_commit) m |= SHAPE_RWC;
  if (cfg->thrifty) m |= SHAPE_THRIFTY;
  if (cfg->ephemeral_leader) m |= SHAPE_EPHEMERAL;
  if (n_faults) m |= SHAPE_NFAULTS;
  for (uint32_t w = 0; w < wl->outstanding && w < PAXISIM_MAX_WORKERS; w++)
    if (wl->start_step[w]) m |= SHAPE_LATE_WORKERS;
  if (wl->max_requests) m |= SHAPE_MAX_REQUESTS;
  if (wl->locality_ppm) m |= SHAPE_LOCALITY;
  if (wl->move_every) m |= SHAPE_MOVE;
  return m;
}

// The pinned fields as a filled Params holds them, in shape.h's order: paxisim_create's cross-check
// of shape_misfit against what fill_params really wrote.
struct ShapeFields {
  uint32_t N, NS, NI, NK, Z, W, q1, q2, kv, dist, rwc, thrifty, ephemeral, nfaults, late_workers, max_requests,
      locality_ppm, move_every, key_tail;
};
inline bool shape_fields_fit(const ShapeFields& f) {
  return f.N == 5u && f.NS == 6u && f.NI == 5u && f.NK == 1u && f.Z == 1u && f.W == 16u &&
         f.q1 == PAXISIM_Q_MAJORITY && f.q2 == PAXISIM_Q_MAJORITY && f.kv == 1u && f.dist == PAXISIM_DIST_UNIFORM &&
         !f.rwc && !f.thrifty && !f.ephemeral && !f.nfaults && !f.late_workers && !f.max_requests &&
         !f.locality_ppm && !f.move_every && !f.key_tail;
}

}  // namespace pxs
