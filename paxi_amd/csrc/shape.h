// shape.h — the config-shape fields of Params as the step kernels read them.
//
// The device code of sim_core.h, paxos_kernel.h, paxisim_dev.h and the hook headers reads these
// fields as SH_<field>(P), never as P.<field>.  In a default build every accessor is the field
// itself, token for token, so a unit's device code is what it was with P.<field> written out.  A
// unit built with -DPXS_SHAPE=1 (__graft_entry__.TU_FLAGS) reads the constants of one fixed shape
// instead - 5-replica Multi-Paxos with config 2's features, the headline - and so carries none of
// the code of the features that shape does not have: with every feature behind a wave-uniform
// run-time test the headline kernel spilled 60 VGPRs and 369 SGPRs; with them gone it spills no VGPR.
//
// The constants have to reach the code as constants: __builtin_assume on the fields changes
// nothing, and overwriting the fields of the by-value Params sends the struct to scratch.
//
// Host code fills and reads Params as ever.  shape_plan.h (host only) decides at create whether a
// handle has this shape; only then does it run the fixed-shape unit, so a constant below always
// equals the handle's field.  Pinned (set A): N, NS, NI, NK, Z, W, q1, q2, kv, dist, rwc, thrifty,
// ephemeral, nfaults, late_workers, max_requests, locality_ppm, move_every, key_tail.  Not pinned:
// the fault process (drop_ppm, slow_ppm: five replicas without random faults are as common), and
// M, D, WK, phase_sort, phase_period, compact, fz (set B: the resource report gives them nothing
// more to win - the VGPR spills are already gone - so they stay run-time values).
#pragma once

#ifndef PXS_SHAPE
#define PXS_SHAPE 0
#endif

#if PXS_SHAPE
#define SH_N(P) (5u)
#define SH_NS(P) (6u)
#define SH_NI(P) (5u)
#define SH_NK(P) (1u)
#define SH_Z(P) (1u)
#define SH_W(P) (16u)
#define SH_q1(P) (PAXISIM_Q_MAJORITY)
#define SH_q2(P) (PAXISIM_Q_MAJORITY)
#define SH_kv(P) (1u)
#define SH_dist(P) (PAXISIM_DIST_UNIFORM)
#define SH_rwc(P) (0u)
#define SH_thrifty(P) (0u)
#define SH_ephemeral(P) (0u)
#define SH_nfaults(P) (0u)
#define SH_late_workers(P) (0u)
#define SH_max_requests(P) (0u)
#define SH_locality_ppm(P) (0u)
#define SH_move_every(P) (0u)
#define SH_move_every_div(P) (1u)   // the divisor in wl_key_moving, dead code under this shape
#define SH_key_tail(P) (0u)
#else
#define SH_N(P) P.N
#define SH_NS(P) P.NS
#define SH_NI(P) P.NI
#define SH_NK(P) P.NK
#define SH_Z(P) P.Z
#define SH_W(P) P.W
#define SH_q1(P) P.q1
#define SH_q2(P) P.q2
#define SH_kv(P) P.kv
#define SH_dist(P) P.dist
#define SH_rwc(P) P.rwc
#define SH_thrifty(P) P.thrifty
#define SH_ephemeral(P) P.ephemeral
#define SH_nfaults(P) P.nfaults
#define SH_late_workers(P) P.late_workers
#define SH_max_requests(P) P.max_requests
#define SH_locality_ppm(P) P.locality_ppm
#define SH_move_every(P) P.move_every
#define SH_move_every_div(P) P.move_every
#define SH_key_tail(P) P.key_tail
#endif
