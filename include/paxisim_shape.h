/* paxisim_shape.h — which step-kernel unit a handle runs.
 *
 * An extension of paxisim.h: one new symbol, PAXISIM_ABI_VERSION stays 14 and no struct of
 * paxisim.h changes.  It is a header of its own so that paxisim.h, which every step-kernel unit
 * includes, stays byte-identical.
 *
 * The library holds the 5-replica Multi-Paxos step kernels twice: the generic unit, which serves
 * every config, and a unit compiled for one fixed config shape - the headline's: 5 replicas in one
 * zone, window 16, majority quorums, a Database, uniform keys, and no thrifty, ephemeral-leader or
 * ReplyWhenCommit option, scripted fault, late worker, request limit, zone locality or moving keys
 * (the random fault process, mailbox, delay and workers are free).  paxisim_create picks the fixed-
 * shape unit for a handle of exactly that shape; both keep the same state in the same layout and
 * compute the same results, so the choice shows in speed alone.  PAXISIM_SHAPE=0 in the environment
 * of paxisim_create keeps every handle on the generic unit (1 is the default, any other value is
 * PAXISIM_EINVAL).  A handle leaves the fixed-shape unit when paxisim_fault_add gives it a scripted
 * fault (or paxisim_restore brings some), and returns to it when a restore leaves it none.
 */
#ifndef PAXISIM_SHAPE_H
#define PAXISIM_SHAPE_H

#include "paxisim.h"

#ifdef __cplusplus
extern "C" {
#endif

enum paxisim_unit {
  PAXISIM_UNIT_GENERIC      = 0,  /* the unit of the handle's protocol and replica count */
  PAXISIM_UNIT_FIXED_PAXOS5 = 1   /* 5-replica Multi-Paxos compiled for the fixed shape above */
};

/* *unit = the enum paxisim_unit whose kernels the handle's next launch runs.  No device work. */
int paxisim_step_unit(paxisim* h, uint32_t* unit);

#ifdef __cplusplus
}
#endif

#endif /* PAXISIM_SHAPE_H */
