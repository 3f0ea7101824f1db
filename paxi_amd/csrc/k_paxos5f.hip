// k_paxos5f.hip — Multi-Paxos serial step kernel, 5 replicas, compiled for config 2's fixed shape
// (shape.h, built with -DPXS_SHAPE=1): the unit of the headline.  k_paxos5s.hip is the unit of every
// other 5-replica config; paxisim_create chooses between them (shape_plan.h).
#define PXS_STEP_INSTANCE
#include "paxos_kernel.h"
#include "step_ops.h"

#if !PXS_SHAPE
#error "k_paxos5f.hip is built with -DPXS_SHAPE=1 (__graft_entry__.TU_FLAGS)"
#endif

namespace pxs {
StepOps paxos5_fixed_step_ops() { return SerialInstance<5, PaxosProto>::ops(); }
}  // namespace pxs
