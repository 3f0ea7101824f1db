/* paxisim_verdict.h — per-cluster verdict words and a device-side search over them.
 *
 * An extension of paxisim.h: new symbols only, PAXISIM_ABI_VERSION stays 14 and no struct of
 * paxisim.h changes.  It is a header of its own so that paxisim.h, which every step-kernel unit
 * includes, stays byte-identical.
 *
 * The totals of paxisim_check, paxisim_linearizable, paxisim_client_linearizable, paxisim_consensus
 * and paxisim_stats.flagged[] say how many clusters; the verdict word says which.  One u32 per
 * cluster, indexed by the local cluster id (never by the slot), evaluated on the device:
 *
 *   bits 0..7   the PAXISIM_F_* values: the OR of the replicas' flags
 *   bit  8      PAXISIM_V_AGREE         the cluster is one that paxisim_check counts (0 for EPaxos)
 *   bit  9      PAXISIM_V_CONSENSUS     paxisim_consensus_failed's mask for the cluster is non-zero
 *   bit  10     PAXISIM_V_LIN           ABD's replica-side history has an anomaly in this cluster
 *   bit  11     PAXISIM_V_CLIENT_LIN    the client history has an anomaly in this cluster
 *   bit  12     PAXISIM_V_LIN_SKIPPED   a requested linearizability scan skipped a partition of this
 *                                       cluster (more than 16384 ops): bits 10 / 11 are unknown there
 *   bit  13     PAXISIM_V_TRUNCATED     a requested scan judged a truncated prefix: a client-history
 *                                       row (CLIENT_LIN) or a multi-version row (CONSENSUS) of this
 *                                       cluster dropped entries
 *   bit  16     PAXISIM_V_QUIET         every mailbox bucket of the cluster is empty (all arrival
 *                                       steps, all links, the client queues included), every worker's
 *                                       start_step has passed and the cluster is not POISON
 *   bit  17     PAXISIM_V_WAITING       some worker's current command id is non-zero, as
 *                                       paxisim_read_client reports it
 *   bit  18     PAXISIM_V_STALLED       QUIET and WAITING: a worker waits for a reply and no message
 *                                       is in flight anywhere (Paxi has no retries)
 *
 * Bits 9 to 13 come from the scans, which are expensive, so every call takes a `scans` mask of
 * PAXISIM_V_CONSENSUS | PAXISIM_V_LIN | PAXISIM_V_CLIENT_LIN: only the requested scans run, and the
 * bits of scans not requested are 0.  Every other bit is always evaluated.  Any other bit in `scans`
 * is PAXISIM_EINVAL.  A requested scan the handle cannot run is PAXISIM_EUNSUPP before anything is
 * launched: LIN without protocol ABD and history > 0, CLIENT_LIN without
 * paxisim_client_history_enable, CONSENSUS without paxisim_multiversion_enable.
 *
 * Every call evaluates afresh: nothing is cached between calls, and the word buffers are scratch,
 * not simulation state (a snapshot does not carry them).  The calls that take a handle do what every
 * readout does first: join the pools, check the pipelined launches' error word, sync the stream.
 */
#ifndef PAXISIM_VERDICT_H
#define PAXISIM_VERDICT_H

#include "paxisim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PAXISIM_V_FLAGS        0x000000FFu   /* the PAXISIM_F_* bits */
#define PAXISIM_V_AGREE        0x00000100u
#define PAXISIM_V_CONSENSUS    0x00000200u
#define PAXISIM_V_LIN          0x00000400u
#define PAXISIM_V_CLIENT_LIN   0x00000800u
#define PAXISIM_V_LIN_SKIPPED  0x00001000u
#define PAXISIM_V_TRUNCATED    0x00002000u
#define PAXISIM_V_QUIET        0x00010000u
#define PAXISIM_V_WAITING      0x00020000u
#define PAXISIM_V_STALLED      0x00040000u
#define PAXISIM_V_SCANS        (PAXISIM_V_CONSENSUS | PAXISIM_V_LIN | PAXISIM_V_CLIENT_LIN)
#define PAXISIM_V_ALL          0x00073FFFu   /* every defined bit */

/* The bits this handle can produce: the always-evaluated ones (AGREE only where paxisim_check
 * compares anything, so not for EPaxos) and those of the scans it can run. */
int paxisim_verdict_available(paxisim* h, uint32_t* bits);

/* words[i] = the verdict word of local cluster lo + i, i in [0, n).  A range outside the handle:
 * PAXISIM_ERANGE. */
int paxisim_verdicts(paxisim* h, uint32_t scans, uint64_t lo, uint64_t n, uint32_t* words);

/* The local ids of the clusters whose word matches, ascending:
 *   (any == 0 || (word & any) != 0) && (word & none) == 0.
 * At most cap ids are written (ids may be NULL when cap is 0); *total is the exact number of
 * matches either way.  Bits in any or none outside PAXISIM_V_ALL: PAXISIM_EINVAL. */
int paxisim_find(paxisim* h, uint32_t scans, uint32_t any, uint32_t none,
                 uint64_t* ids, uint64_t cap, uint64_t* total);

/* counts[b] = the clusters whose word has bit b set; counts[0..7] equal paxisim_stats.flagged[]. */
int paxisim_verdict_counts(paxisim* h, uint32_t scans, uint64_t counts[32]);

/* The same search over n caller-supplied words on `device`, with no handle: ids are indices into
 * words.  any and none are taken as they are. */
int paxisim_select_words(int device, const uint32_t* words, uint64_t n, uint32_t any, uint32_t none,
                         uint64_t* ids, uint64_t cap, uint64_t* total);

#ifdef __cplusplus
}
#endif
#endif
