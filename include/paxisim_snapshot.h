/* paxisim_snapshot.h — snapshot, restore and fork of a paxisim handle.
 *
 * An extension of paxisim.h: new symbols only, PAXISIM_ABI_VERSION stays 14 and no struct of
 * paxisim.h changes.  It is a header of its own so that paxisim.h, which every step-kernel unit
 * includes, stays byte-identical.
 *
 * A snapshot is the whole simulation state of a handle at its current step, as one
 * self-describing little-endian blob.  Of the mailboxes it carries only the live records: the
 * first cnt[box][lane] of each bucket's mbox_cap slots, packed on the device, so the blob's
 * mailbox section is exactly 16 * mailbox_records bytes however large the mailbox region is.
 *
 * Quiescence: snapshot_size, snapshot, restore and fork first do what every readout does (join
 * the pools, check the pipelined launches' error word, sync the stream); a handle with a sticky
 * pipeline error refuses with that error.
 *
 * Blob format, version 1.  All integers little-endian; offsets in bytes.
 *
 *   header (256 bytes)
 *     0   char[8]  magic "PXSSNAP\0"
 *     8   u32      version (1)
 *     12  u32      header_bytes (256)
 *     16  char[32] paxisim_build_id() of the library that wrote it, NUL padded
 *     48  u64      plan_hash: hash of the plan section's words
 *     56  u64      total_bytes = header_bytes + the sum of section_bytes
 *     64  u32      protocol (enum paxisim_protocol, as given to paxisim_create)
 *     68  u32      n_replicas
 *     72  u64      clusters
 *     80  u64      cluster_base
 *     88  u32      step: steps simulated so far (t)
 *     92  u32      recorders: PAXISIM_SNAP_HAS_* bits
 *     96  u64      mailbox_records: live mailbox records carried
 *     104 u64[9]   section_bytes, in the order of enum paxisim_snapshot_section
 *     176 u32      lat_bins        (0: no latency recorder)
 *     180 u32      ch_cap          (0: no client history)
 *     184 u32      mv_cap          (0: no multi-version Database)
 *     188 u32      tr_cap          (0: no trace)
 *     192 u32      tr_from
 *     196 u32      tr_to
 *     200 u32      tr_rows         traced clusters
 *     204 u32      n_faults        scripted fault windows
 *     208 u32      n_pools
 *     212 u32      n_plan_words
 *     216 u8[40]   zero
 *   sections, back to back, in this order (a section may be empty):
 *     PLAN     n_plan_words u64: the plan fingerprint's words (snapshot_plan.h, plan_word_names)
 *     FAULTS   n_faults x 48 B: the scripted fault table in its device form
 *     POOLS    n_pools x 48 B: {compaction words [8] u32, last_cmp u32, 3 x 0}
 *     ARENA    every per-cluster array but the mailbox records (create_plan.h carve_arena order)
 *     MAILBOX  mailbox_records x 16 B: the live records, by 64-cluster block, box, position, lane
 *     LAT      issue stamps [WK][C] u32, accumulators [8][WK][lat_bins + 4] u64
 *     CHIST    counts [WK][C] u32, ops [WK][C][ch_cap] x 16 B
 *     MV       counts [K][N][C] u32, values [K][N][C][mv_cap] u32
 *     TRACE    row table [C] u32, counts [tr_rows][N] u32, records [tr_rows][N][tr_cap][2] x 16 B
 *
 * The image layout and field meanings inside ARENA belong to the build that wrote the blob, which
 * is why restore asks for the same build id and the same plan.
 */
#ifndef PAXISIM_SNAPSHOT_H
#define PAXISIM_SNAPSHOT_H

#include "paxisim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PAXISIM_SNAPSHOT_VERSION  1
#define PAXISIM_SNAPSHOT_HEADER   256
#define PAXISIM_SNAPSHOT_SECTIONS 9

enum paxisim_snapshot_section {
  PAXISIM_SNAP_PLAN = 0, PAXISIM_SNAP_FAULTS, PAXISIM_SNAP_POOLS, PAXISIM_SNAP_ARENA, PAXISIM_SNAP_MAILBOX,
  PAXISIM_SNAP_LAT, PAXISIM_SNAP_CHIST, PAXISIM_SNAP_MV, PAXISIM_SNAP_TRACE
};

#define PAXISIM_SNAP_HAS_LAT    1u
#define PAXISIM_SNAP_HAS_CHIST  2u
#define PAXISIM_SNAP_HAS_MV     4u
#define PAXISIM_SNAP_HAS_TRACE  8u

/* a struct tag only (no typedef): the parsing function below bears the same name */
struct paxisim_snapshot_info {
  uint32_t version;
  uint32_t protocol;          /* enum paxisim_protocol */
  uint32_t n_replicas;
  uint32_t step;              /* t */
  uint64_t clusters, cluster_base;
  uint64_t mailbox_records;   /* live records carried: section_bytes[MAILBOX] / 16 */
  uint64_t total_bytes;
  uint64_t plan_hash;
  uint32_t recorders;         /* PAXISIM_SNAP_HAS_* */
  uint32_t n_faults;
  uint64_t section_bytes[PAXISIM_SNAPSHOT_SECTIONS];
  char build_id[32];
};

/* The exact size of a snapshot taken now (it runs the live-record count pass). */
int paxisim_snapshot_size(paxisim* h, uint64_t* bytes);

/* Write the snapshot into buf[0, cap).  cap below the size: PAXISIM_ERANGE, and nothing is written
 * past cap.  *written (may be NULL) receives the size. */
int paxisim_snapshot(paxisim* h, void* buf, uint64_t cap, uint64_t* written);

/* Overwrite the whole simulation state of h with the blob's.  h may be fresh or have run to any
 * step (restoring onto the handle that took the snapshot is a rewind); afterwards every readout and
 * every later step is what the source handle's was at the moment of the snapshot.  kernel_time
 * counters are not state and stay as they are.
 * PAXISIM_EINVAL, with a message naming the first difference, when the blob is truncated, has a
 * bad magic or version, section sizes that do not add up to `bytes`, another build id than the
 * library's, or another plan than the handle's (config, workload and its tables, fault process,
 * everything paxisim_create decided: layout numbers, kernel form, pools).  The scripted fault table
 * is state: restore replaces the handle's.  Recorders: latency, client history and multi-version
 * must be enabled alike with the same sizes on both sides.  The trace: alike on both sides, its
 * rows are carried; on the handle only, its rows are emptied and recording goes on from the
 * restored step inside its window; in the blob only, or with another table, PAXISIM_EINVAL.
 * A refused restore leaves h unchanged: everything is validated before the first device write. */
int paxisim_restore(paxisim* h, const void* buf, uint64_t bytes);

/* A second, independent handle on the same device at the same state, device to device.  It uses
 * the parent's plan and create-time knobs as they were decided at the parent's create (the
 * environment is not read again) and its own copies of the workload tables.  kernel_time counters
 * start at 0.  The mailbox region is filled by a live-record copy, never copied whole. */
int paxisim_fork(paxisim* h, paxisim** out);

/* Parse a blob's header: host only, works with no device. */
int paxisim_snapshot_info(const void* buf, uint64_t bytes, struct paxisim_snapshot_info* out);

#ifdef __cplusplus
}
#endif
#endif
