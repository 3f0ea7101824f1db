// host_snapshot.hip — snapshot, restore and fork (include/paxisim_snapshot.h, DESIGN.md §3.16,
// snapshot_plan.h, snapshot_kernel.h).  The arena but rec goes as plain copies; rec goes as its live
// records; the recorders' buffers as snapshot_plan.h snap_recorder_bufs lists them.
#include "host.h"
#include "lat_kernel.h"
#include "snapshot_kernel.h"
#include "snapshot_plan.h"
#include "trace_kernel.h"

using namespace pxs;
using namespace pxs_host;

static_assert(SNAP_LAT_SLICES == LAT_SLICES && SNAP_LAT_EXTRA == LAT_EXTRA, "snapshot_plan.h: the latency accumulators");
static_assert(SNAP_CMP_WORDS == CM_SUMS, "snapshot_plan.h: a pool's compaction words");
static_assert(sizeof(DevFault) == 48, "include/paxisim_snapshot.h: the FAULTS section");
extern "C" const char* paxisim_build_id(void);

// the moving-Mu tables back from the device: the handle keeps no host copy (create_on_device)
static int move_tables_host(paxisim* h, std::vector<uint32_t>& out) {
  out.clear();
  if (!h->d_move) return 0;
  out.resize((size_t)h->P.move_tables * PAXISIM_MAX_KEYS);
  HIPCHK(read_back(h, out.data(), h->d_move, out.size() * sizeof(uint32_t)));
  return 0;
}

static int handle_plan(paxisim* h, PlanWords* pw) {
  std::vector<uint32_t> mv;
  if (const int rc = move_tables_host(h, mv)) return rc;
  Params Q = h->P;
  const ArenaSize sz = carve_arena(Q, h->cfg.policy, nullptr, false);
  PlanExtra x;
  x.arena_zero = sz.zero_bytes;
  x.arena_total = sz.total;
  x.serial = h->ops.serial;
  x.staged = h->ops.staged;
  x.chunk = h->S;
  x.pipe_max = h->pipe_max;
  x.cmp_every = h->cmp_every;
  x.late_until = h->late_until;
  x.pipe_slots = h->pipe_slots;
  x.npools = h->npools;
  x.pool1_base = h->npools > 1 ? h->pool[1].base : 0u;
  x.move_cdf = mv.empty() ? nullptr : mv.data();
  paxisim_config cfg = h->cfg;
  cfg.protocol = h->P.variant;   // the protocol the caller asked for
  *pw = plan_words(cfg, h->wl, h->fp, h->P, x);
  return 0;
}

static unsigned snap_grid(uint64_t blocks) { return (unsigned)((blocks + SNAP_WAVES - 1) / SNAP_WAVES); }

// The count pass: per-block live records, scanned to each block's offset in the packed stream;
// offs: [blocks + 1] on the device, the grand total in its last word and *total.
static int mbox_count_pass(paxisim* h, DevBuf& offs, uint64_t* total) {
  const Params& P = h->P;
  const uint64_t blocks = P.C / LANES;
  const hipError_t e = offs.alloc<unsigned long long>(blocks + 1);
  if (e != hipSuccess) return fail(PAXISIM_ENOMEM, "snapshot count buffer (%llu bytes): %s",
                                   (unsigned long long)((blocks + 1) * 8), hipGetErrorString(e));
  unsigned long long* d = offs.as<unsigned long long>();
  unsigned long long tot = 0;
  mbox_count<<<snap_grid(blocks), SNAP_WAVES * LANES, 0, h->stream>>>(P.image, P.img, P.D * P.N * P.NS, P.M, blocks, d);
  mbox_scan<<<1, 1024, 0, h->stream>>>(d, blocks, d + blocks);
  HIPCHK(hipGetLastError());
  HIPCHK(read_back(h, &tot, d + blocks, sizeof tot));
  *total = tot;
  return 0;
}

static int snap_header_of(paxisim* h, uint64_t records, PlanWords* pw, SnapHeader* H) {
  if (const int rc = handle_plan(h, pw)) return rc;
  *H = snap_header(paxisim_build_id(), *pw, h->P.variant, h->P, h->cfg.policy, h->t, (uint32_t)h->faults.size(), h->npools,
                   snap_recorders(h->P, h->tr_rows), records);
  return 0;
}

extern "C" int paxisim_snapshot_size(paxisim* h, uint64_t* bytes) {
  if (!h || !bytes) return fail(PAXISIM_EINVAL, "null argument");
  if (const int rc = quiesce(h)) return rc;
  uint64_t records = 0;
  {
    DevBuf offs;
    if (const int rc = mbox_count_pass(h, offs, &records)) return rc;
  }
  PlanWords pw;
  SnapHeader H;
  if (const int rc = snap_header_of(h, records, &pw, &H)) return rc;
  *bytes = H.total_bytes;
  return 0;
}

extern "C" int paxisim_snapshot(paxisim* h, void* buf, uint64_t cap, uint64_t* written) {
  if (!h || !buf) return fail(PAXISIM_EINVAL, "null argument");
  if (const int rc = quiesce(h)) return rc;
  const Params& P = h->P;
  DevBuf offs, pack;
  uint64_t records = 0;
  if (const int rc = mbox_count_pass(h, offs, &records)) return rc;
  PlanWords pw;
  SnapHeader H;
  if (const int rc = snap_header_of(h, records, &pw, &H)) return rc;
  if (cap < H.total_bytes)
    return fail(PAXISIM_ERANGE, "snapshot needs %llu bytes, the buffer holds %llu", (unsigned long long)H.total_bytes,
                (unsigned long long)cap);
  if (records) {   // the packed stage, sized from the count pass
    const hipError_t e = pack.alloc<uint4>(records);
    if (e != hipSuccess)
      return fail(PAXISIM_ENOMEM, "snapshot packed stage (%llu bytes): %s", (unsigned long long)(records * sizeof(uint4)),
                  hipGetErrorString(e));
  }
  uint8_t* out = static_cast<uint8_t*>(buf);
  auto at = [&](uint32_t s) { return out + snap_offset(H, s); };
  memcpy(out, &H, sizeof H);
  memcpy(at(PAXISIM_SNAP_PLAN), pw.w.data(), pw.w.size() * 8);
  if (!h->faults.empty()) memcpy(at(PAXISIM_SNAP_FAULTS), h->faults.data(), h->faults.size() * sizeof(DevFault));
  hipError_t e = hipSuccess;
  auto d2h = [&](uint8_t* dst, const void* src, size_t n) {
    if (e == hipSuccess && n) e = hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, h->stream);
  };
  for (uint32_t p = 0; p < h->npools; p++) {
    uint8_t* w = at(PAXISIM_SNAP_POOLS) + (size_t)p * SNAP_POOL_BYTES;
    memset(w, 0, SNAP_POOL_BYTES);
    memcpy(w + 4 * SNAP_CMP_WORDS, &h->pool[p].last_cmp, 4);
    d2h(w, h->pool[p].d_cmp, 4 * SNAP_CMP_WORDS);
  }
  d2h(at(PAXISIM_SNAP_ARENA), h->arena, H.section_bytes[PAXISIM_SNAP_ARENA]);
  if (records && e == hipSuccess) {
    const uint64_t blocks = P.C / LANES;
    mbox_pack<<<snap_grid(blocks), SNAP_WAVES * LANES, 0, h->stream>>>(P.image, P.img, P.rec, P.rec_per_block,
                                                                      P.D * P.N * P.NS, P.M, blocks,
                                                                      offs.as<unsigned long long>(), records, pack.as<uint4>());
    e = hipGetLastError();
    d2h(at(PAXISIM_SNAP_MAILBOX), pack.p, records * sizeof(uint4));
  }
  for (const SnapBuf& b : snap_recorder_bufs(P, h->tr_rows)) d2h(at(b.section) + b.offset, b.ptr, b.bytes);
  if (P.tr_cap) memcpy(at(PAXISIM_SNAP_TRACE), h->tr_row.data(), snap_tr_row_bytes(P));
  const hipError_t es = hipStreamSynchronize(h->stream);   // whatever failed: the copies wrote the caller's buffer
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail(PAXISIM_EDEVICE, "snapshot: %s", hipGetErrorString(e));
  if (written) *written = H.total_bytes;
  return 0;
}

extern "C" int paxisim_snapshot_info(const void* buf, uint64_t bytes, struct paxisim_snapshot_info* out) {
  return snap_info(buf, bytes, out);
}

extern "C" int paxisim_restore(paxisim* h, const void* buf, uint64_t bytes) {
  if (!h || !buf) return fail(PAXISIM_EINVAL, "null argument");
  if (const int rc = quiesce(h)) return rc;
  Params& P = h->P;
  PlanWords pw;
  if (const int rc = handle_plan(h, &pw)) return rc;
  SnapHeader H;
  bool trace_carried = false;
  const SnapRecorders r = snap_recorders(P, h->tr_rows);
  if (const int rc = snap_check_restore(buf, bytes, paxisim_build_id(), pw, P, h->cfg.policy, h->npools, r, &H, &trace_carried))
    return rc;
  const uint8_t* in = static_cast<const uint8_t*>(buf);
  auto at = [&](uint32_t s) { return in + snap_offset(H, s); };
  if (trace_carried && memcmp(at(PAXISIM_SNAP_TRACE), h->tr_row.data(), snap_tr_row_bytes(P)))
    return fail(PAXISIM_EINVAL, "snapshot recorders differ: the traced clusters");
  // the pools' bounds lie inside their regions
  uint32_t cmp[MAX_POOLS][SNAP_CMP_WORDS], last_cmp[MAX_POOLS] = {0, 0};
  for (uint32_t p = 0; p < h->npools; p++) {
    const uint8_t* w = at(PAXISIM_SNAP_POOLS) + (size_t)p * SNAP_POOL_BYTES;
    memcpy(cmp[p], w, sizeof cmp[p]);
    memcpy(&last_cmp[p], w + sizeof cmp[p], 4);
    if (cmp[p][CM_BOUND] < h->pool[p].base || cmp[p][CM_BOUND] > h->pool[p].end)
      return fail(PAXISIM_EINVAL, "snapshot pool %u: bound %u outside its region [%u, %u]", p, cmp[p][CM_BOUND],
                  h->pool[p].base, h->pool[p].end);
  }
  if (H.step >= T_MAX) return fail(PAXISIM_EINVAL, "snapshot step %u", H.step);
  // the mailbox counts of the blob's images: every block's offset in the packed stream, and their
  // total, which must be the records carried (the counts decide what is live)
  const uint64_t blocks = P.C / LANES;
  const uint32_t nbox = P.D * P.N * P.NS;
  std::vector<unsigned long long> offs(blocks + 1);
  {
    const uint8_t* img0 = at(PAXISIM_SNAP_ARENA) + (P.image - static_cast<const uint8_t*>(h->arena));
    unsigned long long tot = 0;
    for (uint64_t b = 0; b < blocks; b++) {
      offs[b] = tot;
      const uint8_t* c = img0 + b * (size_t)P.img.bytes + P.img.off_cnt;
      for (size_t i = 0; i < (size_t)nbox * LANES; i++) tot += c[i] < P.M ? c[i] : P.M;
    }
    offs[blocks] = tot;
    if (tot != H.mailbox_records)
      return fail(PAXISIM_EINVAL, "snapshot mailbox counts add up to %llu records, the snapshot carries %llu", tot,
                  (unsigned long long)H.mailbox_records);
  }
  // everything the device writes need, before the first of them
  DevBuf d_offs, d_pack;
  const uint64_t records = H.mailbox_records;
  hipError_t e = d_offs.alloc<unsigned long long>(offs.size());
  if (e == hipSuccess && records) e = d_pack.alloc<uint4>(records);
  if (e != hipSuccess)
    return fail(PAXISIM_ENOMEM, "restore packed stage (%llu bytes): %s", (unsigned long long)(records * sizeof(uint4)),
                hipGetErrorString(e));
  auto h2d = [&](void* dst, const void* src, size_t n) {
    if (e == hipSuccess && n) e = hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, h->stream);
  };
  h2d(h->arena, at(PAXISIM_SNAP_ARENA), H.section_bytes[PAXISIM_SNAP_ARENA]);
  if (records) {
    h2d(d_offs.p, offs.data(), offs.size() * sizeof(unsigned long long));
    h2d(d_pack.p, at(PAXISIM_SNAP_MAILBOX), records * sizeof(uint4));
    if (e == hipSuccess) {
      mbox_unpack<<<snap_grid(blocks), SNAP_WAVES * LANES, 0, h->stream>>>(P.image, P.img, P.rec, P.rec_per_block, nbox, P.M,
                                                                          blocks, d_offs.as<unsigned long long>(), records,
                                                                          d_pack.as<uint4>());
      e = hipGetLastError();
    }
  }
  for (uint32_t p = 0; p < h->npools; p++) h2d(h->pool[p].d_cmp, cmp[p], sizeof cmp[p]);
  std::vector<DevFault> faults(H.n_faults);
  if (H.n_faults) memcpy(static_cast<void*>(faults.data()), at(PAXISIM_SNAP_FAULTS), H.n_faults * sizeof(DevFault));
  h2d(h->d_faults, faults.data(), faults.size() * sizeof(DevFault));
  for (const SnapBuf& b : snap_recorder_bufs(P, h->tr_rows))
    if (b.section != PAXISIM_SNAP_TRACE || trace_carried) h2d(b.ptr, at(b.section) + b.offset, b.bytes);
  if (P.tr_cap && !trace_carried && e == hipSuccess)   // the handle's trace alone: empty rows, recording goes on from the restored step
    e = hipMemsetAsync(P.tr_cnt, 0, snap_tr_cnt_bytes(P, h->tr_rows), h->stream);
  const hipError_t es = hipStreamSynchronize(h->stream);   // the copies read the caller's buffer and these vectors
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail(PAXISIM_EDEVICE, "restore: %s (the handle's state is undefined)", hipGetErrorString(e));
  h->faults.swap(faults);
  P.nfaults = H.n_faults;
  if (h->shape_fit) select_unit(h);   // the unit follows the restored fault count (either way)
  h->t = H.step;
  for (uint32_t p = 0; p < h->npools; p++) h->pool[p].last_cmp = last_cmp[p];
  return 0;
}

extern "C" int paxisim_fork(paxisim* h, paxisim** out) {
  if (!h || !out) return fail(PAXISIM_EINVAL, "null argument");
  if (const int rc = quiesce(h)) return rc;
  std::vector<uint32_t> mv;
  if (const int rc = move_tables_host(h, mv)) return rc;
  PlanWords pw;
  if (const int rc = handle_plan(h, &pw)) return rc;
  paxisim* f = new (std::nothrow) paxisim();
  if (!f) return fail(PAXISIM_ENOMEM, "oom");
  auto drop = [&](int rc) {
    paxisim_destroy(f);
    return rc;
  };
  f->cfg = h->cfg;
  f->wl = h->wl;
  f->wl.move_cdf = mv.empty() ? nullptr : mv.data();   // create uploads its own copy and keeps no pointer
  f->fp = h->fp;
  f->kn = h->kn;
  const Params& P = h->P;
  if (const int rc = create_on_device(f, h->kn, P.variant, P.N)) return drop(rc);
  if (P.lat_bins)
    if (const int rc = paxisim_latency_enable(f, P.lat_bins)) return drop(rc);
  if (P.ch_cap)
    if (const int rc = paxisim_client_history_enable(f, P.ch_cap)) return drop(rc);
  if (P.mv_cap)
    if (const int rc = paxisim_multiversion_enable(f, P.mv_cap)) return drop(rc);
  if (P.tr_cap) {
    std::vector<uint64_t> cl(h->tr_rows);
    for (uint64_t c = 0; c < h->cfg.clusters; c++)
      if (h->tr_row[c] != TR_NONE) cl[h->tr_row[c]] = c;
    if (const int rc = paxisim_trace_enable(f, cl.data(), h->tr_rows, P.tr_cap, P.tr_from, P.tr_to)) return drop(rc);
  }
  {   // the same plan, or the copies below would not fit
    PlanWords fw;
    if (const int rc = handle_plan(f, &fw)) return drop(rc);
    for (size_t i = 0; i < pw.w.size(); i++)
      if (fw.w[i] != pw.w[i])
        return drop(fail(PAXISIM_EDEVICE, "fork: the new handle's plan differs: %s (parent %llu, fork %llu)", pw.names[i],
                         (unsigned long long)pw.w[i], (unsigned long long)fw.w[i]));
  }
  const Params& Q = f->P;
  const ArenaSize sz = [&] { Params T = P; return carve_arena(T, h->cfg.policy, nullptr, false); }();
  hipError_t e = hipSuccess;
  auto d2d = [&](void* dst, const void* src, size_t n) {
    if (e == hipSuccess && n) e = hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, f->stream);
  };
  d2d(f->arena, h->arena, sz.zero_bytes);   // everything but rec
  if (e == hipSuccess) {                    // rec: the live records, by the counts just copied
    const uint64_t blocks = P.C / LANES;
    mbox_copy_live<<<snap_grid(blocks), SNAP_WAVES * LANES, 0, f->stream>>>(Q.image, Q.img, P.rec, Q.rec, Q.rec_per_block,
                                                                           Q.D * Q.N * Q.NS, Q.M, blocks);
    e = hipGetLastError();
  }
  for (uint32_t p = 0; p < h->npools; p++) d2d(f->pool[p].d_cmp, h->pool[p].d_cmp, sizeof(uint32_t) * SNAP_CMP_WORDS);
  d2d(f->d_faults, h->d_faults, h->faults.size() * sizeof(DevFault));
  const auto from = snap_recorder_bufs(P, h->tr_rows), to = snap_recorder_bufs(Q, f->tr_rows);
  for (uint32_t i = 0; i < SNAP_NBUF; i++) d2d(to[i].ptr, from[i].ptr, from[i].bytes);
  if (e == hipSuccess) e = hipStreamSynchronize(f->stream);
  if (e != hipSuccess) return drop(fail(PAXISIM_EDEVICE, "fork: %s", hipGetErrorString(e)));
  f->faults = h->faults;
  f->P.nfaults = P.nfaults;
  if (f->shape_fit) select_unit(f);
  f->t = h->t;
  for (uint32_t p = 0; p < h->npools; p++) f->pool[p].last_cmp = h->pool[p].last_cmp;
  if (f->npools > 1) f->main_ahead = true;   // the pools' streams wait for these copies
  *out = f;
  return 0;
}
