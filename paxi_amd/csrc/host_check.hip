// host_check.hip — the recorders a handle can switch on and the checks over what they and the
// replicas keep: the agreement scan, client request latency, the ABD and the client-side op
// histories with their linearizability scans, the multi-version Database and Consensus, message
// traces, and the per-cluster verdict words with the search over them.
#include <type_traits>

#define PXS_LAT_REDUCE   // this unit defines and launches lat_reduce (lat_kernel.h)
#define PXS_CHIST_READ   // and chist_read_kernel (chist_kernel.h)
#define PXS_MV_SCAN      // and mv_consensus_kernel (mv_kernel.h)
#include "host.h"
#include "sim_core.h"   // the workload's draws, and lat_kernel.h, chist_kernel.h, mv_kernel.h, trace_kernel.h
#include "lin_kernel.h"
#include "verdict_kernel.h"

using namespace pxs;
using namespace pxs_host;

// The allocate-and-fill step of the four *_enable calls: every buffer of the list allocated, then
// zeroed or loaded from `init` where asked, on the handle's stream, complete on return - or none
// left allocated.
struct NewBuf {
  void** p;
  size_t bytes;
  bool zero;
  const void* init;   // host data to load, or null
};
template <class T>
static NewBuf new_buf(T*& p, size_t bytes, bool zero, const void* init = nullptr) {
  return NewBuf{reinterpret_cast<void**>(&p), bytes, zero, init};
}
static hipError_t alloc_all(paxisim* h, std::initializer_list<NewBuf> list) {
  hipError_t e = hipSuccess;
  for (const NewBuf& b : list)
    if (e == hipSuccess) e = hipMalloc(b.p, b.bytes);
  for (const NewBuf& b : list) {
    if (e == hipSuccess && b.init) e = hipMemcpyAsync(*b.p, b.init, b.bytes, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && b.zero) e = hipMemsetAsync(*b.p, 0, b.bytes, h->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess)
    for (const NewBuf& b : list) {
      if (*b.p) (void)hipFree(*b.p);
      *b.p = nullptr;
    }
  return e;
}

// Agreement scan (client.go:279-320; tla/wpaxos.tla Safety): replicas that
// executed the same number of slots must hold the same digest, and digest
// checkpoints taken at the same executed count must agree.  The per-cluster body is verdict_kernel.h agree_bad, which the
// verdict pass calls too, so the count and the PAXISIM_V_AGREE bit cannot drift apart.
__global__ void check_kernel(Params P, uint64_t* out) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t bad = 0;
  if (c < P.clusters && P.protocol != PAXISIM_EPAXOS) bad = agree_bad(P, c) ? 1u : 0u;   // EPaxos: no single log (paxisim.h)
  bad = wave_sum(bad);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd((unsigned long long*)out, (unsigned long long)bad);
}

extern "C" int paxisim_check(paxisim* h, uint64_t* violations) {
  if (!h || !violations) return fail(PAXISIM_EINVAL, "null argument");
  if (const int rc = enter_checked(h)) return rc;   // results only of launches that fully ran
  HIPCHK(hipMemsetAsync(h->d_scratch, 0, sizeof(uint64_t), h->stream));
  check_kernel<<<(unsigned)(h->P.C / 256 + 1), 256, 0, h->stream>>>(h->P, h->d_scratch);
  HIPCHK(hipGetLastError());
  HIPCHK(read_back(h, violations, h->d_scratch, sizeof(uint64_t)));
  return 0;
}

// ---------------------------------------------------------------------------
// Client request latency (include/paxisim.h, DESIGN.md §3.12, lat_kernel.h)
// ---------------------------------------------------------------------------
static size_t lat_acc_words(const Params& P) { return (size_t)LAT_SLICES * P.WK * lat_row(P.lat_bins); }

extern "C" int paxisim_latency_enable(paxisim* h, uint32_t bins) {
  if (!h) return fail(PAXISIM_EINVAL, "null handle");
  if (bins < 16u || bins > PAXISIM_LAT_MAX_BINS || (bins & (bins - 1u)))
    return fail(PAXISIM_EINVAL, "latency bins must be a power of two in [16, %u]", PAXISIM_LAT_MAX_BINS);
  if (h->P.lat_bins) return fail(PAXISIM_EINVAL, "latency is already enabled");
  if (h->t) return fail(PAXISIM_EINVAL, "latency can only be enabled before the first step");
  if (const int jrc = enter(h)) return jrc;
  // the recording build of the handle's kernel: the same instance, so the launch shape chosen at create fits it
  const StepOps ops = lat_step_ops_for(h->P.protocol, h->P.N, h->P.wlds != 0, h->ops.serial);
  int vgprs = 0, maxthr = 0;
  if (!ops.launch || ops.serial != h->ops.serial || ops.staged != h->ops.staged ||
      ops.attrs(&vgprs, &maxthr) != hipSuccess || (!ops.serial && h->P.G * h->P.N * LANES > (uint32_t)maxthr))
    return fail(PAXISIM_EUNSUPP, "no latency-recording build of this handle's step kernel");
  Params P = h->P;
  P.lat_bins = bins;
  // every worker present at create issued its first request at step 0: the zeroed stamps
  const size_t sb = sizeof(uint32_t) * P.WK * P.C, ab = sizeof(unsigned long long) * lat_acc_words(P);
  const size_t ob = sizeof(unsigned long long) * P.WK * lat_row(bins);
  unsigned long long* o = nullptr;
  const hipError_t e = alloc_all(h, {new_buf(P.lat_stamp, sb, true), new_buf(P.lat_acc, ab, true), new_buf(o, ob, false)});
  if (e != hipSuccess) return fail(PAXISIM_ENOMEM, "latency buffers (%zu bytes): %s", sb + ab + ob, hipGetErrorString(e));
  h->P = P;
  h->ops = ops;
  h->lds_set = -1;        // the dynamic-LDS ceiling is per kernel
  if (h->fixed) select_unit(h);   // the recording twin of the fixed-shape unit
  h->d_lat_out = o;
  return 0;
}

extern "C" int paxisim_latency_reset(paxisim* h) {
  if (!h) return fail(PAXISIM_EINVAL, "null handle");
  if (!h->P.lat_bins) return fail(PAXISIM_EINVAL, "latency is not enabled");
  if (const int jrc = enter(h)) return jrc;
  // on the launch stream: after every step launched so far, before the next one
  HIPCHK(hipMemsetAsync(h->P.lat_acc, 0, sizeof(unsigned long long) * lat_acc_words(h->P), h->stream));
  return 0;
}

extern "C" int paxisim_latency_get(paxisim* h, uint32_t worker, paxisim_latency* out, uint64_t* hist) {
  if (!h || !out) return fail(PAXISIM_EINVAL, "null argument");
  if (!h->P.lat_bins) return fail(PAXISIM_EINVAL, "latency is not enabled");
  if (worker != PAXISIM_ALL_WORKERS && worker >= h->P.WK) return fail(PAXISIM_EINVAL, "no worker %u", worker);
  if (const int rc = enter_checked(h)) return rc;   // results only of launches that fully ran
  const uint32_t bins = h->P.lat_bins;
  const size_t row = lat_row(bins), n = (size_t)h->P.WK * row;
  lat_reduce<<<(unsigned)((n + 255) / 256), 256, 0, h->stream>>>(h->P, h->d_lat_out);
  HIPCHK(hipGetLastError());
  std::vector<unsigned long long> acc(n);
  HIPCHK(read_back(h, acc.data(), h->d_lat_out, n * sizeof(unsigned long long)));
  memset(out, 0, sizeof *out);
  out->bins = bins;
  out->min = 0xFFFFFFFFu;
  if (hist) memset(hist, 0, sizeof(uint64_t) * bins);
  for (uint32_t w = 0; w < h->P.WK; w++) {
    if (worker != PAXISIM_ALL_WORKERS && w != worker) continue;
    const unsigned long long* a = acc.data() + (size_t)w * row;
    uint64_t cnt = a[bins + LAT_OVF];
    for (uint32_t b = 0; b < bins; b++) {
      cnt += a[b];
      if (hist) hist[b] += a[b];
    }
    out->count += cnt;
    out->sum += a[bins + LAT_SUM];
    out->overflow += a[bins + LAT_OVF];
    if (cnt) {
      out->min = std::min(out->min, 0xFFFFFFFFu - (uint32_t)a[bins + LAT_NMIN]);
      out->max = std::max(out->max, (uint32_t)a[bins + LAT_MAX]);
    }
  }
  return 0;
}

extern "C" int paxisim_latency_stat_of(const paxisim_latency* l, const uint64_t* hist, double step_ms,
                                       paxisim_latency_stat* out) {
  if (!l || !hist || !out) return fail(PAXISIM_EINVAL, "null argument");
  if (l->bins > PAXISIM_LAT_MAX_BINS) return fail(PAXISIM_ERANGE, "bins exceeds PAXISIM_LAT_MAX_BINS");
  if (l->count == 0) return fail(PAXISIM_EINVAL, "no samples");
  memset(out, 0, sizeof *out);
  out->size = l->count;
  out->mean = (double)l->sum * step_ms / (double)l->count;
  out->min = l->min * step_ms;
  out->max = l->max * step_ms;
  out->exact = 1;
  // stat.go:44-66: element int(p * size) of the sorted samples
  const double ps[4] = {0.5, 0.95, 0.99, 0.999};
  double* dst[4] = {&out->median, &out->p95, &out->p99, &out->p999};
  for (int k = 0; k < 4; k++) {
    uint64_t idx = (uint64_t)(ps[k] * (double)l->count);
    if (idx >= l->count) idx = l->count - 1;
    uint64_t cum = 0;
    uint32_t b = 0;
    for (; b < l->bins; b++) {
      cum += hist[b];
      if (idx < cum) break;
    }
    if (b < l->bins) {
      *dst[k] = b * step_ms;
    } else {                      // inside the overflow bin: only its bounds are known
      *dst[k] = out->max;
      out->exact = 0;
    }
  }
  return 0;
}

// Completed ABD operations of one cluster, 5 words per op {key, is_write,
// value, start, end}, replicas in index order, each in completion order.
extern "C" int paxisim_history(paxisim* h, uint64_t cluster, uint32_t* buf, uint32_t cap_ops, uint32_t* n_out) {
  if (!h || !n_out) return fail(PAXISIM_EINVAL, "null argument");
  if (cluster >= h->cfg.clusters) return fail(PAXISIM_ERANGE, "cluster");
  if (const int rc = enter_checked(h)) return rc;   // results only of launches that fully ran
  HIPCHK(hipStreamSynchronize(h->stream));   // step kernels run on the non-blocking h->stream
  const Params& P = h->P;
  std::vector<uint32_t> len(P.N);
  for (uint32_t r = 0; r < P.N; r++)
    HIPCHK(hipMemcpy(&len[r], &P.execute[rc_host(P, r, cluster)], 4, hipMemcpyDeviceToHost));
  uint32_t n = 0;
  for (uint32_t r = 0; r < P.N && P.H; r++) {
    std::vector<uint4> tmp(len[r]);
    if (len[r])
      HIPCHK(hipMemcpy(tmp.data(), &P.hist[((size_t)r * P.C + cluster) * P.H], len[r] * sizeof(uint4),
                       hipMemcpyDeviceToHost));
    for (uint32_t j = 0; j < len[r]; j++, n++) {
      if (!buf || n >= cap_ops) continue;
      uint32_t* o = buf + 5 * (size_t)n;
      o[0] = tmp[j].x & 0x7FFFFFFFu;
      o[1] = tmp[j].x >> 31;
      o[2] = tmp[j].y;
      o[3] = tmp[j].z;
      o[4] = tmp[j].w;
    }
  }
  *n_out = n;
  return 0;
}

// History.ReadFile (history.go:115-178) into the device history of one replica.
extern "C" int paxisim_history_load(paxisim* h, uint64_t cluster, uint32_t replica, const uint32_t* ops, uint32_t n) {
  if (!h || (n && !ops)) return fail(PAXISIM_EINVAL, "null argument");
  if (cluster >= h->cfg.clusters || replica >= h->P.N) return fail(PAXISIM_ERANGE, "bad replica");
  if (h->P.protocol != PAXISIM_ABD) return fail(PAXISIM_EUNSUPP, "op history is kept by ABD only");
  if (n > h->P.H) return fail(PAXISIM_EINVAL, "%u ops exceed history capacity %u", n, h->P.H);
  if (const int jrc = enter(h)) return jrc;
  HIPCHK(hipStreamSynchronize(h->stream));
  const Params& P = h->P;
  std::vector<uint4> tmp(n ? n : 1);
  for (uint32_t j = 0; j < n; j++) {
    const uint32_t* o = ops + 5 * (size_t)j;
    if (o[0] >= h->P.keys || o[1] > 1u) return fail(PAXISIM_EINVAL, "op %u: bad key (keys = %u) or is_write", j, h->P.keys);
    tmp[j] = make_uint4(o[0] | (o[1] << 31), o[2], o[3], o[4]);
  }
  if (n)
    HIPCHK(hipMemcpy(&P.hist[((size_t)replica * P.C + cluster) * P.H], tmp.data(), n * sizeof(uint4),
                     hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(&P.execute[rc_host(P, replica, cluster)], &n, 4, hipMemcpyHostToDevice));
  return 0;
}

// History.Linearizable over the history source S of every cluster (lin_kernel.h): LinAbd, the
// replicas' completed ABD ops, or LinClient, the workers' ops of any protocol (chist_kernel.h).
template <class S>
static int lin_scan(paxisim* h, uint64_t* anomalies, uint64_t* ops, uint64_t* skipped, uint32_t* mark = nullptr,
                    uint32_t mark_bit = 0) {
  if (const int rc = enter_checked(h)) return rc;   // results only of launches that fully ran
  HIPCHK(hipStreamSynchronize(h->stream));
  const Params& P = h->P;
  // clusters per launch: each gets a stage of sources * per_source ops (ABD: N*H; its history grouped by key).
  // The stage takes up to a quarter of the free HBM (2-16 GiB): fewer, longer
  // launches leave less of each launch's last round of workgroups idle
  // (config 3: 21 -> 6 launches); PAXISIM_LIN_STAGE_MB overrides (A/B).
  const size_t cap = (size_t)S::sources(P) * S::per_source(P);
  size_t budget = 2ull << 30, freeb = 0, totb = 0;
  if (hipMemGetInfo(&freeb, &totb) == hipSuccess) budget = std::max(budget, std::min<size_t>(freeb / 4, 16ull << 30));
  if (const char* e = getenv("PAXISIM_LIN_STAGE_MB")) budget = std::max<size_t>(1, (size_t)atoll(e)) << 20;
  const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(P.clusters, budget / (cap * sizeof(uint4))));
  DevBuf d_stage, d_big, d_out, d_bws;
  size_t bws_bytes = 0;
  const size_t nout = LIN_NOUT + 8;
  HIPCHK(d_stage.alloc<uint4>(chunk * cap));
  HIPCHK(d_big.alloc<uint2>(chunk * P.keys));
  HIPCHK(d_out.alloc<unsigned long long>(nout));
  uint4* stage = d_stage.as<uint4>();
  uint2* big = d_big.as<uint2>();
  unsigned long long* out = d_out.as<unsigned long long>();
  HIPCHK(hipMemsetAsync(out, 0, nout * sizeof(unsigned long long), h->stream));
  const uint32_t lds = LIN_LW * LIN_SORT_BYTES;
  unsigned long long tot[LIN_NOUT] = {0};
  for (uint64_t c0 = 0; c0 < P.clusters; c0 += chunk) {
    const uint64_t nc = std::min<uint64_t>(chunk, P.clusters - c0);
    HIPCHK(hipMemsetAsync(out + LIN_BIG, 0, 2 * sizeof(unsigned long long), h->stream));
    lin_cluster_kernel<S><<<(unsigned)nc, LIN_LW * 64, lds, h->stream>>>(P, c0, stage, out, big, mark, mark_bit);
    unsigned long long bc[2] = {0, 0};
    HIPCHK(hipGetLastError());
    HIPCHK(read_back(h, bc, out + LIN_BIG, sizeof bc));
    if (bc[0]) {   // partitions above LIN_SMAX ops: one wave each, scratch in HBM
      tot[LIN_BIG] += bc[0];
      tot[LIN_NMAX] = std::max<unsigned long long>(tot[LIN_NMAX], bc[1]);
      const uint32_t nw = (uint32_t)((bc[1] + 63u) / 64u);     // bc[1] <= LIN_VMAX (larger: skipped)
      const size_t per = lin_scratch_bytes(nw, true);
      const uint32_t waves = (uint32_t)std::max<unsigned long long>(
          1, std::min<unsigned long long>(std::min<unsigned long long>(bc[0], 2048), (2ull << 30) / per));
      const size_t need = (size_t)waves * per;
      if (need > bws_bytes) {
        HIPCHK(d_bws.alloc<uint8_t>(need));
        bws_bytes = need;
      }
      uint8_t* bws = d_bws.as<uint8_t>();
      const uint32_t* idmap = std::is_same<S, LinAbd>::value ? P.cl_of : nullptr;   // LinAbd walks slots
      if (nw <= 64u)
        lin_big_kernel<1><<<waves, 64, 0, h->stream>>>(stage, big, (uint32_t)bc[0], bws, nw, out, mark, mark_bit, c0,
                                                       (uint32_t)cap, idmap);
      else
        lin_big_kernel<LIN_WPL_MAX><<<waves, 64, 0, h->stream>>>(stage, big, (uint32_t)bc[0], bws, nw, out, mark,
                                                                 mark_bit, c0, (uint32_t)cap, idmap);
      HIPCHK(hipGetLastError());
    }
  }
  uint64_t res[LIN_NOUT + 8] = {0};
  HIPCHK(read_back(h, res, out, sizeof res));
#ifdef PXS_LIN_STAMPS
  fprintf(stderr, "lin stamps (wave-cycles): p1 %llu p2 %llu sort %llu run %llu | add %llu look %llu merge %llu reach %llu\n",
          (unsigned long long)res[LIN_NOUT + 0], (unsigned long long)res[LIN_NOUT + 1], (unsigned long long)res[LIN_NOUT + 2],
          (unsigned long long)res[LIN_NOUT + 3], (unsigned long long)res[LIN_NOUT + 4], (unsigned long long)res[LIN_NOUT + 5],
          (unsigned long long)res[LIN_NOUT + 6], (unsigned long long)res[LIN_NOUT + 7]);
#endif
  h->lin_big = tot[LIN_BIG];
  h->lin_nmax = tot[LIN_NMAX];
  if (anomalies) *anomalies = res[LIN_ANOM];
  if (ops) *ops = res[LIN_OPS];
  if (skipped) *skipped = res[LIN_SKIP];   // partitions above LIN_VMAX ops (not checked)
  return 0;
}

extern "C" int paxisim_linearizable(paxisim* h, uint64_t* anomalies, uint64_t* ops, uint64_t* skipped) {
  if (!h) return fail(PAXISIM_EINVAL, "null handle");
  if (h->P.protocol != PAXISIM_ABD || h->P.H == 0)
    return fail(PAXISIM_EUNSUPP, "linearizability scan needs protocol ABD with history > 0");
  return lin_scan<LinAbd>(h, anomalies, ops, skipped);
}

// ---------------------------------------------------------------------------
// Client-side op history of every protocol (include/paxisim.h, DESIGN.md §3.13, chist_kernel.h)
// ---------------------------------------------------------------------------
extern "C" int paxisim_client_history_enable(paxisim* h, uint32_t ops_per_worker) {
  if (!h) return fail(PAXISIM_EINVAL, "null handle");
  if (ops_per_worker == 0 || ops_per_worker > PAXISIM_CLIENT_HISTORY_MAX)
    return fail(PAXISIM_EINVAL, "ops_per_worker must be in [1, %u]", PAXISIM_CLIENT_HISTORY_MAX);
  if (h->P.ch_cap) return fail(PAXISIM_EINVAL, "the client history is already enabled");
  if (h->t) return fail(PAXISIM_EINVAL, "the client history can only be enabled before the first step");
  if (!h->P.lat_bins)
    return fail(PAXISIM_EINVAL, "the client history needs the recording step kernels and their issue stamps: "
                                "call paxisim_latency_enable first");
  if (h->P.protocol != PAXISIM_ABD && !h->P.kv)
    return fail(PAXISIM_EUNSUPP, "replies carry no read values (config.kv = 0)");
  if (const int jrc = enter(h)) return jrc;
  Params P = h->P;
  P.ch_cap = ops_per_worker;
  const size_t cb = sizeof(uint32_t) * P.WK * P.C, ob = sizeof(uint4) * P.WK * P.C * (size_t)ops_per_worker;
  const hipError_t e = alloc_all(h, {new_buf(P.ch_cnt, cb, true), new_buf(P.ch_ops, ob, false)});
  if (e != hipSuccess) return fail(PAXISIM_ENOMEM, "client history buffers (%zu bytes): %s", cb + ob, hipGetErrorString(e));
  h->P = P;
  return 0;
}

// The ops of one cluster, 5 words per op {key, is_write, value, start, end}, workers in index
// order, each in completion order; *dropped_out: the ops past ops_per_worker, counted only.
extern "C" int paxisim_client_history(paxisim* h, uint64_t cluster, uint32_t* buf, uint32_t cap_ops, uint32_t* n_out,
                                      uint32_t* dropped_out) {
  if (!h || !n_out) return fail(PAXISIM_EINVAL, "null argument");
  if (!h->P.ch_cap) return fail(PAXISIM_EINVAL, "the client history is not enabled");
  if (cluster >= h->cfg.clusters) return fail(PAXISIM_ERANGE, "cluster");
  if (const int rc = enter_checked(h)) return rc;   // results only of launches that fully ran
  const Params& P = h->P;
  const uint32_t tot = P.WK * P.ch_cap;
  DevBuf d_ops, d_cnt;
  std::vector<uint4> tmp(tot);
  std::vector<uint32_t> cnt(P.WK);
  HIPCHK(d_ops.alloc<uint4>(tot));
  HIPCHK(d_cnt.alloc<uint32_t>(P.WK));
  chist_read_kernel<<<(tot + 255u) / 256u, 256, 0, h->stream>>>(P, cluster, d_ops.as<uint4>(), d_cnt.as<uint32_t>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(tmp.data(), d_ops.p, tot * sizeof(uint4), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(read_back(h, cnt.data(), d_cnt.p, P.WK * sizeof(uint32_t)));
  uint32_t n = 0, dropped = 0;
  for (uint32_t w = 0; w < P.WK; w++) {
    const uint32_t len = std::min(cnt[w], P.ch_cap);
    dropped += cnt[w] - len;
    for (uint32_t j = 0; j < len; j++, n++) {
      if (!buf || n >= cap_ops) continue;
      const uint4& r = tmp[(size_t)w * P.ch_cap + j];
      uint32_t* o = buf + 5 * (size_t)n;
      o[0] = r.x & 0x7FFFFFFFu;
      o[1] = r.x >> 31;
      o[2] = r.y;
      o[3] = r.z;
      o[4] = r.w;
    }
  }
  *n_out = n;
  if (dropped_out) *dropped_out = dropped;
  return 0;
}

// History.ReadFile (history.go:115-178) into the device history of one worker: literal records.
extern "C" int paxisim_client_history_load(paxisim* h, uint64_t cluster, uint32_t worker, const uint32_t* ops,
                                           uint32_t n) {
  if (!h || (n && !ops)) return fail(PAXISIM_EINVAL, "null argument");
  if (!h->P.ch_cap) return fail(PAXISIM_EINVAL, "the client history is not enabled");
  if (cluster >= h->cfg.clusters || worker >= h->P.WK) return fail(PAXISIM_ERANGE, "bad worker");
  if (n > h->P.ch_cap) return fail(PAXISIM_EINVAL, "%u ops exceed history capacity %u", n, h->P.ch_cap);
  if (const int rc = enter_checked(h)) return rc;   // results only of launches that fully ran
  HIPCHK(hipStreamSynchronize(h->stream));
  const Params& P = h->P;
  std::vector<uint4> tmp(n ? n : 1);
  for (uint32_t j = 0; j < n; j++) {
    const uint32_t* o = ops + 5 * (size_t)j;
    if (o[0] >= P.keys || o[1] > 1u) return fail(PAXISIM_EINVAL, "op %u: bad key (keys = %u) or is_write", j, P.keys);
    tmp[j] = make_uint4(CH_LITERAL | (o[1] ? CH_WRITE : 0u) | o[0], o[2], o[3], o[4]);
  }
  const size_t row = chist_row(P, worker, cluster);
  if (n) HIPCHK(hipMemcpy(&P.ch_ops[row * P.ch_cap], tmp.data(), n * sizeof(uint4), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(&P.ch_cnt[row], &n, 4, hipMemcpyHostToDevice));
  return 0;
}

extern "C" int paxisim_client_linearizable(paxisim* h, uint64_t* anomalies, uint64_t* ops, uint64_t* skipped) {
  if (!h) return fail(PAXISIM_EINVAL, "null handle");
  if (!h->P.ch_cap) return fail(PAXISIM_EINVAL, "the client history is not enabled");
  return lin_scan<LinClient>(h, anomalies, ops, skipped);
}

// ---------------------------------------------------------------------------
// Multi-version Database and Consensus (include/paxisim.h, DESIGN.md §3.14, mv_kernel.h)
// ---------------------------------------------------------------------------
extern "C" int paxisim_multiversion_enable(paxisim* h, uint32_t versions_per_key) {
  if (!h) return fail(PAXISIM_EINVAL, "null handle");
  if (versions_per_key == 0 || versions_per_key > PAXISIM_MV_MAX)
    return fail(PAXISIM_EINVAL, "versions_per_key must be in [1, %u]", PAXISIM_MV_MAX);
  if (h->P.mv_cap) return fail(PAXISIM_EINVAL, "multiversion is already enabled");
  if (h->t) return fail(PAXISIM_EINVAL, "multiversion can only be enabled before the first step");
  if (!h->P.lat_bins)
    return fail(PAXISIM_EINVAL, "multiversion needs the recording step kernels: call paxisim_latency_enable first");
  if (h->P.protocol == PAXISIM_ABD)
    return fail(PAXISIM_EUNSUPP, "ABD's KV is written by versioned Sets, not by Execute of a log: no put order to record");
  if (!h->P.kv) return fail(PAXISIM_EUNSUPP, "replicas keep no Database (config.kv = 0)");
  if (const int jrc = enter(h)) return jrc;
  Params P = h->P;
  P.mv_cap = versions_per_key;
  const size_t rows = (size_t)P.keys * P.N * P.C;
  const size_t cb = sizeof(uint32_t) * rows, vb = cb * versions_per_key;
  const hipError_t e = alloc_all(h, {new_buf(P.mv_cnt, cb, true), new_buf(P.mv_val, vb, false)});
  if (e != hipSuccess) return fail(PAXISIM_ENOMEM, "multiversion buffers (%zu bytes): %s", cb + vb, hipGetErrorString(e));
  h->P = P;
  return 0;
}

// Database.History(key) of one replica: the row is contiguous and indexed by the cluster id, so
// the readout is a copy of the count and one of the kept values.
extern "C" int paxisim_kv_history(paxisim* h, uint64_t cluster, uint32_t replica, uint32_t key, uint32_t* values,
                                  uint32_t cap, uint32_t* n_out, uint32_t* dropped_out) {
  if (!h || !n_out) return fail(PAXISIM_EINVAL, "null argument");
  if (!h->P.mv_cap) return fail(PAXISIM_EINVAL, "multiversion is not enabled");
  if (cluster >= h->cfg.clusters) return fail(PAXISIM_ERANGE, "cluster");
  if (replica >= h->P.N || key >= h->P.keys) return fail(PAXISIM_EINVAL, "no replica %u or key %u", replica, key);
  if (const int rc = enter_checked(h)) return rc;   // results only of launches that fully ran
  const Params& P = h->P;
  const size_t row = mv_row(P, key, replica, cluster);
  uint32_t n = 0;
  HIPCHK(read_back(h, &n, &P.mv_cnt[row], sizeof n));
  const uint32_t kept = std::min(n, P.mv_cap), take = values ? std::min(kept, cap) : 0u;
  if (take) {
    HIPCHK(read_back(h, values, &P.mv_val[row * P.mv_cap], take * sizeof(uint32_t)));
  }
  *n_out = kept;
  if (dropped_out) *dropped_out = n - kept;
  return 0;
}

// client.go:279-320 over clusters [lo, lo + n): totals into tot[MV_NOUT], the failing keys of each
// cluster into masks (either may be null).
static int mv_scan(paxisim* h, uint64_t lo, uint64_t n, uint64_t* tot, uint64_t* masks) {
  if (const int rc = enter_checked(h)) return rc;   // results only of launches that fully ran
  const Params& P = h->P;
  DevBuf d_masks;
  if (masks) {
    HIPCHK(d_masks.alloc<unsigned long long>(n));
    HIPCHK(hipMemsetAsync(d_masks.p, 0, n * sizeof(unsigned long long), h->stream));
  }
  unsigned long long* out = reinterpret_cast<unsigned long long*>(h->d_scratch);
  uint64_t res[MV_NOUT] = {0, 0, 0};
  // a wave per (cluster, key), dealt grid-stride: enough workgroups to fill the device, no more
  const uint64_t pairs = n * P.keys;
  const unsigned grid = (unsigned)std::min<uint64_t>((pairs + MV_WAVES - 1) / MV_WAVES, 8192);
  HIPCHK(hipMemsetAsync(out, 0, sizeof res, h->stream));
  mv_consensus_kernel<<<grid, MV_WAVES * 64, 0, h->stream>>>(P, lo, n, out, d_masks.as<unsigned long long>());
  HIPCHK(hipGetLastError());
  if (masks) HIPCHK(hipMemcpyAsync(masks, d_masks.p, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(read_back(h, res, out, sizeof res));
  if (tot)
    for (int i = 0; i < MV_NOUT; i++) tot[i] = res[i];
  return 0;
}

extern "C" int paxisim_consensus(paxisim* h, uint64_t* failed, uint64_t* versions, uint64_t* dropped) {
  if (!h) return fail(PAXISIM_EINVAL, "null handle");
  if (!h->P.mv_cap) return fail(PAXISIM_EINVAL, "multiversion is not enabled");
  uint64_t tot[MV_NOUT];
  if (const int rc = mv_scan(h, 0, h->cfg.clusters, tot, nullptr)) return rc;
  if (failed) *failed = tot[MV_FAILED];
  if (versions) *versions = tot[MV_VERSIONS];
  if (dropped) *dropped = tot[MV_DROPPED];
  return 0;
}

extern "C" int paxisim_consensus_failed(paxisim* h, uint64_t cluster_lo, uint64_t n, uint64_t* key_masks) {
  if (!h || (n && !key_masks)) return fail(PAXISIM_EINVAL, "null argument");
  if (!h->P.mv_cap) return fail(PAXISIM_EINVAL, "multiversion is not enabled");
  if (cluster_lo > h->cfg.clusters || n > h->cfg.clusters - cluster_lo) return fail(PAXISIM_ERANGE, "cluster range");
  if (n == 0) return 0;
  return mv_scan(h, cluster_lo, n, nullptr, key_masks);
}

// ---------------------------------------------------------------------------
// Message traces of chosen clusters (include/paxisim.h, DESIGN.md §3.15, trace_kernel.h)
// ---------------------------------------------------------------------------
extern "C" int paxisim_trace_enable(paxisim* h, const uint64_t* clusters, uint32_t n_clusters,
                                    uint32_t records_per_replica, uint32_t step_from, uint32_t step_to) {
  if (!h) return fail(PAXISIM_EINVAL, "null handle");
  if (h->P.tr_cap) return fail(PAXISIM_EINVAL, "tracing is already enabled");
  if (h->t) return fail(PAXISIM_EINVAL, "tracing can only be enabled before the first step");
  if (!h->P.lat_bins)
    return fail(PAXISIM_EINVAL, "tracing needs the recording step kernels: call paxisim_latency_enable first");
  if (n_clusters == 0 || n_clusters > PAXISIM_TRACE_MAX_CLUSTERS || !clusters)
    return fail(PAXISIM_EINVAL, "n_clusters must be in [1, %u]", PAXISIM_TRACE_MAX_CLUSTERS);
  if (records_per_replica == 0 || records_per_replica > PAXISIM_TRACE_MAX_RECORDS)
    return fail(PAXISIM_EINVAL, "records_per_replica must be in [1, %u]", PAXISIM_TRACE_MAX_RECORDS);
  if (step_from >= step_to) return fail(PAXISIM_EINVAL, "empty step window [%u, %u)", step_from, step_to);
  std::vector<uint32_t> row(h->P.C, TR_NONE);
  for (uint32_t i = 0; i < n_clusters; i++) {
    if (clusters[i] >= h->cfg.clusters)
      return fail(PAXISIM_ERANGE, "traced cluster %llu outside the handle", (unsigned long long)clusters[i]);
    if (row[clusters[i]] != TR_NONE)
      return fail(PAXISIM_EINVAL, "cluster %llu is listed twice", (unsigned long long)clusters[i]);
    row[clusters[i]] = i;
  }
  if (const int jrc = enter(h)) return jrc;
  Params P = h->P;
  P.tr_cap = records_per_replica;
  P.tr_from = step_from;
  P.tr_to = step_to;
  const size_t rows = (size_t)n_clusters * P.N;
  const size_t tb = sizeof(uint32_t) * row.size(), cb = sizeof(uint32_t) * rows;
  const size_t rb = 2 * sizeof(uint4) * rows * records_per_replica;
  uint32_t* d_row = nullptr;
  const hipError_t e =
      alloc_all(h, {new_buf(d_row, tb, false, row.data()), new_buf(P.tr_cnt, cb, true), new_buf(P.tr_rec, rb, false)});
  if (e != hipSuccess) return fail(PAXISIM_ENOMEM, "trace buffers (%zu bytes): %s", tb + cb + rb, hipGetErrorString(e));
  P.tr_row = d_row;
  h->P = P;
  h->tr_rows = n_clusters;
  h->tr_row.swap(row);
  return 0;
}

// The row is contiguous and found by the cluster id, so the readout is a copy of the count and one
// of the kept slots.
extern "C" int paxisim_trace_read(paxisim* h, uint64_t cluster, uint32_t replica, paxisim_trace_record* out,
                                  uint32_t cap, uint32_t* n_out, uint32_t* dropped_out) {
  if (!h || !n_out) return fail(PAXISIM_EINVAL, "null argument");
  if (!h->P.tr_cap) return fail(PAXISIM_EINVAL, "tracing is not enabled");
  if (cluster >= h->cfg.clusters || h->tr_row[cluster] == TR_NONE)
    return fail(PAXISIM_EINVAL, "cluster %llu is not traced", (unsigned long long)cluster);
  if (replica >= h->P.N) return fail(PAXISIM_EINVAL, "no replica %u", replica);
  if (const int rc = enter_checked(h)) return rc;   // results only of launches that fully ran
  const Params& P = h->P;
  const size_t ri = trace_row(P, h->tr_row[cluster], replica);
  uint32_t n = 0;
  HIPCHK(read_back(h, &n, &P.tr_cnt[ri], sizeof n));
  const uint32_t kept = std::min(n, P.tr_cap), take = out ? std::min(kept, cap) : 0u;
  if (take) {
    std::vector<uint4> tmp(2 * (size_t)take);
    HIPCHK(hipMemcpyAsync(tmp.data(), &P.tr_rec[ri * P.tr_cap * 2], tmp.size() * sizeof(uint4), hipMemcpyDeviceToHost,
                          h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (uint32_t k = 0; k < take; k++) {
      const uint4 &a = tmp[2 * (size_t)k], &m = tmp[2 * (size_t)k + 1];
      out[k] = paxisim_trace_record{a.x, a.y, m.x, m.y, m.z, m.w};
    }
  }
  *n_out = kept;
  if (dropped_out) *dropped_out = n - kept;
  return 0;
}

extern "C" int paxisim_trace_totals(paxisim* h, uint64_t* records, uint64_t* dropped) {
  if (!h) return fail(PAXISIM_EINVAL, "null handle");
  if (!h->P.tr_cap) return fail(PAXISIM_EINVAL, "tracing is not enabled");
  if (const int rc = enter_checked(h)) return rc;   // results only of launches that fully ran
  const Params& P = h->P;
  std::vector<uint32_t> cnt((size_t)h->tr_rows * P.N);
  HIPCHK(read_back(h, cnt.data(), P.tr_cnt, cnt.size() * sizeof(uint32_t)));
  uint64_t kept = 0, lost = 0;
  for (const uint32_t n : cnt) {
    kept += std::min(n, P.tr_cap);
    lost += n - std::min(n, P.tr_cap);
  }
  if (records) *records = kept;
  if (dropped) *dropped = lost;
  return 0;
}

// ---------------------------------------------------------------------------
// Per-cluster verdict words and the search over them (include/paxisim_verdict.h, DESIGN.md §3.17,
// verdict_kernel.h)
// ---------------------------------------------------------------------------
static_assert(LIN_MARK_SKIPPED == PAXISIM_V_LIN_SKIPPED, "lin_kernel.h: the skipped mark is the verdict bit");
static_assert(LIN_VMAX == 16384u, "include/paxisim_verdict.h: the partition size PAXISIM_V_LIN_SKIPPED speaks of");

static uint32_t verdict_bits(const paxisim* h) {
  uint32_t b = PAXISIM_V_FLAGS | PAXISIM_V_QUIET | PAXISIM_V_WAITING | PAXISIM_V_STALLED;
  if (h->P.protocol != PAXISIM_EPAXOS) b |= PAXISIM_V_AGREE;
  if (h->P.mv_cap) b |= PAXISIM_V_CONSENSUS | PAXISIM_V_TRUNCATED;
  if (h->P.protocol == PAXISIM_ABD && h->P.H) b |= PAXISIM_V_LIN | PAXISIM_V_LIN_SKIPPED;
  if (h->P.ch_cap) b |= PAXISIM_V_CLIENT_LIN | PAXISIM_V_LIN_SKIPPED | PAXISIM_V_TRUNCATED;
  return b;
}

// The scans a call asks for: refused before anything is launched.
static int verdict_scans_ok(const paxisim* h, uint32_t scans) {
  if (scans & ~PAXISIM_V_SCANS)
    return fail(PAXISIM_EINVAL, "scans 0x%x: only CONSENSUS, LIN and CLIENT_LIN are scans", scans);
  if ((scans & PAXISIM_V_LIN) && (h->P.protocol != PAXISIM_ABD || h->P.H == 0))
    return fail(PAXISIM_EUNSUPP, "the LIN scan needs protocol ABD with history > 0");
  if ((scans & PAXISIM_V_CLIENT_LIN) && !h->P.ch_cap)
    return fail(PAXISIM_EUNSUPP, "the CLIENT_LIN scan needs paxisim_client_history_enable");
  if ((scans & PAXISIM_V_CONSENSUS) && !h->P.mv_cap)
    return fail(PAXISIM_EUNSUPP, "the CONSENSUS scan needs paxisim_multiversion_enable");
  return 0;
}

// The verdict word of every cluster, evaluated now: words is [clusters] on the device, complete
// when this returns.
static int verdict_eval(paxisim* h, uint32_t scans, DevBuf& words) {
  if (const int rc = quiesce(h)) return rc;
  const Params& P = h->P;
  const uint64_t n = P.clusters;
  DevBuf marks, masks;
  hipError_t e = words.alloc<uint32_t>(n);
  if (e == hipSuccess && (scans & (PAXISIM_V_LIN | PAXISIM_V_CLIENT_LIN))) {
    // (P.C entries: a slot-walking scan marks cl_of[slot], which is below C for every slot)
    e = marks.alloc<uint32_t>(P.C);
    if (e == hipSuccess) e = hipMemsetAsync(marks.p, 0, P.C * sizeof(uint32_t), h->stream);
  }
  if (e == hipSuccess && (scans & PAXISIM_V_CONSENSUS)) {
    e = masks.alloc<unsigned long long>(n);
    if (e == hipSuccess) e = hipMemsetAsync(masks.p, 0, n * sizeof(unsigned long long), h->stream);
  }
  if (e != hipSuccess) return fail(PAXISIM_ENOMEM, "verdict buffers: %s", hipGetErrorString(e));
  if (scans & PAXISIM_V_LIN)
    if (const int rc = lin_scan<LinAbd>(h, nullptr, nullptr, nullptr, marks.as<uint32_t>(), PAXISIM_V_LIN)) return rc;
  if (scans & PAXISIM_V_CLIENT_LIN)
    if (const int rc = lin_scan<LinClient>(h, nullptr, nullptr, nullptr, marks.as<uint32_t>(), PAXISIM_V_CLIENT_LIN))
      return rc;
  if (scans & PAXISIM_V_CONSENSUS) {   // mv_scan's launch, its masks kept on the device
    unsigned long long* out = reinterpret_cast<unsigned long long*>(h->d_scratch);
    const uint64_t pairs = n * P.keys;
    const unsigned grid = (unsigned)std::min<uint64_t>((pairs + MV_WAVES - 1) / MV_WAVES, 8192);
    HIPCHK(hipMemsetAsync(out, 0, MV_NOUT * sizeof(unsigned long long), h->stream));
    mv_consensus_kernel<<<grid, MV_WAVES * 64, 0, h->stream>>>(P, 0, n, out, masks.as<unsigned long long>());
    HIPCHK(hipGetLastError());
  }
  VerdictScans in;
  in.mv_masks = masks.as<unsigned long long>();
  in.marks = marks.as<uint32_t>();
  in.scans = scans;
  in.started = h->t >= h->late_until ? 1u : 0u;
  verdict_kernel<<<(unsigned)((n + 255) / 256), 256, 0, h->stream>>>(P, in, words.as<uint32_t>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));   // the scans' buffers are freed on return
  return 0;
}

// The select over n device words on `stream` (verdict_kernel.h): the matching indices, ascending.
static int select_run(hipStream_t stream, const uint32_t* d_words, uint64_t n, uint32_t any, uint32_t none,
                      uint64_t* ids, uint64_t cap, uint64_t* total) {
  *total = 0;
  if (n == 0) return 0;
  const uint64_t nwg = (n + SEL_WG - 1) / SEL_WG;
  if (nwg > 0x7FFFFFFFull)
    return fail(PAXISIM_ERANGE, "select: %llu words are more than one launch covers", (unsigned long long)n);
  DevBuf offs, out;
  hipError_t e = offs.alloc<unsigned long long>(nwg + 1);
  if (e != hipSuccess) return fail(PAXISIM_ENOMEM, "select offsets: %s", hipGetErrorString(e));
  unsigned long long* d_offs = offs.as<unsigned long long>();
  unsigned long long tot = 0;
  select_count<<<(unsigned)nwg, SEL_WG, 0, stream>>>(d_words, n, any, none, d_offs);
  select_scan<<<1, SEL_SCAN, 0, stream>>>(d_offs, nwg, d_offs + nwg);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(&tot, d_offs + nwg, sizeof tot, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  *total = tot;
  const uint64_t k = std::min<uint64_t>(tot, cap);
  if (k == 0) return 0;
  e = out.alloc<unsigned long long>(k);
  if (e != hipSuccess) return fail(PAXISIM_ENOMEM, "select ids (%llu): %s", (unsigned long long)k, hipGetErrorString(e));
  select_scatter<<<(unsigned)nwg, SEL_WG, 0, stream>>>(d_words, n, any, none, d_offs, out.as<unsigned long long>(), k);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(ids, out.p, k * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  return 0;
}

extern "C" int paxisim_verdict_available(paxisim* h, uint32_t* bits) {
  if (!h || !bits) return fail(PAXISIM_EINVAL, "null argument");
  if (const int rc = quiesce(h)) return rc;
  *bits = verdict_bits(h);
  return 0;
}

extern "C" int paxisim_verdicts(paxisim* h, uint32_t scans, uint64_t lo, uint64_t n, uint32_t* words) {
  if (!h || (n && !words)) return fail(PAXISIM_EINVAL, "null argument");
  if (const int rc = verdict_scans_ok(h, scans)) return rc;
  if (lo > h->cfg.clusters || n > h->cfg.clusters - lo) return fail(PAXISIM_ERANGE, "cluster range");
  if (n == 0) return 0;
  DevBuf d;
  if (const int rc = verdict_eval(h, scans, d)) return rc;
  HIPCHK(read_back(h, words, d.as<uint32_t>() + lo, n * sizeof(uint32_t)));
  return 0;
}

extern "C" int paxisim_find(paxisim* h, uint32_t scans, uint32_t any, uint32_t none, uint64_t* ids, uint64_t cap,
                            uint64_t* total) {
  if (!h || !total || (cap && !ids)) return fail(PAXISIM_EINVAL, "null argument");
  if ((any | none) & ~PAXISIM_V_ALL)
    return fail(PAXISIM_EINVAL, "any 0x%x / none 0x%x: bits outside the defined ones", any, none);
  if (const int rc = verdict_scans_ok(h, scans)) return rc;
  DevBuf d;
  if (const int rc = verdict_eval(h, scans, d)) return rc;
  return select_run(h->stream, d.as<uint32_t>(), h->P.clusters, any, none, ids, cap, total);
}

extern "C" int paxisim_verdict_counts(paxisim* h, uint32_t scans, uint64_t counts[32]) {
  if (!h || !counts) return fail(PAXISIM_EINVAL, "null argument");
  if (const int rc = verdict_scans_ok(h, scans)) return rc;
  DevBuf d, c;
  if (const int rc = verdict_eval(h, scans, d)) return rc;
  const uint64_t n = h->P.clusters;
  const hipError_t e = c.alloc<unsigned long long>(32);
  if (e != hipSuccess) return fail(PAXISIM_ENOMEM, "verdict counts: %s", hipGetErrorString(e));
  HIPCHK(hipMemsetAsync(c.p, 0, 32 * sizeof(unsigned long long), h->stream));
  verdict_count_kernel<<<(unsigned)((n + 255) / 256), 256, 0, h->stream>>>(d.as<uint32_t>(), n,
                                                                         c.as<unsigned long long>());
  HIPCHK(hipGetLastError());
  HIPCHK(read_back(h, counts, c.p, 32 * sizeof(uint64_t)));
  return 0;
}

extern "C" int paxisim_select_words(int device, const uint32_t* words, uint64_t n, uint32_t any, uint32_t none,
                                    uint64_t* ids, uint64_t cap, uint64_t* total) {
  if (!total || (n && !words) || (cap && !ids)) return fail(PAXISIM_EINVAL, "null argument");
  *total = 0;
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(device));
  DevBuf d;
  const hipError_t e = d.alloc<uint32_t>(n);
  if (e != hipSuccess) return fail(PAXISIM_ENOMEM, "select words (%llu): %s", (unsigned long long)n, hipGetErrorString(e));
  HIPCHK(hipMemcpy(d.p, words, n * sizeof(uint32_t), hipMemcpyHostToDevice));
  return select_run(nullptr, d.as<uint32_t>(), n, any, none, ids, cap, total);
}
