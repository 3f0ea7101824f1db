// Stand-alone check of paxi_amd/csrc/pool_plan.h (built and run by tests/test_pool_plan.py with the
// host compiler's address and undefined-behaviour sanitizers).  Exits non-zero at the first failure.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pool_plan.h"

using namespace pxs;

static int g_fail = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      std::printf("FAIL %s: ", #cond);        \
      std::printf(__VA_ARGS__);               \
      std::printf("\n");                      \
      if (++g_fail > 20) std::exit(1);        \
    }                                         \
  } while (0)

struct Ref {   // one launch of the loop paxisim_step ran before pools
  uint32_t t0, n, K;
  bool compact;
};

// paxisim_step's loop restated directly (one pool: the handle's own t and last_cmp)
static std::vector<Ref> reference(uint32_t& t, uint32_t nsteps, uint32_t S, uint32_t pipe_max, bool compact,
                                  uint32_t cmp_every, uint32_t late_until, uint32_t& last_cmp) {
  std::vector<Ref> out;
  while (nsteps > 0) {
    const uint32_t n = nsteps < S ? nsteps : S;
    uint32_t K = 1;
    if (pipe_max > 1 && n == S) {
      auto due = [&](uint32_t at) { return compact && at >= late_until && at - last_cmp >= cmp_every; };
      while (K < pipe_max && (K + 1u) * n <= nsteps && !due(t + K * n)) K++;
    }
    Ref r{t, n, K, false};
    t += K * n;
    nsteps -= K * n;
    if (compact && t >= late_until && t - last_cmp >= cmp_every) {
      r.compact = true;
      last_cmp = t;
    }
    out.push_back(r);
  }
  return out;
}

struct Shape {
  uint32_t S, pipe_max, cmp_every, late_until;
  bool compact;
};

// one run: the calls in `lens` one after another, for 1 and for 2 pools
static void run(const Shape& sh, const std::vector<uint32_t>& lens, bool aligned) {
  // one pool against the restated loop
  {
    PoolPlanIn in;
    in.S = sh.S; in.pipe_max = sh.pipe_max; in.cmp_every = sh.cmp_every; in.late_until = sh.late_until;
    in.compact = sh.compact; in.npools = 1;
    in.last_cmp[0] = pool_first_cmp(0, sh.S);
    CHECK(in.last_cmp[0] == 0, "pool 0 starts at last_cmp 0");
    uint32_t t = 0, rt = 0, rlast = 0;
    for (uint32_t len : lens) {
      in.t = t; in.nsteps = len;
      const std::vector<PoolLaunch> got = pool_plan(in);
      const std::vector<Ref> want = reference(rt, len, sh.S, sh.pipe_max, sh.compact, sh.cmp_every, sh.late_until, rlast);
      CHECK(got.size() == want.size(), "S=%u call %u at t=%u: %zu launches, loop makes %zu", sh.S, len, t, got.size(),
            want.size());
      for (size_t i = 0; i < got.size() && i < want.size(); i++)
        CHECK(got[i].pool == 0 && got[i].t0 == want[i].t0 && got[i].n == want[i].n && got[i].chunks == want[i].K &&
                  got[i].compact == want[i].compact,
              "S=%u call %u launch %zu: (%u,%u,%u,%d) vs loop (%u,%u,%u,%d)", sh.S, len, i, got[i].t0, got[i].n,
              got[i].chunks, (int)got[i].compact, want[i].t0, want[i].n, want[i].K, (int)want[i].compact);
      t += len;
      CHECK(in.last_cmp[0] == rlast, "last_cmp %u vs loop %u", in.last_cmp[0], rlast);
    }
  }
  // two pools
  PoolPlanIn in;
  in.S = sh.S; in.pipe_max = sh.pipe_max; in.cmp_every = sh.cmp_every; in.late_until = sh.late_until;
  in.compact = sh.compact; in.npools = 2;
  for (uint32_t p = 0; p < 2; p++) in.last_cmp[p] = pool_first_cmp(p, sh.S);
  std::vector<uint32_t> cmp_at[2];
  uint32_t t = 0;
  for (uint32_t len : lens) {
    in.t = t; in.nsteps = len;
    uint32_t last[2] = {in.last_cmp[0], in.last_cmp[1]};
    const std::vector<PoolLaunch> plan = pool_plan(in);
    uint32_t at[2] = {t, t};
    uint32_t prev_t0 = t;
    for (const PoolLaunch& L : plan) {
      CHECK(L.pool < 2, "pool %u", L.pool);
      if (L.pool >= 2) continue;
      const uint32_t p = L.pool;
      CHECK(L.t0 == at[p], "pool %u launch starts at %u, pool is at %u", p, L.t0, at[p]);
      CHECK(L.t0 >= prev_t0, "launches out of start order: %u after %u", L.t0, prev_t0);
      prev_t0 = L.t0;
      CHECK(L.n >= 1 && L.n <= sh.S && L.chunks >= 1, "n=%u chunks=%u", L.n, L.chunks);
      CHECK(L.chunks <= (sh.pipe_max > 1 ? sh.pipe_max : 1u), "%u chunks exceed pipe_max %u", L.chunks, sh.pipe_max);
      CHECK(L.chunks == 1 || L.n == sh.S, "a fused launch of %u-step chunks (S=%u)", L.n, sh.S);
      // no launch crosses a due compaction of its pool: none is due at an inner chunk boundary
      for (uint32_t k = 1; k < L.chunks; k++)
        CHECK(!pool_due(in, p, last[p], L.t0 + k * L.n), "pool %u launch at %u crosses the compaction due at %u", p,
              L.t0, L.t0 + k * L.n);
      at[p] = L.t0 + L.chunks * L.n;
      CHECK(L.compact == pool_due(in, p, last[p], at[p]), "pool %u compaction flag at %u", p, at[p]);
      if (L.compact) {
        CHECK(sh.compact && at[p] >= sh.late_until, "compaction at %u before late_until %u", at[p], sh.late_until);
        last[p] = at[p];
        cmp_at[p].push_back(at[p]);
      }
    }
    t += len;
    for (uint32_t p = 0; p < 2; p++) {
      CHECK(at[p] == t, "pool %u ends the call at %u, not %u", p, at[p], t);
      CHECK(in.last_cmp[p] == last[p], "pool %u last_cmp %u vs %u", p, in.last_cmp[p], last[p]);
    }
  }
  // With every call a whole number of chunks, cmp_every a multiple of S and late_until on a chunk
  // boundary or before the first compaction, a pool's compactions fall every cmp_every steps from its
  // first, and pool 1's first is one chunk after pool 0's: the k-th differ by S.
  if (aligned && sh.compact) {
    const size_t n = cmp_at[0].size() < cmp_at[1].size() ? cmp_at[0].size() : cmp_at[1].size();
    for (size_t k = 0; k < n; k++)
      CHECK(cmp_at[1][k] == cmp_at[0][k] + sh.S, "S=%u cmp_every=%u late=%u: compaction %zu at %u and %u", sh.S,
            sh.cmp_every, sh.late_until, k, cmp_at[0][k], cmp_at[1][k]);
    CHECK(cmp_at[0].size() - n <= 1, "pool 0 compacted %zu times, pool 1 %zu", cmp_at[0].size(), cmp_at[1].size());
  }
}

int main() {
  // the headline shape (config 2): 20-step chunks, up to 4 per launch, compaction every 60, calls of 400
  const Shape c2{20, 4, 60, 1, true};
  run(c2, std::vector<uint32_t>(30, 400), true);
  {
    PoolPlanIn in;
    in.S = 20; in.pipe_max = 4; in.cmp_every = 60; in.late_until = 1; in.compact = true; in.npools = 2;
    in.last_cmp[1] = pool_first_cmp(1, 20);
    in.t = 0; in.nsteps = 400;
    const std::vector<PoolLaunch> plan = pool_plan(in);
    // pool 0: 6 launches of 3 chunks and one of 2; pool 1: one of 4, five of 3, one of 1
    CHECK(plan.size() == 14, "config-2 call: %zu launches", plan.size());
    CHECK(plan[0].pool == 0 && plan[0].chunks == 3 && plan[0].compact, "first launch");
    CHECK(plan[1].pool == 1 && plan[1].chunks == 4 && plan[1].compact, "second launch");
    CHECK(in.last_cmp[0] == 360 && in.last_cmp[1] == 380, "last_cmp %u %u", in.last_cmp[0], in.last_cmp[1]);
  }
  const uint32_t Ss[] = {1, 8, 20, 25};
  const uint32_t pipes[] = {1, 2, 3, 4, 7};
  const uint32_t lates[] = {0, 1, 40, 100, 333};
  const std::vector<std::vector<uint32_t>> odd = {
      {1, 19, 61, 137}, {137, 137, 137}, {61, 1, 1, 400, 19}, {19, 19, 19, 19, 19, 19}, {400, 61, 400, 137, 1}};
  for (uint32_t S : Ss)
    for (uint32_t pm : pipes)
      for (uint32_t late : lates)
        for (int comp = 0; comp < 2; comp++) {
          const uint32_t every[] = {(pm < 3 ? pm : 3) * S, 2 * S, 5 * S, 16, 50, 1};
          for (uint32_t ce : every) {
            const Shape sh{S, pm, ce, late, comp != 0};
            for (const auto& lens : odd) run(sh, lens, false);
            // whole-chunk calls: the offset of one chunk holds when cmp_every is a whole number of
            // chunks and late_until does not land between the pools' first compactions off a boundary
            const bool aligned = ce % S == 0 && late % S == 0;
            run(sh, std::vector<uint32_t>(12, 20 * S), aligned);
            run(sh, {3 * S, 7 * S, S, 20 * S, 2 * S, 11 * S}, aligned);
          }
        }
  // region split: a multiple of 8 tiles nearest the middle; none when a region would be empty
  CHECK(pool_split_tile(1, 64) == 0, "one tile");
  CHECK(pool_split_tile(10, 581) == 8, "581 clusters");
  CHECK(pool_split_tile(33, 2085) == 16, "2085 clusters");
  CHECK(pool_split_tile(17, 1033) == 8, "1033 clusters");
  CHECK(pool_split_tile(16384, 1u << 20) == 8192, "config 2");
  CHECK(pool_split_tile(8, 512) == 0, "512 clusters: region 1 would be empty");
  CHECK(pool_split_tile(9, 513) == 8, "513 clusters");
  for (uint32_t tiles = 1; tiles < 300; tiles++) {
    const uint32_t s = pool_split_tile(tiles, (uint64_t)tiles * 64);
    CHECK(s % 8 == 0 && s < tiles, "split %u of %u tiles", s, tiles);
    if (s) CHECK(2 * s + 8 >= tiles && 2 * s <= tiles + 8, "split %u of %u tiles is not near the middle", s, tiles);
  }
  // kernel-time union
  CHECK(interval_union({}) == 0.0, "empty union");
  CHECK(interval_union({{0, 2}, {1, 3}, {5, 6}}) == 4.0, "overlap and gap");
  CHECK(interval_union({{5, 6}, {-1, 1}, {0, 0.5}}) == 3.0, "unsorted, nested, negative start");
  CHECK(interval_union({{0, 1}, {1, 2}}) == 2.0, "touching");
  if (g_fail) return 1;
  std::printf("pool_plan OK\n");
  return 0;
}
