// Launch schedule of the MSM device phase (host side, no HIP calls): everything msm.hip's driver decides about a plan - workspace
// layout, which sort runs, every grid and dynamic-LDS size, the fix-up merge, the fold levels and the tail - as integers that the
// driver (msm_device_t) only executes and the CPU test twin (hosttest.hip ht_msm_schedule) can read.
#pragma once
#include "msm_finish.hpp"
#include "msm_plan.hpp"

namespace ncg {

// ---- the sorts (kernels: msm.hip 3, 3b, 3c)
constexpr int SORT2_MAX_RANGES = 256;   // ranges per window: 64, or 128 / 256 where 64 regions would not fit the staged kernel (Sort2::lgr)
constexpr int SORT2_SLICES = 8;
constexpr int SORT2_PER_THREAD = 20;
constexpr int SORT2_STAGE = 1024 * SORT2_PER_THREAD;   // entries: 80 KB of LDS
struct Sort2 {
  int lgr;                // log2(ranges per window): 6..8
  int sh, idxbits;        // log2(buckets per range), bits of an entry index
  int top_w, top_base, top_sh;   // local index of the plan's top window (-1: not in this plan / full), first bucket its ranges cover, its sh
};
constexpr int MSM_SMALL_N = 1 << 15;     // points: 64 KB of LDS digits
constexpr int MSM_SMALL_NB = 1 << 13;    // buckets per window: 32 KB of LDS counters
inline bool msm_small_sort_ok(const MsmPlan& pl) {
  return !pl.endo && !pl.shared && pl.part_flags == 3 && pl.n_layout <= pl.n && pl.n <= MSM_SMALL_N && pl.nb <= MSM_SMALL_NB;
}

// does the two-level form apply to this plan?  Fills the per-plan constants.
inline bool msm_sort2_ok(const MsmPlan& pl, int n_max, Sort2* s2) {
  if (pl.shared || pl.nb < 1024 || pl.nb > (1 << 15)) return false;
  int lg = 0;
  while ((1 << lg) < pl.nb) lg++;
  int ib = 1;
  while (ib < 31 && (1u << ib) < (unsigned)std::max(n_max, 2)) ib++;
  // 64 ranges per window; 128 / 256 where a region would otherwise hold more than 16 384 entries on average (the staged kernel
  // takes up to SORT2_STAGE = 20 480): the 2^21 entries of an endomorphism plan over 2^20 G1 points, plans of 2^21 / 2^22 points
  int lgr = 6;
  while (lgr < 8 && (n_max >> lgr) > 16384 && lg - lgr > 1) lgr++;
  if (ib + 1 + (lg - lgr) > 32) return false;
  s2->lgr = lgr;
  s2->sh = lg - lgr;
  s2->idxbits = ib;
  s2->top_w = -1;
  s2->top_base = 0;
  s2->top_sh = lg - lgr;
  if (!pl.endo && !pl.top_tb) {   // generic plans whose top window is not spread (MsmPlan::top_tb): the top window's field v = (k + H') >> c (nwin - 1) lies in [half, vmax] (H' carries the window's
                    // own half), so its digits v - half are >= 0 and its buckets are [0, vmax - half) only
    const int nwt = pl.nwin_total ? pl.nwin_total : pl.nwin;
    const int wl = nwt - 1 - pl.w0;   // local index of the top window
    if (wl >= 0 && wl < pl.nwin) {
      // the ONE computation of the top field's bound (msm_plan.hpp; ADVICE r05: the sort, the spread and the tail must agree on it).
      // A scalar >= the group order can exceed it: its top digit then wraps through `& (R - 1)` into another region of this window -
      // memory-safe (every region index stays below R), and harmless only because such a call returns the bad-scalar error and
      // its sum is discarded by every caller (k_msm_digits records the index; msm_finish_t / job_finish_host check it first)
      const uint32_t vmax = msm_plan_top_vmax(pl);
      const uint32_t half = 1u << (pl.c - 1);
      const uint32_t span = vmax >= half ? vmax - half + 2u : half;   // buckets the window can reach: largest digit vmax - half, + 1, + 1 of slack (msm_plan_top_spread: maxd + 1)
      int tb = 0;
      while ((1u << tb) < span) tb++;
      if ((1u << tb) < half) {
        s2->top_w = wl;
        s2->top_base = 0;
        s2->top_sh = std::max(0, tb - lgr);
      }
    }
  }
  return true;
}
// words of the scratch the two-level sort keeps where the one-level sort keeps its per-chunk bucket counts
inline size_t msm_sort2_words(const MsmPlan& pl) {
  return (size_t)pl.nwin * ((size_t)pl.Q * SORT2_MAX_RANGES + 2 * (SORT2_MAX_RANGES + 1) + 3) + 8 + (size_t)pl.nwin * pl.nb * SORT2_SLICES;
}

// ---- fix-up, fold and tail (kernels: msm.hip 4, 5, 5b)
// A run longer than MSM_RUN_SERIAL heads goes to the fix-up's work list (k_msm_fixup_merge), which k_msm_fixup_long runs through
// with MSM_LONG_BLOCKS workgroups.
constexpr int MSM_RUN_SERIAL = 2;
constexpr int MSM_RUN_SERIAL_SHARED = 8;
constexpr int MSM_LONG_BLOCKS = 512;
constexpr int MSM_TAIL_THREADS = 512;
// the fix-up merge of the SMALL plans: 2^MERGE_TREE_ULOG units per bucket (two: measured against four and against one unit with the
// work-list threshold at 15, profiles/r06_ab_small_msm.txt; see k_msm_fixup_merge_tree)
constexpr int MERGE_TREE_ULOG = 1;
// k_msm_tail's scratch: MSM_TAIL_REGION accumulators PER WINDOW in each of its two ping-pong regions
constexpr int MSM_TAIL_REGION = 2 * MSM_TAIL_THREADS + 64;
// exchange slots of a cooperative unit (msm_coop.hpp COOP_SLOTS; msm.hip asserts the LDS words of a unit against TailOps)
constexpr int MSM_UNIT_SLOTS = 10;
// a "unit" of the fix-up / fold / tail kernels (TailOps): one item, or a group of four items where the curve has cooperative units
constexpr int msm_unit_shift(const MsmShape& sh, bool coop) { return sh.ls + (coop ? 2 : 0); }
constexpr int msm_unit_scratch_words(const MsmShape& sh, bool coop) { return coop ? MSM_UNIT_SLOTS * (sh.acc_words / 4) : 0; }
constexpr int msm_unit_lds_words(const MsmShape& sh, bool coop) { return msm_unit_scratch_words(sh, coop) + sh.acc_words; }

// ---- workspace layout (byte offsets; every region 256-byte aligned)
struct MsmLayout {
  size_t pts_mont, digits, counts, bucket_start, sorted, sort_tmp, shared_start, buckets, part_pts, part_meta, long_runs, bad, red0, red1, tail0, tail1, fin, total;
};
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// sort2: msm_sort2_ok of the plan (also for plans the one-launch sort takes: their workspace is sized alike); seg: msm_seg's segment
inline MsmLayout msm_layout(const MsmPlan& pl_in, const MsmShape& sh, bool sort2, int seg) {
  MsmLayout L;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    size_t o = off;
    off = align256(off + bytes);
    return o;
  };
  MsmPlan pl = pl_in;
  if (pl.n_layout > pl.n) pl.n = pl.n_layout;  // parts of one MSM: every part addresses the layout of the largest
  if (pl.Q_layout > pl.Q) pl.Q = pl.Q_layout;
  const size_t XW = (size_t)sh.acc_words;
  L.pts_mont = take((pl.endo || pl.pts_stored || pl.shared) ? 0 : (size_t)pl.n * sh.aff_words * 4);  // else: the caller's array
  L.digits = take((size_t)pl.nwin * pl.n * 2);
  L.counts = take(sort2 ? msm_sort2_words(pl) * 4 : (size_t)pl.nwin * pl.Q * pl.nb * 4);
  L.bucket_start = take((size_t)pl.nwin * (pl.nb + 1) * 4);
  L.sorted = take((size_t)pl.nwin * pl.n * 4);
  L.sort_tmp = take(sort2 ? (size_t)pl.nwin * pl.n * 4 : 0);   // the regions of the two-level sort
  L.shared_start = take((size_t)(pl.nb + 1) * 4);
  const MsmPlan av = msm_acc_view(pl);   // one window of nwin * n entries in shared-bucket mode
  L.buckets = take((size_t)av.nwin * av.nb * XW * 4);
  const size_t nseg = (size_t)((av.n + seg - 1) / seg);
  L.part_pts = take((size_t)av.nwin * nseg * 2 * XW * 4);
  L.part_meta = take((size_t)av.nwin * nseg * 4 * 4);
  // work list of the long runs: a counter + (window, bucket, first lane, last lane) per run of more than
  // MSM_RUN_SERIAL heads - such runs cover disjoint lane ranges, so there are at most nwin * nseg / MSM_RUN_SERIAL
  // (with a run_serial override below 2 - tests - adjacent runs share a lane: at most one run per lane)
  L.long_runs = take(16 + ((size_t)av.nwin * (nseg + 1)) * 16);
  L.bad = take(64);
  // fold ping-pong: level l output holds (l+1) * nwin * nb/2^l points <= nwin*nb (l = 1, 2)
  size_t red = (size_t)av.nwin * std::max(av.nb, av.c) * XW * 4;
  L.red0 = take(red);
  L.red1 = take(red);
  // the tail workgroups' private ping-pong (levels that fit one workgroup per window: at most 2 * 512 additions
  // per window and level) and the grouped window sums
  const size_t tail = (size_t)av.nwin * MSM_TAIL_REGION * XW * 4;
  L.tail0 = take(tail);
  L.tail1 = take(tail);
  L.fin = take((size_t)msm_ngroups(av.c) * av.nwin * XW * 4);
  L.total = off;
  return L;
}

// ---- the schedule
enum { MSM_SORT_SMALL, MSM_SORT_TWO_LEVEL, MSM_SORT_ONE_LEVEL };
enum { MSM_MERGE_PLAIN, MSM_MERGE_UNITS, MSM_MERGE_TREE };
struct MsmGrid { unsigned x, y; };
struct MsmFoldLevel {
  long tasks;     // additions and copies of the level, all windows
  int coop;       // k_msm_reduce_level_coop (four items per addition) / k_msm_reduce_level
  unsigned grid;
};
struct MsmSchedule {
  MsmLayout layout;
  MsmPlan av;                // msm_acc_view: the plan the kernels after the sort see
  bool part_first, part_last;
  // points and digits
  bool pts_in_place;         // the caller's array is in storage format already (endomorphism, resident and precomputed plans)
  unsigned pts_grid, digits_grid;
  // sort
  int sort;                  // MSM_SORT_*
  Sort2 s2;                  // two-level sort
  MsmGrid sort_grid;         // the per-(chunk, window) kernels of both counting sorts
  size_t small_lds, hist_lds, scan_lds;
  bool split_totals;
  MsmGrid totals_grid;
  unsigned shared_grid;      // shared totals / starts (shared-bucket plans)
  int scatter_n, scatter_per;   // scatter pass p takes buckets [p * per, min(nb, (p + 1) * per))
  // accumulate and fix-up
  MsmSeg sg;
  MsmGrid acc_grid;
  size_t acc_reserve;        // untouched LDS that pins the grid's placement (MSM_ACC_PIN), 0 = none
  bool acc_sparse;           // the launch holds a spread top window
  int run_serial;            // heads the owner of a cut bucket adds itself: the value the merge kernel runs with and the trace reports
  int merge;                 // MSM_MERGE_*
  MsmGrid merge_grid;
  size_t merge_lds, long_lds;
  // fold and tail
  int nfold;
  MsmFoldLevel fold[16];     // the levels that are launches of their own (c <= 16: at most 15 levels)
  size_t fold_coop_lds;
  int narr, n_in;            // the tail's entry state
  int tail_units;
  size_t tail_lds;
  int ngroups, top_w;
};

inline MsmSchedule msm_schedule(const MsmPlan& pl, const MsmShape& sh) {
  MsmSchedule S;
  S.part_first = (pl.part_flags & 1) != 0;
  S.part_last = (pl.part_flags & 2) != 0;
  S.pts_in_place = pl.endo || pl.pts_stored || pl.shared;
  S.pts_grid = (unsigned)((((size_t)pl.n << sh.ls) + 255) / 256);
  S.digits_grid = (unsigned)((pl.n + 255) / 256);

  // the layout decides on the plan with n = max(n, n_layout), the launch on (plan, max(n, n_layout)): msm_sort2_ok reads n from
  // its argument alone, so the two are one call
  const bool sort2 = msm_sort2_ok(pl, std::max(pl.n, pl.n_layout), &S.s2);
  S.sort = msm_small_sort_ok(pl) ? MSM_SORT_SMALL : sort2 ? MSM_SORT_TWO_LEVEL : MSM_SORT_ONE_LEVEL;   // small: digits + sort + the two clears in one launch (3c)
  S.sort_grid = pl.xcd_map ? MsmGrid{(unsigned)(pl.Q * ((pl.nwin + 7) & ~7)), 1u} : MsmGrid{(unsigned)pl.Q, (unsigned)pl.nwin};
  S.small_lds = (size_t)pl.nb * 4 + (size_t)((pl.n + 1) & ~1) * 2;
  S.hist_lds = (size_t)pl.nb * 4;
  S.scan_lds = (size_t)(pl.nb + pl.nb / 32 + 1) * 4;
  S.split_totals = pl.Q >= 64;
  S.totals_grid = {(unsigned)(S.split_totals ? (pl.nb + 31) / 32 : (pl.nb + 255) / 256), (unsigned)pl.nwin};
  S.shared_grid = (unsigned)((pl.nb + 255) / 256);
  {
    const int passes = std::max(1, std::min(pl.scatter_passes, pl.nb / 256));
    S.scatter_per = (pl.nb + passes - 1) / passes;
    S.scatter_n = (pl.nb + S.scatter_per - 1) / S.scatter_per;   // passes whose range is not empty
  }

  // from here on: the accumulate view (shared-bucket mode: ONE window of nwin * n entries whose starts are shared_start)
  const MsmPlan& av = S.av = msm_acc_view(pl);
  S.sg = msm_seg(av);   // parts of one MSM: the segment is the layout plan's (msm_seg: n_layout), the lanes are this part's
  S.layout = msm_layout(pl, sh, sort2, S.sg.seg);
  S.acc_grid = {(unsigned)((((size_t)S.sg.nseg << sh.ls) + 255) / 256), (unsigned)av.nwin};
  const int pin = msm_acc_pinned((long)S.acc_grid.x * S.acc_grid.y);
  S.acc_reserve = pin ? MSM_ACC_PIN[pin - 1].lds : 0;
  S.top_w = (pl.nwin_total ? pl.nwin_total : pl.nwin) - 1 - pl.w0;
  S.acc_sparse = pl.top_tb && S.top_w >= 0 && S.top_w < pl.nwin;
  if (!pl.top_tb) S.top_w = -1;

  // How many heads the owner of a run adds itself.  A bucket of m entries cut by lanes of `seg` entries has up to
  // ceil(m / seg) heads; m is n / nb on average and rarely above m + 4 sqrt(m).  The seg that fills the chip in one
  // round can be a third of that (verified G1 set of 2^17 points: 64 entries per bucket, seg 20), and with a fixed
  // limit of 2 EVERY bucket went to the work list - 40 000 runs through 512 workgroups, 2.9 ms against 1.0 ms for the
  // generic path.  A serial head costs one dependent addition (3 us); the work list is for real outliers (equal
  // scalars, a short top window).
  const double m_avg = (double)av.n / (double)av.nb;
  const int heads_typ = (int)std::ceil((m_avg + 4.0 * std::sqrt(m_avg) + 1.0) / (double)S.sg.seg);
  const int run_serial_auto = std::max(MSM_RUN_SERIAL, std::min(8, heads_typ));
  const bool rs_forced = pl.run_serial_override >= 0;  // ncg_msm_set_tuning: exactly this many (tests force the work list)
  const int run_serial = rs_forced ? pl.run_serial_override : run_serial_auto;
  // shared-bucket mode: every bucket holds nwin * n / nb entries, i.e. a handful of pieces - all of them, so their
  // owners add them serially (fully parallel over the buckets), as cooperative groups where the curve has them;
  // the work list is for the outliers only
  // ... and the same kernel for per-window plans whose buckets are cut into three or more pieces as a rule (lanes of `seg`
  // entries against buckets of n / nb: the two-window ranks of a window-sharded MSM run seg = 16 against 32-entry buckets):
  // the owner's serial chain of 3-4 single-lane additions (~30 us each on a lone wave) was the longest kernel of such a share
  // after the accumulate itself (138 us of 0.88 ms); four lanes per addition shorten every link of it
  const bool merge_units = (pl.shared || run_serial_auto >= 3) && sh.coop;
  // short segments (plans that do not fill the chip): a tree of 2^MERGE_TREE_ULOG units per bucket, up to 16 pieces
  const bool merge_tree = merge_units && S.sg.seg < 16;
  S.merge = merge_tree ? MSM_MERGE_TREE : merge_units ? MSM_MERGE_UNITS : MSM_MERGE_PLAIN;
  // the threshold the fix-up kernel actually runs with, decided ONCE (the trace reported another value than the launch
  // used for per-window plans on the cooperative-units kernel).  Units: up to 8 pieces per bucket stay with the bucket's own unit
  // (a cooperative addition is ~8 us; the work list costs a launch-wide 120 us as soon as many buckets overflow - the top window
  // of 254-bit scalars holds 64-entry buckets)
  S.run_serial = rs_forced ? run_serial : std::max(run_serial, merge_tree ? 15 : (merge_units || pl.shared) ? MSM_RUN_SERIAL_SHARED : MSM_RUN_SERIAL);
  const int ushift = msm_unit_shift(sh, sh.coop), ulds = msm_unit_lds_words(sh, sh.coop);
  if (S.merge == MSM_MERGE_PLAIN) {
    S.merge_grid = S.acc_grid;
    S.merge_lds = 0;
  } else {
    S.merge_grid = {(unsigned)((((size_t)av.nb << (ushift + (merge_tree ? MERGE_TREE_ULOG : 0))) + 255) / 256), (unsigned)av.nwin};
    S.merge_lds = (size_t)(256 >> ushift) * ulds * 4;
  }
  S.long_lds = (size_t)(MSM_TAIL_THREADS >> ushift) * ulds * 4;

  // fold: nb -> 1 per window in c-1 levels.  Wide levels: one item per addition (throughput); levels that no longer
  // fill the chip: four items per addition (latency, msm_coop.hpp); the last levels + the grouping: k_msm_tail.
  // cooperative form wherever the group offers it and the level fits the resident lanes
  S.tail_units = MSM_TAIL_THREADS >> ushift;
  S.tail_lds = (size_t)S.tail_units * ulds * 4;
  // lanes the chip keeps resident for these kernels (2 waves/SIMD): beyond that the cooperative form costs throughput
  const long coop_max_tasks = (65536L * 2) >> (sh.ls + 2);
  S.fold_coop_lds = (size_t)(256 >> (sh.ls + 2)) * msm_unit_scratch_words(sh, true) * 4;
  // a level that needs more than `tail_rounds` rounds of the tail workgroup's units is a launch of its own: chip-wide it costs
  // 9-13 us, inside the tail 8-12 us PER ROUND (one workgroup per window)
  constexpr int tail_rounds = 1;
  S.nfold = 0;
  S.narr = 1;
  S.n_in = av.nb;
  while (S.n_in > 1 && (long)(S.narr + 1) * (S.n_in >> 1) > (long)tail_rounds * S.tail_units) {
    MsmFoldLevel& lv = S.fold[S.nfold++];
    lv.tasks = (long)(S.narr + 1) * av.nwin * (S.n_in >> 1);
    lv.coop = sh.coop && lv.tasks <= coop_max_tasks;
    lv.grid = (unsigned)(((lv.tasks << (lv.coop ? sh.ls + 2 : sh.ls)) + 255) / 256);
    S.narr++;
    S.n_in >>= 1;
  }
  S.ngroups = msm_ngroups(av.c);
  return S;
}

}  // namespace ncg
