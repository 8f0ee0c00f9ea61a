// vsx_plan.cpp -- host side of libvsx, the planner: pairs -> wavefront tasks of one kernel class each -> direction-buffer chunks
// (vsx_plan_create, a driver over named stages), and what runs a plan (vsx_plan_run, vsx_plan_sync, vsx_plan_describe).
// See vsx_context.cpp for the layout of the host layer.
#include "vsx_host_internal.h"

#include <cinttypes>
#include <utility>

using vsxp::fail;
using namespace vsxh;

// r05j same-box A/B, 25 000 queries x 32 candidates, two runs each (profiles/r05/r05j_pairprof_first_contact.txt): DP 400 x 400 16.53 -> 14.45 ms,
// 300 x 300 9.96 -> 8.68, 250 x 1000 22.12 -> 20.39, 150 x 1000 16.04 -> 14.50.  Default ON (it engages only where a query has >= 4 eligible tasks)
#ifndef VSX_PAIRPROF_DEFAULT
#define VSX_PAIRPROF_DEFAULT 1
#endif
// Can any H/E/F value of a (Q x D) alignment reach the 16-bit limits?  With all 12 penalties >= 0,
//   B = max(|match|, |mismatch|, every gap extension), G = max(every gap open):
//   every H, E, F, border and intermediate of onestep lies in [-(3G + (Q+Dp+4)B) - (G+B), min(Q,Dp)*B]
//   (lower bound: the pure-extension chains E(i,j) >= E(i,0) - jB, F(i,j) >= F(0,j) - iB from the borders
//   -(go + k*ge); upper bound: <= one match per diagonal step).  If that interval is inside
//   (SHRT_MIN + max(go+ge), SHRT_MAX), no saturation occurs and the reference's overflow rule
//   (align_simd.cpp:1432-1444, :1774-1786) can never fire, so the kernel may skip the min/max tracking.
static bool no_overflow_possible(const vsx_ctx * ctx, int64_t Q, int64_t D)
{
  int64_t B = std::max<int64_t>(std::llabs(ctx->P.match), std::llabs(ctx->P.mismatch));
  int64_t G = 0;
  for (int k = 0; k < 12; ++k)
    {
      if (ctx->pen[k] < 0) return false;
      if (k < 6) G = std::max<int64_t>(G, ctx->pen[k]); else B = std::max<int64_t>(B, ctx->pen[k]);
    }
  // TOPPAD dummy rows (above query row 0) run the interior recurrence; a horizontal gap opened inside them must never beat the
  // true top border H(-1, j) = -(go_ql + j ge_ql): after n columns it has lost QR_q(interior) + (n - 1) R_q(interior) against
  // the border's n ge_ql, so both QR_q(interior) >= ge_ql and R_q(interior) >= ge_ql are needed (found by oracle/soak.py: with
  // ge_ql = 5 > ge_qi = 4 a 77-column terminal gap was priced through the dummy rows)
  if (ctx->pen[2] + ctx->pen[8] < ctx->pen[6] || ctx->pen[8] < ctx->pen[6]) return false;
  const int64_t Dp = (D + 3) & ~3ll;
  return 4 * G + (Q + Dp + 16) * B < 32000;
}

// The TILT class (vsx_forward_kernel): every value is shifted by (i + j) g with -R - 2 <= i < Q, -1 <= j < Dp + 16 and g <= B,
// scores grow by 2g: the interval of no_overflow_possible() widened by that shift must still fit.
// Returns 0 (not admitted), 1 (TILT: values biased by 0x8000 into unsigned 16 bits) or 2 (the MAX3 sub-class: the same bound
// must hold for HALF the range -- values biased by 0x3E00 have to stay inside [0, 0x7BFF], the finite non-negative fp16 patterns,
// for v_pk_maximum3_f16 to be an integer maximum; vsx_forward_kernel MAX3).  VSX_MAX3=0 switches the sub-class off (A/B, tests).
static int tilt_possible(const vsx_ctx * ctx, int64_t Q, int64_t D)
{
  if (ctx->Pt.tilt == 0) return 0;
  static const bool max3_off = std::getenv("VSX_MAX3") && std::strcmp(std::getenv("VSX_MAX3"), "0") == 0;
  int64_t B = std::max<int64_t>(std::llabs(ctx->P.match), std::llabs(ctx->P.mismatch));
  int64_t G = 0;
  for (int k = 0; k < 12; ++k)
    if (k < 6) G = std::max<int64_t>(G, ctx->pen[k]); else B = std::max<int64_t>(B, ctx->pen[k]);
  const int64_t Dp = (D + 3) & ~3ll;
  const int64_t reach = 4 * G + 2 * (Q + Dp + 64) * B;          // |value| of anything the kernel forms stays below this
  // (pen[4] = the query's right-end gap open: the MAX3 kernel's interior steps read "the last row continues to the left" off ext-left
  //  alone, which covers "left" only when that penalty is positive -- vsx_forward_kernel LASTFAST; the reference's default is 1)
  if (reach < 15800 && !max3_off && ctx->pen[4] > 0 &&
      ctx->device < 64 && g_max3_state[ctx->device].load(std::memory_order_relaxed) == 1) return 2;         // 0x3E00 = 15872 each way inside [0, 0x7BFF]
  return reach < 32000 ? 1 : 0;
}

int vsxh::pick_rows(int Q)
{
  static const int forced = std::getenv("VSX_ROWS") ? std::atoi(std::getenv("VSX_ROWS")) : 0;      // A/B experiments: rows per lane
  if (forced > 0 && Q >= forced) return forced;
  int cnt = 0;
  const int * rows = vsx_supported_rows(&cnt);
  int idx = cnt - 1;
  for (int k = 0; k < cnt; ++k)
    if (16 * rows[k] >= Q) { idx = k; break; }
  // a single, partially filled pipeline position would put the last query row at r != R-1
  while (idx > 0 && Q < rows[idx]) --idx;
  return rows[idx];
}

// ---- vsx_plan_create: a driver over one function per stage.  A stage that fails has set the error; the plan, held by the driver,
// ---- then gives back its slot, cursor and events (~vsx_plan)

namespace {

struct ProtoTask : KernelClass { uint32_t q; uint32_t n; uint32_t pair[8]; };
struct ClassCount { KernelClass cls; size_t count; };

// what the stages hand on
struct PlanDraft {
  std::vector<uint32_t> gpu_pairs;                     // the pairs that need the DP; from group_by_query on: by query, targets longest first
  std::vector<std::vector<ProtoTask>> part;            // group_by_query -> mark_pair_groups: the tasks of each host thread's queries ...
  std::vector<std::vector<std::pair<size_t, size_t>>> pair_cand;      // ... and in them the [first, end) task ranges of queries that may form PAIR groups
  std::vector<ProtoTask> protos;                       // every task, from sort_by_class on in launch order
  uint64_t budget_dwords = 0;                          // checkpoint dwords a chunk may use
  std::vector<uint64_t> t_dwords, t_slab, t_pair0;     // per task: checkpoint dwords; slab words, then first slab word; first pair of the plan's order
  double t_classify = 0, t_group = 0, t_budget = 0, t_tasks = 0, t_device = 0;      // the phases of the VSX_DEBUG_TIMING line (seconds)
};

// r05, sparse tasks: a task of <= 2 (<= 4) targets of the TILT family shares its wave with three (one) other tasks of its class
// (vsx_forward_kernel NQ) instead of leaving three (two) of the four lane groups idle.  VSX_SPARSE=0: every task is a wave (A/B, tests)
bool sparse_enabled()
{
  static const bool sparse_on = !(std::getenv("VSX_SPARSE") && std::strcmp(std::getenv("VSX_SPARSE"), "0") == 0);
  return sparse_on;
}

bool targets_pure(const ProtoTask & pt, const vsx_seqset * targets, const uint32_t * tidx)
{
  bool pure = true;
  for (uint32_t sidx = 0; sidx < pt.n && pure; ++sidx) pure = !targets->impure[tidx[pt.pair[sidx]]];
  return pure;
}

// the classes of the tasks `take` admits and how many tasks each has, in first-seen order
template <typename Take>
std::vector<ClassCount> count_by_class(const std::vector<ProtoTask> & protos, Take take)
{
  std::vector<ClassCount> cls;
  for (const ProtoTask & pt : protos)
    {
      if (!take(pt)) continue;
      bool found = false;
      for (ClassCount & c : cls) if (c.cls == pt.cls()) { ++c.count; found = true; break; }
      if (!found) cls.push_back(ClassCount {pt.cls(), 1});
    }
  return cls;
}

int validate_pairs(const vsx_seqset * queries, const vsx_seqset * targets, uint64_t n_pairs, const uint32_t * qidx, const uint32_t * tidx)
{
  const int nthc = pass_threads(n_pairs, 32768);
  std::vector<uint64_t> bad((size_t) nthc, UINT64_MAX);
  auto check = [&](int t) {
    const auto [lo, hi] = slice_of(n_pairs, t, nthc);
    for (uint64_t k = lo; k < hi; ++k)
      if (qidx[k] >= queries->n || tidx[k] >= targets->n) { bad[(size_t) t] = k; return; }
  };
  run_threads(nthc, check);
  for (int t = 0; t < nthc; ++t)
    if (bad[(size_t) t] != UINT64_MAX)
      return fail(VSX_EINVAL, "vsx_plan_create: pair %" PRIu64 " references a sequence out of range", bad[(size_t) t]);
  return VSX_OK;
}

// r06: a block nobody uses, the LARGEST such -- plans that follow one another (the stages of a clustering round, of a search window:
// each is destroyed, i.e. its traceback has finished, before the next is made) then keep ONE block warm instead of growing three in
// turn: 2 M x 300 bp --cluster_fast spent 1.1 s of its 6-7 s in eight multi-GB hipMallocs (profiles/r06/r06e_cluster_blocks.txt).
// A pipeline of slices (vsx_align_pairs) finds the earlier plans' blocks taken and so still alternates; when all are taken, the one
// acquired longest ago (its traceback finishes first).
void acquire_dir_slot(vsx_ctx * ctx, vsx_plan & pl)
{
  std::lock_guard<std::mutex> lk(ctx->slot_mu);
  const unsigned seq = ctx->plan_seq.fetch_add(1);
  int pick = -1;
  for (int k = 0; k < 3; ++k)
    if (ctx->slot_refs[k] == 0 && (pick < 0 || ctx->shared_dir[k].bytes() > ctx->shared_dir[pick].bytes())) pick = k;
  if (pick < 0)
    for (int k = 0; k < 3; ++k)
      if (pick < 0 || (int) (seq - ctx->slot_stamp[k]) > (int) (seq - ctx->slot_stamp[pick])) pick = k;
  ++ctx->slot_refs[pick];
  ctx->slot_stamp[pick] = seq;
  pl.dir_slot = pick;
  pl.slot_held = true;
}

// ---- the reference's closed-form / sentinel cases (no DP) ----
// host threads classify contiguous slices: the common case (a pair for the GPU) is handled in place, the rare closed-form
// pairs are collected per slice and answered serially below (they append to shared CIGAR lists, in pair order)
void classify_pairs(const vsx_ctx * ctx, const vsx_seqset * queries, const vsx_seqset * targets, uint64_t n_pairs,
                    const uint32_t * qidx, const uint32_t * tidx, PlanDraft & d, vsx_plan & pl)
{
  const int nthc = pass_threads(n_pairs, 32768);
  std::vector<uint32_t> & gpu_pairs = d.gpu_pairs;
  std::vector<std::vector<uint32_t>> gp((size_t) nthc), special((size_t) nthc);
  std::vector<uint64_t> pcells((size_t) nthc, 0);
  auto classify = [&](int t) {
    const auto [lo, hi] = slice_of(n_pairs, t, nthc);
    gp[(size_t) t].reserve(hi - lo);
    uint64_t cells = 0;
    for (uint64_t k = lo; k < hi; ++k)
      {
        const int64_t Q = queries->len[qidx[k]], D = targets->len[tidx[k]];
        if (ctx->force_fallback || Q == 0 || D == 0 || !fits(Q, D)) { special[(size_t) t].push_back((uint32_t) k); continue; }
        gp[(size_t) t].push_back((uint32_t) k);
        cells += (uint64_t) Q * (uint64_t) D;
      }
    pcells[(size_t) t] = cells;
  };
  run_threads(nthc, classify);
  size_t total = 0;
  for (auto & v : gp) total += v.size();
  gpu_pairs.resize(total);
  {
    std::vector<size_t> base((size_t) nthc);
    size_t acc = 0;
    for (int t = 0; t < nthc; ++t) { base[(size_t) t] = acc; acc += gp[(size_t) t].size(); pl.cells += pcells[(size_t) t]; }
    auto place = [&](int t) { if (!gp[(size_t) t].empty()) std::memcpy(gpu_pairs.data() + base[(size_t) t], gp[(size_t) t].data(), gp[(size_t) t].size() * 4); };
    run_threads(nthc, place);
  }
  for (int t = 0; t < nthc; ++t)
    for (uint32_t k : special[(size_t) t])
      {
        const int64_t Q = queries->len[qidx[k]], D = targets->len[tidx[k]];
        pl.host_pairs.push_back(k);
        pl.host_out.emplace_back();
        VsxPairOut & o = pl.host_out.back();
        auto sentinel = [&]() { o = VsxPairOut {}; o.score = 32767; };
        if (ctx->force_fallback) { sentinel(); continue; }              // align_simd.cpp:1463-1479
        if (Q == 0)                                                      // :1481-1539
          {
            if (!fits(0, D)) { sentinel(); continue; }
            o = VsxPairOut {};
            o.aligned = (uint16_t) D; o.gaps = (uint16_t) D;
            if (D > 0)
              {
                const int64_t a = -(int64_t) ctx->pen[1] - D * (int64_t) ctx->pen[7];
                const int64_t b = -(int64_t) ctx->pen[5] - D * (int64_t) ctx->pen[11];
                o.score = (int16_t) (uint16_t) (std::max(a, b) & 0xffff);   // plain narrowing cast :1515
                pl.host_cigar.push_back(std::to_string(D) + "I");
                pl.host_cigar_pair.push_back(k);
                pl.host_cigar_run.push_back(((uint32_t) D << 2) | 1u);
              }
            continue;
          }
        sentinel();                                                      // D == 0 or the size guard (:1867-1882)
      }
}

// ---- group by query -> tasks of <= 8 targets, similar lengths together (host threads over query groups) ----
void group_by_query(const vsx_ctx * ctx, const vsx_seqset * queries, const vsx_seqset * targets, uint64_t n_pairs,
                    const uint32_t * qidx, const uint32_t * tidx, PlanDraft & d)
{
  // r05, pair-profile classes (vsx_forward_kernel PAIR): groups of four whole-wave tasks of ONE pure-ACGT query with pure-ACGT targets
  // run as a workgroup that shares a pair-indexed dword profile (5 instead of 6 instructions per lane-row).  Worth it only for queries
  // with many targets (--allpairs_global); needs the purity of both sets.  VSX_PAIRPROF=0 / 1 overrides the default below
  // (r06, ADVICE r05: the purity of the two sets is asked for only once the grouping below has found a query with four whole-wave tasks --
  //  a search's windows never have one, and every new query set used to pay a purity pass with a device-wide synchronisation)
  static const bool pair_env = std::getenv("VSX_PAIRPROF") ? std::strcmp(std::getenv("VSX_PAIRPROF"), "0") != 0 : (VSX_PAIRPROF_DEFAULT != 0);
  const bool pair_try = pair_env && n_pairs >= 32;
  const bool sparse_on = sparse_enabled();
  std::vector<uint32_t> & gpu_pairs = d.gpu_pairs;
  auto by_query = [&](uint32_t a, uint32_t b) { return qidx[a] < qidx[b]; };
  if (!std::is_sorted(gpu_pairs.begin(), gpu_pairs.end(), by_query)) std::stable_sort(gpu_pairs.begin(), gpu_pairs.end(), by_query);
  std::vector<size_t> group_begin;                       // start of every query's run in gpu_pairs, plus the end
  for (size_t b = 0; b < gpu_pairs.size();)
    {
      group_begin.push_back(b);
      const uint32_t q = qidx[gpu_pairs[b]];
      size_t e = b;
      while (e < gpu_pairs.size() && qidx[gpu_pairs[e]] == q) ++e;
      b = e;
    }
  group_begin.push_back(gpu_pairs.size());
  const size_t ngroups = group_begin.size() - 1;
  const int nth = pass_threads(gpu_pairs.size(), 16384);
  d.part.resize((size_t) nth);
  d.pair_cand.resize((size_t) nth);
  auto work = [&](int t) {
    // contiguous ranges of groups with about the same number of pairs
    const auto [p_lo, p_hi] = slice_of(gpu_pairs.size(), t, nth);
    const size_t g_lo = (size_t) (std::lower_bound(group_begin.begin(), group_begin.end() - 1, p_lo) - group_begin.begin());
    const size_t g_hi = (t == nth - 1) ? ngroups : (size_t) (std::lower_bound(group_begin.begin(), group_begin.end() - 1, p_hi) - group_begin.begin());
    std::vector<ProtoTask> & outp = d.part[(size_t) t];
    for (size_t g = g_lo; g < g_hi; ++g)
      {
        const size_t b = group_begin[g], e = group_begin[g + 1];
        const uint32_t q = qidx[gpu_pairs[b]];
        std::stable_sort(gpu_pairs.begin() + (long) b, gpu_pairs.begin() + (long) e,
                         [&](uint32_t x, uint32_t y) { return targets->len[tidx[x]] > targets->len[tidx[y]]; });
        const int rows = pick_rows((int) queries->len[q]);
        const size_t first_of_query = outp.size();
        for (size_t x = b; x < e; x += VSX_TASK_SLOTS)
          {
            ProtoTask pt {};
            pt.q = q; pt.rows = rows;
            pt.n = (uint32_t) std::min<size_t>(VSX_TASK_SLOTS, e - x);
            uint32_t dmax = 0;
            for (uint32_t sidx = 0; sidx < pt.n; ++sidx)
              {
                pt.pair[sidx] = gpu_pairs[x + sidx];
                dmax = std::max(dmax, targets->len[tidx[pt.pair[sidx]]]);
              }
            pt.track = (!ctx->tb_packed && no_overflow_possible(ctx, queries->len[q], dmax)) ? 0 : 1;
            pt.tilt = (pt.track == 0) ? tilt_possible(ctx, queries->len[q], dmax) : 0;
            pt.nq = 1;
            if (sparse_on && pt.tilt && rows >= 4 && pt.n <= 4 && (int64_t) queries->len[q] <= 16ll * rows)      // (one strip: the hand-over rows are per wave)
              pt.nq = pt.n <= 2 ? 4 : 2;
            outp.push_back(pt);
          }
        if (pair_try && rows >= 4 && outp.size() - first_of_query >= 4 && (int64_t) queries->len[q] <= 16ll * rows)     // (one strip: the PAIR kernels are ONE variants)
          {
            size_t eligible = 0;
            for (size_t k = first_of_query; k < outp.size(); ++k) eligible += (outp[k].nq == 1 && outp[k].tilt) ? 1 : 0;
            if (eligible >= 4) d.pair_cand[(size_t) t].emplace_back(first_of_query, outp.size());
          }
      }
  };
  run_threads(nth, work);
}

// the PAIR groups among the candidates of group_by_query (needs the purity of both sets); then the threads' tasks become one list
int mark_pair_groups(const vsx_seqset * queries, const vsx_seqset * targets, const uint32_t * tidx, PlanDraft & d)
{
  bool any_pair_cand = false;
  for (const auto & v : d.pair_cand) any_pair_cand = any_pair_cand || !v.empty();
  if (any_pair_cand)
    {
      int rc = ensure_impure(queries);
      if (rc == VSX_OK) rc = ensure_impure(targets);
      if (rc != VSX_OK) return rc;
    }
  auto mark_pairs = [&](int t) {
    std::vector<ProtoTask> & outp = d.part[(size_t) t];
    for (const std::pair<size_t, size_t> & range : d.pair_cand[(size_t) t])
      {
        const size_t first_of_query = range.first, end_of_query = range.second;
        if (queries->impure[outp[first_of_query].q]) continue;
        // whole groups of four eligible tasks of this query (same kernel class, every target plain ACGT) -> nq = 8; what is left over
        // stays in the whole-wave class.  The tasks of a query are consecutive and stay so through the stable class sort below.
        std::vector<size_t> ok;
        for (size_t k = first_of_query; k < end_of_query; ++k)
          {
            const ProtoTask & pt = outp[k];
            if (pt.nq != 1 || !pt.tilt) continue;
            if (targets_pure(pt, targets, tidx)) ok.push_back(k);
          }
        // (groups must not mix the MAX3 and the 16-bit TILT sub-class: take runs of equal tilt)
        size_t i0 = 0;
        while (i0 < ok.size())
          {
            size_t i1 = i0;
            while (i1 < ok.size() && outp[ok[i1]].tilt == outp[ok[i0]].tilt) ++i1;
            const size_t whole = (i1 - i0) / 4 * 4;
            for (size_t k = i0; k < i0 + whole; ++k) outp[ok[k]].nq = 8;
            i0 = i1;
          }
      }
  };
  if (any_pair_cand) run_threads((int) d.part.size(), mark_pairs);
  size_t total = 0;
  for (auto & v : d.part) total += v.size();
  d.protos.reserve(total);
  for (auto & v : d.part) d.protos.insert(d.protos.end(), v.begin(), v.end());
  return VSX_OK;
}

// r04: a class with a handful of tasks still costs a launch of each kernel on the plan's streams, and a one-wave launch is a pure
// latency chain (profiles/r04/r04z_shape_300x300_summary.txt: four tasks with 18 rows per lane beside 99 996 with 20 -- queries a few
// symbols short of 289 -- took 0.15 ms of DP and 0.61 ms of traceback, 11 % of the step's traceback time).  Any row count with
// 16 R >= Q is valid for a query, so the tasks of a sparse class join the next denser class of the same kind.
void merge_thin_row_classes(const vsx_seqset * queries, PlanDraft & d)
{
  const std::vector<ClassCount> cls = count_by_class(d.protos, [](const ProtoTask &) { return true; });
  std::vector<std::pair<size_t, int>> move;                                 // class index -> new rows
  for (size_t a = 0; a < cls.size(); ++a)
    {
      int best = 0;
      for (const ClassCount & c : cls)
        if (c.cls.same_but_rows(cls[a].cls) && c.cls.rows > cls[a].cls.rows &&
            c.count >= 32 * cls[a].count && (best == 0 || c.cls.rows < best))
          best = c.cls.rows;
      if (best && cls[a].count < 4096) move.emplace_back(a, best);
    }
  for (auto & mv : move)                                                    // (a target class that moves itself takes its newcomers along)
    for (int hop = 0; hop < 4; ++hop)
      for (const auto & other : move)
        {
          const KernelClass & a = cls[mv.first].cls, & o = cls[other.first].cls;
          if (o.rows == mv.second && o.same_but_rows(a)) { mv.second = other.second; break; }
        }
  if (!move.empty())
    for (ProtoTask & pt : d.protos)
      for (const auto & mv : move)
        if (pt.cls() == cls[mv.first].cls)
          {
            // (only queries that still span two pipeline positions: a query shorter than one position of the new class would make
            //  position 0 the last position as well, a shape no row count chosen by pick_rows() ever produces)
            if ((int) queries->len[pt.q] > mv.second) pt.rows = mv.second;
            break;
          }
}

// a SMALL sparse class is not worth its own launches: below one round of the chip (256 CUs x <= 16 waves) whole-wave tasks already
// have the SIMDs largely to themselves -- packing four of them into one slower wave frees nothing -- and every extra class is one more
// DP launch in the plan's stream (r05c: the speculative alignments of --cluster_fast, ~30 k pairs per round in three classes, ran
// 0.44 -> 0.64 s with sparse classes of a few thousand tasks each).  VSX_SPARSE_MIN=n: the smallest class kept (tests: 1)
void demote_small_sparse_classes(PlanDraft & d)
{
  if (!sparse_enabled()) return;
  static const size_t sparse_min = std::getenv("VSX_SPARSE_MIN") ? (size_t) std::atoll(std::getenv("VSX_SPARSE_MIN")) : 4096;
  auto sparse = [](const ProtoTask & pt) { return pt.nq == 2 || pt.nq == 4; };
  const std::vector<ClassCount> ks = count_by_class(d.protos, sparse);
  bool any = false;
  for (const ClassCount & c : ks) any = any || c.count < sparse_min;
  if (any)
    for (ProtoTask & pt : d.protos)
      if (sparse(pt))
        for (const ClassCount & c : ks)
          if (c.count < sparse_min && pt.cls() == c.cls) { pt.nq = 1; break; }
}

// split-profile classes (vsx_forward_kernel SPLIT): a whole-wave single-strip MAX3 task whose TARGETS are all plain A / C / G / T reads
// its scores from two dword tables, LO[sym][row] and HI[sym][row] = score << 16, and adds both to the diagonal in one v_add3_u32 (5
// instead of 6 instructions per lane-row).  Needs the purity of the target set only (once per set).  VSX_SPLITPROF=0 switches it off
//
// What the PAIR groups and the sparse classes left in the whole-wave MAX3 class, single-strip, in a row class
// that has the kernel, every target plain ACGT -> nq = 16.  After the merging of sparse row classes above, so that the byte-profile
// tasks merge exactly as they would without this class and a task that moved to a denser row class joins with its new row count
int mark_split_profile(const vsx_seqset * queries, const vsx_seqset * targets, const uint32_t * tidx, PlanDraft & d)
{
  static const bool split_env = !(std::getenv("VSX_SPLITPROF") && std::strcmp(std::getenv("VSX_SPLITPROF"), "0") == 0);
  if (!split_env) return VSX_OK;
  std::vector<ProtoTask> & protos = d.protos;
  auto split_shape = [&](const ProtoTask & pt) {
    return pt.nq == 1 && pt.tilt == 2 && VSX_SPLIT_ROWS(pt.rows) && (int64_t) queries->len[pt.q] <= 16ll * pt.rows;
  };
  bool any = false;
  for (size_t x = 0; x < protos.size() && !any; ++x) any = split_shape(protos[x]);
  if (!any) return VSX_OK;
  const int rc = ensure_impure(targets);
  if (rc != VSX_OK) return rc;
  const int nts = pass_threads(protos.size(), 4096);
  run_threads(nts, [&](int th) {
    const auto [lo, hi] = slice_of(protos.size(), th, nts);
    for (size_t x = lo; x < hi; ++x)
      if (split_shape(protos[x]) && targets_pure(protos[x], targets, tidx)) protos[x].nq = 16;
  });
  return VSX_OK;
}

// kernel classes together (one launch per class and chunk)
void sort_by_class(PlanDraft & d)
{
  auto by_class = [](const ProtoTask & a, const ProtoTask & b) { return a.cls() < b.cls(); };
  if (!std::is_sorted(d.protos.begin(), d.protos.end(), by_class)) std::stable_sort(d.protos.begin(), d.protos.end(), by_class);
}

// ---- direction-buffer budget ----
int choose_dir_budget(vsx_ctx * ctx, uint64_t dir_budget_bytes, PlanDraft & d, const vsx_plan & pl)
{
  if (dir_budget_bytes == 0)
    {
      size_t free_b = 0, total_b = 0;
      {
        vsxp::Stopwatch sw(d.t_budget);
        VSX_HIP(hipMemGetInfo(&free_b, &total_b));
      }
      free_b += ctx->pool.idle_bytes() + ctx->shared_dir[pl.dir_slot].bytes();   // blocks this context can hand straight back / already holds
      dir_budget_bytes = std::min<uint64_t>((uint64_t) (free_b * 0.4), 128ull << 30);
      // stay inside the context's current checkpoint block unless it is less than half of what could be had: a slightly
      // larger request would cost another multi-second hipMalloc
      const uint64_t have = ctx->shared_dir[pl.dir_slot].bytes();
      if (have >= dir_budget_bytes / 2) dir_budget_bytes = have;
    }
  d.budget_dwords = std::max<uint64_t>(dir_budget_bytes / 4, 1);
  return VSX_OK;
}

// tasks: (1) host threads fill the descriptors and sizes, (2) a serial scan assigns checkpoint / strip / slab offsets and cuts
// chunks and launches, (3) host threads write the per-pair tables.  (1) and (3) are bound by random reads of the sequence
// tables; the scan touches 3 numbers per task.
void fill_task_descriptors(const vsx_seqset * queries, const vsx_seqset * targets, const uint32_t * tidx, PlanDraft & d, vsx_plan & pl)
{
  const std::vector<ProtoTask> & protos = d.protos;
  const size_t NT = protos.size();
  pl.tasks.resize(NT);
  pl.pair_slot.resize(d.gpu_pairs.size());
  pl.pair_ids.resize(d.gpu_pairs.size());
  pl.slab_off.resize(d.gpu_pairs.size());
  d.t_dwords.resize(NT); d.t_slab.resize(NT); d.t_pair0.resize(NT);
  const int ntt = pass_threads(NT, 4096);
  run_threads(ntt, [&](int th) {
    const auto [lo, hi] = slice_of(NT, th, ntt);
    for (size_t x = lo; x < hi; ++x)
      {
        const ProtoTask & pt = protos[x];
        VsxTask t {};
        t.qoff = queries->off[pt.q];
        t.qlen = queries->len[pt.q];
        t.rows = (uint32_t) pt.rows;
        uint32_t dmax = 0;
        uint64_t slab = 0;
        for (uint32_t sl = 0; sl < pt.n; ++sl)
          {
            const uint32_t ti = tidx[pt.pair[sl]];
            t.toff[sl] = targets->off[ti];
            t.tlen[sl] = targets->len[ti];
            dmax = std::max(dmax, (targets->len[ti] + 3u) & ~3u);
            slab += (uint64_t) t.qlen + t.tlen[sl] + 1;
          }
        t.steps = dmax + 16;                                // pipeline drain (15) rounded to an even step count: the DP
                                                            // kernel stores row checkpoints two steps at a time
        const uint64_t total_lanes = (t.qlen + pt.rows - 1) / pt.rows;
        const uint64_t nstrips = (total_lanes + 15) / 16;
        d.t_dwords[x] = vsx_ckpt_dwords(nstrips, t.steps, (uint64_t) pt.rows, pt.tilt);
        t.strip_off = nstrips > 1 ? 2ull * 4 * t.steps : 0;                          // size for now, offset after the scan
        d.t_slab[x] = slab;
        pl.tasks[x] = t;
      }
  });
}

// the serial scan: checkpoint / strip / slab offsets of every task, the chunks and their launches
void layout_chunks(PlanDraft & d, vsx_plan & pl)
{
  const std::vector<ProtoTask> & protos = d.protos;
  const size_t NT = protos.size();
  const uint64_t budget_dwords = d.budget_dwords;
  size_t np_out = 0;
  Chunk cur;
  auto close_chunk = [&]() {
    if (cur.task_count) pl.chunks.push_back(cur);
    Chunk nc;
    nc.task_first = cur.task_first + cur.task_count;
    nc.pair_first = cur.pair_first + cur.pair_count;
    cur = nc;
  };
  // sparse-task classes: the nq tasks of a wave -- consecutive tasks of the launch, counted from its first -- share ONE checkpoint block
  // and one step range (the longest of them); `wave_left` tasks of the open wave are still to come, they take `wave_off` / `wave_steps`
  uint32_t wave_left = 0, wave_steps = 0, wave_group = 0, pair_left = 0;
  uint64_t wave_off = 0;
  for (size_t x = 0; x < NT; ++x)
    {
      const ProtoTask & pt = protos[x];
      VsxTask & t = pl.tasks[x];
      uint64_t dwords = d.t_dwords[x];
      const uint64_t strip = t.strip_off;
      const bool sparse_task = pt.nq == 2 || pt.nq == 4;
      if (pt.nq == 8)
        {
          // a pair-profile group of four (consecutive tasks of one query): never cut a chunk inside it
          if (pair_left == 0)
            {
              pair_left = 4;
              // (the WHOLE group must fit: a chunk that overshoots the budget -- which is the size of the context's current block once one
              //  exists -- by three tasks asks for a slightly larger block while the old one is still held by the plans in flight:
              //  out of memory in the middle of an allpairs run, profiles/r05/r05j_pairprof_first_contact.txt)
              uint64_t gsum = 0;
              for (size_t y = x; y < std::min(NT, x + 4); ++y) gsum += d.t_dwords[y];
              if (cur.task_count && cur.dir_dwords + gsum + VSX_CK_SLACK_DW > budget_dwords) close_chunk();
            }
          --pair_left;
        }
      else if (sparse_task && wave_left == 0)
        {
          // a new wave: its tasks are x .. x + nq - 1 as far as the class reaches (a chunk is never cut inside a wave)
          uint32_t smax = t.steps, members = 1;
          while (members < (uint32_t) pt.nq && x + members < NT && protos[x].cls() == protos[x + members].cls()) { smax = std::max(smax, pl.tasks[x + members].steps); ++members; }
          wave_left = members; wave_steps = smax; wave_group = 0;
          dwords = vsx_ckpt_dwords(1, smax, (uint64_t) pt.rows, pt.tilt);
          if (cur.task_count && cur.dir_dwords + dwords + VSX_CK_SLACK_DW > budget_dwords) close_chunk();
          wave_off = cur.dir_dwords;
        }
      else if (sparse_task) dwords = 0;                   // (the wave's block is already counted)
      else if (cur.task_count && cur.dir_dwords + dwords + VSX_CK_SLACK_DW > budget_dwords) close_chunk();
      if (sparse_task)
        {
          t.dir_off = wave_off;
          t.steps = wave_steps;
          t.group0 = wave_group;
          wave_group += 4u / (uint32_t) pt.nq;
          --wave_left;
        }
      else t.dir_off = cur.dir_dwords;
      t.strip_off = cur.strip_elems;
      cur.dir_dwords += dwords;
      cur.strip_elems += strip;
      pl.dir_bytes_total += dwords * 4;
      if (cur.launches.empty() || cur.launches.back().cls() != pt.cls())
        cur.launches.push_back(Launch {pt.cls(), (uint32_t) x, 0, cur.pair_first + cur.pair_count, 0});
      cur.launches.back().count++;
      if (strip != 0) cur.launches.back().multi = true;           // (a task owns hand-over rows only when it has a second strip)
      cur.launches.back().pair_count += pt.n;
      d.t_pair0[x] = np_out;
      np_out += pt.n;
      const uint64_t slab = d.t_slab[x];
      d.t_slab[x] = cur.slab_words;                       // from here on: the task's first slab word (chunk-relative)
      cur.slab_words += slab;
      cur.pair_count += pt.n;
      cur.task_count++;
    }
  close_chunk();
}

void fill_pair_tables(const PlanDraft & d, vsx_plan & pl)
{
  const size_t NT = d.protos.size();
  const int ntt = pass_threads(NT, 4096);
  run_threads(ntt, [&](int th) {
    const auto [lo, hi] = slice_of(NT, th, ntt);
    for (size_t x = lo; x < hi; ++x)
      {
        const ProtoTask & pt = d.protos[x];
        const VsxTask & t = pl.tasks[x];
        uint64_t slab = d.t_slab[x];
        for (uint32_t sl = 0; sl < pt.n; ++sl)
          {
            const size_t o = (size_t) d.t_pair0[x] + sl;
            pl.pair_slot[o] = (uint32_t) x * VSX_TASK_SLOTS + sl;
            pl.pair_ids[o] = pt.pair[sl];
            pl.slab_off[o] = slab;
            slab += (uint64_t) t.qlen + t.tlen[sl] + 1;
          }
      }
  });
}

// output arrays, 16-byte aligned sections of one block: score, aligned, matches, mismatches, gaps (2 B), verdict (1 B), text offset (8 B)
int allocate_output_arrays(vsx_ctx * ctx, uint64_t n_pairs, vsx_plan & pl)
{
  const uint64_t np = std::max<uint64_t>(n_pairs, 1);
  const uint64_t width[7] = {2, 2, 2, 2, 2, 1, 8};
  uint64_t at = 0;
  for (int x = 0; x < 7; ++x) { pl.soa_off[x] = at; at += (np * width[x] + 15) & ~15ull; }
  pl.soa_bytes = at;
  VSX_HIP(pl.d_soa.alloc(&ctx->pool, at));
  uint8_t * b = pl.d_soa.p;
  pl.soa.score = reinterpret_cast<int16_t *>(b + pl.soa_off[0]);
  pl.soa.aligned = reinterpret_cast<uint16_t *>(b + pl.soa_off[1]);
  pl.soa.matches = reinterpret_cast<uint16_t *>(b + pl.soa_off[2]);
  pl.soa.mismatches = reinterpret_cast<uint16_t *>(b + pl.soa_off[3]);
  pl.soa.gaps = reinterpret_cast<uint16_t *>(b + pl.soa_off[4]);
  pl.soa.verdict = b + pl.soa_off[5];
  pl.soa.text_off = reinterpret_cast<uint64_t *>(b + pl.soa_off[6]);
  return VSX_OK;
}

// ---- device buffers ----
int allocate_and_upload(vsx_ctx * ctx, uint64_t n_pairs, vsx_plan & pl)
{
  uint64_t max_dir = 1, max_strip = 1, max_slab = 1, worst_runs = 0;
  for (const Chunk & c : pl.chunks)
    {
      max_dir = std::max(max_dir, c.dir_dwords + VSX_CK_SLACK_DW);
      max_strip = std::max(max_strip, c.strip_elems);
      max_slab = std::max(max_slab, c.slab_words);
      worst_runs += c.slab_words;
    }
  const size_t ngp = pl.pair_ids.size();
  pl.runs_capacity = std::min<uint64_t>(worst_runs, std::max<uint64_t>(16ull << 20, 48ull * ngp)) + 1;
  // tests: a smaller first capacity (words, the capacity itself) forces settle_runs() to resize and run the plan again
  if (const char * c = std::getenv("VSX_TEST_RUNS_CAP")) pl.runs_capacity = std::min<uint64_t>(pl.runs_capacity, std::max<uint64_t>(1, std::strtoull(c, nullptr, 10)));
  VSX_HIP(pl.d_tasks.alloc(&ctx->pool, pl.tasks.size()));
  VSX_HIP(pl.d_pair_slot.alloc(&ctx->pool, ngp));
  VSX_HIP(pl.d_pair_ids.alloc(&ctx->pool, ngp));
  VSX_HIP(pl.d_slab_off.alloc(&ctx->pool, ngp));
  VSX_HIP(pl.d_slot.alloc(&ctx->pool, pl.tasks.size() * VSX_TASK_SLOTS));
  VSX_HIP(pl.d_out.alloc(&ctx->pool, n_pairs));
  VSX_HIP(pl.d_cursor.alloc(&ctx->pool, 3));
  const int arc = allocate_output_arrays(ctx, n_pairs, pl);
  if (arc != VSX_OK) return arc;
  {
    std::lock_guard<std::mutex> lk(ctx->stage_mu);
    if (!ctx->cursor_slots.empty()) { pl.h_cursor = ctx->cursor_slots.back(); ctx->cursor_slots.pop_back(); }
  }
  if (!pl.h_cursor) VSX_HIP(hipHostMalloc(reinterpret_cast<void **>(&pl.h_cursor), 64, hipHostMallocDefault));
  // one checkpoint buffer, reused chunk after chunk: overlapping chunk k's traceback with chunk k+1's DP bought nothing
  // (both are issue-bound), while a second buffer doubled a multi-second hipMalloc
  for (int k = 0; k < 2; ++k)
    {
      const uint64_t need = (k == 0 ? max_dir : max_slab) * 4;
      uint64_t seen = ctx->req_hwm[k].load();
      while (need > seen && !ctx->req_hwm[k].compare_exchange_weak(seen, need)) { }
    }
  VSX_HIP(pl.d_dir[0].alloc(ctx->shared_dir[pl.dir_slot], &ctx->pool, max_dir));
  VSX_HIP(pl.d_strip.alloc(&ctx->pool, max_strip));
  VSX_HIP(pl.d_slab.alloc(ctx->shared_slab, &ctx->pool, max_slab));
  VSX_HIP(pl.d_runs.alloc(&ctx->pool, pl.runs_capacity));
  // text: <= 6 bytes per run (5 digits + op) + NUL + padding per pair in the worst case; typical alignments need ~2 per run
  pl.text_capacity = std::min<uint64_t>(6 * worst_runs + 8 * (uint64_t) ngp, std::max<uint64_t>(32ull << 20, 128ull * ngp)) + 16;
  // tests: the same for the text (bytes): settle() resizes and runs the text kernel again
  if (const char * c = std::getenv("VSX_TEST_TEXT_CAP")) pl.text_capacity = std::min<uint64_t>(pl.text_capacity, std::max<uint64_t>(4, std::strtoull(c, nullptr, 10)));
  VSX_HIP(pl.d_text.alloc(&ctx->pool, pl.text_capacity));
  if (!pl.tasks.empty())
    VSX_HIP(hipMemcpyAsync(pl.d_tasks.p, pl.tasks.data(), pl.tasks.size() * sizeof(VsxTask), hipMemcpyHostToDevice, ctx->stream_up));
  if (ngp)
    {
      VSX_HIP(hipMemcpyAsync(pl.d_pair_slot.p, pl.pair_slot.data(), ngp * 4, hipMemcpyHostToDevice, ctx->stream_up));
      VSX_HIP(hipMemcpyAsync(pl.d_pair_ids.p, pl.pair_ids.data(), ngp * 4, hipMemcpyHostToDevice, ctx->stream_up));
      VSX_HIP(hipMemcpyAsync(pl.d_slab_off.p, pl.slab_off.data(), ngp * 8, hipMemcpyHostToDevice, ctx->stream_up));
    }
  VSX_HIP(hipEventCreate(&pl.ev_begin));
  VSX_HIP(hipEventCreate(&pl.ev_end));
  for (Chunk & c : pl.chunks)
    {
      VSX_HIP(hipEventCreate(&c.e0));
      VSX_HIP(hipEventCreate(&c.e1));
      VSX_HIP(hipEventCreate(&c.e1b));
      VSX_HIP(hipEventCreate(&c.e2));
    }
  VSX_HIP(hipStreamSynchronize(ctx->stream_up));
  return VSX_OK;
}

}  // namespace

extern "C" {

int vsx_plan_create(vsx_ctx * ctx, vsx_plan ** out, const vsx_seqset * queries, const vsx_seqset * targets,
                    uint64_t n_pairs, const uint32_t * qidx, const uint32_t * tidx, uint64_t dir_budget_bytes)
{
  if (!ctx || !out || !queries || !targets || (n_pairs && (!qidx || !tidx)))
    return fail(VSX_EINVAL, "vsx_plan_create: null argument");
  *out = nullptr;
  // a sequence set is device memory: any context of the same GPU may align against it (one Database mirror serves all the
  // worker threads' contexts, shim/vsx_search16_shim.cpp); it must outlive the plans that use it
  if (queries->device != ctx->device || targets->device != ctx->device)
    return fail(VSX_EINVAL, "vsx_plan_create: seqset lives on another device");
  if (n_pairs > 0xffffffffull / 8) return fail(VSX_EINVAL, "vsx_plan_create: too many pairs for one plan");
  static const bool timing = std::getenv("VSX_DEBUG_TIMING") != nullptr;
  PlanDraft d;
  std::unique_ptr<vsx_plan> pl;
  int rc = VSX_OK;
  {
    vsxp::Stopwatch sw(d.t_classify);
    if ((rc = validate_pairs(queries, targets, n_pairs, qidx, tidx)) != VSX_OK) return rc;
    VSX_HIP(hipSetDevice(ctx->device));
    pl.reset(new vsx_plan);
    pl->ctx = ctx; pl->Q = queries; pl->T = targets; pl->n_pairs = n_pairs;
    acquire_dir_slot(ctx, *pl);
    classify_pairs(ctx, queries, targets, n_pairs, qidx, tidx, d, *pl);
  }
  {
    vsxp::Stopwatch sw(d.t_group);
    group_by_query(ctx, queries, targets, n_pairs, qidx, tidx, d);
    if ((rc = mark_pair_groups(queries, targets, tidx, d)) != VSX_OK) return rc;
    merge_thin_row_classes(queries, d);
    demote_small_sparse_classes(d);
    if ((rc = mark_split_profile(queries, targets, tidx, d)) != VSX_OK) return rc;
    sort_by_class(d);
    if ((rc = choose_dir_budget(ctx, dir_budget_bytes, d, *pl)) != VSX_OK) return rc;
  }
  {
    vsxp::Stopwatch sw(d.t_tasks);
    fill_task_descriptors(queries, targets, tidx, d, *pl);
    layout_chunks(d, *pl);
    fill_pair_tables(d, *pl);
  }
  {
    vsxp::Stopwatch sw(d.t_device);
    if ((rc = allocate_and_upload(ctx, n_pairs, *pl)) != VSX_OK) return rc;
  }
  if (timing)
    std::fprintf(stderr, "vsx_plan_create: %llu pairs, %zu tasks: classify %.2f ms, group %.2f ms (budget query %.2f), tasks %.2f ms, device buffers + upload %.2f ms\n",
                 (unsigned long long) n_pairs, pl->tasks.size(), d.t_classify * 1e3, d.t_group * 1e3, d.t_budget * 1e3, d.t_tasks * 1e3, d.t_device * 1e3);
  *out = pl.release();
  return VSX_OK;
}

int vsx_plan_set_filter(vsx_plan * pl, const vsx_filter * f)
{
  if (!pl) return fail(VSX_EINVAL, "vsx_plan_set_filter: null plan");
  pl->filter = VsxFilterDev {};            // (also drops the lists of a ranked plan: plan_set_ranked() follows the filter)
  if (!f) return VSX_OK;
  if (f->iddef < 0 || f->iddef > 4) return fail(VSX_EINVAL, "vsx_plan_set_filter: iddef must be 0..4");
  VsxFilterDev & d = pl->filter;
  d.enabled = 1; d.iddef = f->iddef; d.leftjust = f->leftjust; d.rightjust = f->rightjust;
  d.id = f->id; d.weak_id = f->weak_id; d.maxid = f->maxid; d.mid = f->mid; d.query_cov = f->query_cov; d.target_cov = f->target_cov;
  d.maxsubs = f->maxsubs; d.maxgaps = f->maxgaps; d.mincols = f->mincols; d.maxdiffs = f->maxdiffs;
  pl->ran = false;
  return VSX_OK;
}

}  // extern "C"

// r06: make `pl` a RANKED plan -- its traceback lists the kept and the refused pairs (vsx_device.hip rank_note) for fetch_ranked_core.
int vsxh::plan_set_ranked(vsx_plan * pl)
{
  if (!pl->filter.enabled) return VSX_OK;
  vsx_ctx * ctx = pl->ctx;
  const size_t n = (size_t) pl->n_pairs;
  VSX_HIP(hipSetDevice(ctx->device));
  VSX_HIP(pl->d_rank_counts.alloc(&ctx->pool, 2));
  VSX_HIP(pl->d_kept_pair.alloc(&ctx->pool, n + 1));
  VSX_HIP(pl->d_kept_id.alloc(&ctx->pool, n + 1));
  VSX_HIP(pl->d_refused_pair.alloc(&ctx->pool, n + 1));
  pl->filter.rank_counts = pl->d_rank_counts.p;
  pl->filter.kept_pair = pl->d_kept_pair.p;
  pl->filter.kept_id = pl->d_kept_id.p;
  pl->filter.refused_pair = pl->d_refused_pair.p;
  return VSX_OK;
}

extern "C" {

int vsx_plan_run(vsx_plan * pl)
{
  if (!pl) return fail(VSX_EINVAL, "vsx_plan_run: null plan");
  vsx_ctx * ctx = pl->ctx;
  VSX_HIP(hipSetDevice(ctx->device));
  hipStream_t st = pl->alt_fwd ? ctx->stream_b : ctx->stream, st2 = ctx->stream2;
  const int slot = pl->dir_slot;
  const int poison = vsx_internal_poison_byte();      // -1: off, and no stream operation is added below
  VSX_HIP(hipMemsetAsync(pl->d_cursor.p, 0, 3 * sizeof(unsigned long long), st));
  if (pl->filter.rank_counts) VSX_HIP(hipMemsetAsync(pl->d_rank_counts.p, 0, 2 * sizeof(uint32_t), st));      // (every run: settle() may run a plan twice)
  VSX_HIP(hipEventRecord(pl->ev_begin, st));
  const VsxTextOut tx {pl->d_text.p, pl->text_capacity, pl->d_cursor.p + 1, pl->soa};
  // DP kernels on `st`, tracebacks + text on `st2`.  A plan's DP waits only for the last traceback that read ITS checkpoint
  // block (the context alternates two), so it overlaps the previous plan's traceback; inside a plan the chunks share the block.
  for (size_t k = 0; k < pl->chunks.size(); ++k)
    {
      Chunk & c = pl->chunks[k];
      uint32_t * dir = pl->d_dir[0].p;
      if (k >= 1) VSX_HIP(hipStreamWaitEvent(st, pl->chunks[k - 1].e2, 0));      // buffer reuse: the previous traceback is done
      else if (ctx->ev_tb_used[slot]) VSX_HIP(hipStreamWaitEvent(st, ctx->ev_tb[slot], 0));
      // VSX_POISON: what this chunk is about to use of the SHARED checkpoint block (SharedSlot::acquire hands the current block out
      // untouched) and of the strip buffer; stream-ordered, behind the wait for the last traceback that read the block
      if (poison >= 0)
        {
          VSX_HIP(hipMemsetAsync(dir, poison, (c.dir_dwords + VSX_CK_SLACK_DW) * sizeof(uint32_t), st));
          if (c.strip_elems) VSX_HIP(hipMemsetAsync(pl->d_strip.p, poison, c.strip_elems * sizeof(uint2), st));
        }
      VSX_HIP(hipEventRecord(c.e0, st));
      for (const Launch & L : c.launches)
        {
          VsxDevParams Pf = L.tilt ? ctx->Pt : ctx->P;
          Pf.max3 = (L.tilt == 2) ? 1 : 0;
          Pf.es_skipped = pl->d_cursor.p + 2;
          static const bool one_off = std::getenv("VSX_ONESTRIP") && std::strcmp(std::getenv("VSX_ONESTRIP"), "0") == 0;      // A/B, tests: the general kernels
          VSX_HIP(vsx_launch_forward(L.rows, L.track, L.nq, (L.multi || (one_off && L.nq < 8)) ? 0 : 1, Pf, pl->d_tasks.p + L.first, L.count,
                                    pl->Q->codes(), pl->T->codes(), dir, pl->d_strip.p,
                                    pl->d_slot.p + (size_t) L.first * VSX_TASK_SLOTS, st));
        }
      VSX_HIP(hipEventRecord(c.e1, st));
      VSX_HIP(hipStreamWaitEvent(st2, c.e1, 0));
      if (poison >= 0 && c.slab_words) VSX_HIP(hipMemsetAsync(pl->d_slab.p, poison, c.slab_words * sizeof(uint32_t), st2));      // the shared slab
      VSX_HIP(hipEventRecord(c.e1b, st2));
      for (size_t li = 0; li < c.launches.size();)      // the recompute traceback is specialised on R like the DP kernel
        {
          const Launch & L = c.launches[li];
          // (the sparse-task variants of one class -- nq = 1, 2, 4, adjacent in the class order -- share ONE traceback launch: the
          //  traceback finds a pair's lane group through its task and does not know about nq; their pairs are contiguous)
          uint32_t pair_count = L.pair_count;
          size_t lj = li + 1;
          while (lj < c.launches.size() && c.launches[lj].same_traceback(L)) { pair_count += c.launches[lj].pair_count; ++lj; }
          VsxDevParams Pb = L.tilt ? ctx->Pt : ctx->P;
          Pb.max3 = (L.tilt == 2) ? 1 : 0;         // the checkpoints of the MAX3 class carry its bias
          VSX_HIP(vsx_launch_traceback_ck(L.rows, L.track == 0 ? 1 : 0, Pb, pl->filter, pl->d_tasks.p, pl->d_pair_slot.p + L.pair_first,
                                         pl->d_pair_ids.p + L.pair_first, pair_count, pl->Q->codes(), pl->T->codes(),
                                         dir, pl->d_slot.p, pl->d_slab.p, pl->d_slab_off.p + L.pair_first,
                                         pl->d_runs.p, pl->runs_capacity, pl->d_cursor.p, pl->d_out.p, tx, st2));
          li = lj;
        }
      VSX_HIP(hipEventRecord(c.e2, st2));
    }
  if (pl->chunks.empty()) VSX_HIP(hipStreamWaitEvent(st2, pl->ev_begin, 0));          // (the cursor memset precedes the text kernel)
  VSX_HIP(hipEventRecord(ctx->ev_tb[slot], st2));
  ctx->ev_tb_used[slot] = true;
  // run lists -> CIGAR text, records -> output arrays (pushop / finishop are part of the reference's timed path).  The traceback
  // epilogues have done that for every pair they visited, and every device pair (pair_ids) belongs to a task of a chunk, whose class
  // has a traceback launch above: nothing is left for the text kernel (settle() still runs it when only the text buffer was short).
  // A build without VSX_TB_FUSED_TEXT launches it here for all of them; st2 is in order
  if (!VSX_TB_FUSED_TEXT || pl->chunks.empty())
    VSX_HIP(vsx_launch_cigar_text(pl->d_out.p, pl->d_pair_ids.p, (uint32_t) pl->pair_ids.size(), pl->d_runs.p, pl->runs_capacity,
                                 pl->d_text.p, pl->text_capacity, pl->d_cursor.p + 1, pl->soa, st2));
  VSX_HIP(hipMemcpyAsync(pl->h_cursor, pl->d_cursor.p, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st2));
  VSX_HIP(hipEventRecord(pl->ev_end, st2));
  pl->ran = true;
  pl->host_patched = false;            // the exported records of host-answered pairs point behind THIS run's device runs
  return VSX_OK;
}

int vsx_plan_sync(vsx_plan * pl, vsx_timing * tm)
{
  if (!pl) return fail(VSX_EINVAL, "vsx_plan_sync: null plan");
  if (!pl->ran) return fail(VSX_EINVAL, "vsx_plan_sync: plan has not been run");
  VSX_HIP(hipSetDevice(pl->ctx->device));
  VSX_HIP(hipEventSynchronize(pl->ev_end));
  if (tm)
    {
      *tm = vsx_timing {};
      for (Chunk & c : pl->chunks)
        {
          float a = 0, b = 0;
          VSX_HIP(hipEventElapsedTime(&a, c.e0, c.e1));
          VSX_HIP(hipEventElapsedTime(&b, c.e1b, c.e2));
          tm->forward_ms += a;
          tm->traceback_ms += b;
          tm->forward_launches += (uint32_t) c.launches.size();
          tm->traceback_launches += 1;
        }
      VSX_HIP(hipEventElapsedTime(&tm->total_ms, pl->ev_begin, pl->ev_end));
      tm->cells = pl->cells;
      tm->dir_bytes = pl->dir_bytes_total;
      tm->steps_skipped = pl->h_cursor[2];
    }
  return VSX_OK;
}

int vsx_plan_describe(const vsx_plan * pl, vsx_plan_info * info)
{
  if (!pl || !info) return fail(VSX_EINVAL, "vsx_plan_describe: null argument");
  *info = vsx_plan_info {};
  info->tasks = pl->tasks.size();
  info->chunks = (uint32_t) pl->chunks.size();
  uint64_t best = 0;
  for (const Chunk & c : pl->chunks)
    for (const Launch & L : c.launches)
      {
        if (L.nq == 2 || L.nq == 4) info->tasks_sparse += L.count;
        if (L.nq == 8) info->tasks_pair += L.count;
        if (L.nq == 16) info->tasks_split += L.count;
        info->waves += (L.nq == 2 || L.nq == 4) ? (L.count + (uint32_t) L.nq - 1) / (uint32_t) L.nq : L.count;
        if (L.tilt) info->tasks_tilted += L.count;
        if (L.tilt == 2) info->tasks_max3 += L.count;
        if (L.track) info->tasks_tracked += L.count;
        if (L.count > best) { best = L.count; info->rows_dominant = (uint32_t) L.rows; }
      }
  return VSX_OK;
}

void vsx_plan_destroy(vsx_plan * pl)
{
  if (!pl) return;
  (void) hipSetDevice(pl->ctx->device);
  // all of a plan's device work precedes its ev_end (uploads were synchronised at creation): waiting for the context's
  // streams instead would also wait for the NEXT plan of a pipeline and leave the GPU idle between slices
  if (pl->ran) (void) hipEventSynchronize(pl->ev_end);
  delete pl;
}

}  // extern "C"
