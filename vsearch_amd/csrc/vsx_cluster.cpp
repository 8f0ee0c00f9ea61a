// vsx_cluster.cpp -- the clustering rounds (vsx_cluster_fast, include/vsx_search.h) on the searcher of vsx_search.cpp.
//
// cluster_fast / cluster_smallmem-style greedy centroid clustering (core/cluster.cpp:877-1031 cluster_core_parallel,
// :601-856 evaluate_extra_hits).  Sequences are processed in the given order (the caller sorts: --cluster_fast =
// length descending, Database::sortbylength core/db.cpp:433-450).  A ROUND of `round` sequences is searched against
// the centroids known at the start of the round (one staged GPU search, as vsx_search_batch); the sequential
// reconciliation then replays the reference's intra-round fix-up: sequences of the same round that became centroids
// are inserted into the hit list by shared k-mers and the accept loop is re-run from the top.  The reference
// proves (and the survey verified) that the result does not depend on the round size, i.e. equals the serial
// algorithm; the (query, new-centroid) alignments the fix-up may need are aligned speculatively in one GPU batch.
#include "vsx_search_internal.h"

using namespace vsxs;

namespace {

bool enough_kmers(const vsx_searcher & S, uint32_t shared, uint32_t kmersamplecount)     // searchcore.cpp:251-257
{
  return ((int64_t) shared >= S.minwordmatches) || (shared >= kmersamplecount);
}

// The centroid index grows by up to `round` sequences per round (Dbindex::add_sequence, cluster.cpp:1009).  Rebuilding it
// every round cost 15 % of a 1 M-sequence run and grows quadratically; instead a MAIN index is rebuilt only when the DELTA
// index over the centroids added since has grown past an eighth of it, the small delta is rebuilt every round, and a query is
// counted against both: a centroid lives in exactly one of them, thresholds are per sequence, and the union of the two
// top-N selections contains the top N of the union.
// This is the rebuild rule; the prefetch asks it too (could this round's centroids trigger a rebuild?), so the two agree.
bool main_outgrown(size_t total, size_t main_n, uint64_t round) { return total - main_n > main_n / 8 + 2 * round; }

struct IxDel { void operator()(VsxKmerIndex * p) const { vsx_kmer_index_destroy(p); } };
typedef std::unique_ptr<VsxKmerIndex, IxDel> IndexPtr;
typedef std::vector<std::vector<uint32_t>> WordLists;
typedef std::vector<std::vector<Cand>> CandLists;

// unique words of the members a0 .. a0 + cnt - 1 (they depend on no result: the prefetch computes them one round ahead)
void round_words(const vsx_searcher * S, uint64_t a0, uint64_t cnt, WordLists & dst, std::vector<std::vector<uint64_t>> & seen, int threads)
{
  dst.assign(cnt, {});
  if (seen.size() < (size_t) threads) seen.resize((size_t) threads, std::vector<uint64_t>(seen_words(*S), 0));
  std::atomic<uint64_t> next {0};
  auto work = [&](int tid) {
    for (;;)
      {
        const uint64_t k = next.fetch_add(16);
        if (k >= cnt) break;
        for (uint64_t x = k; x < std::min(cnt, k + 16); ++x)
          unique_kmers(S->blob.data() + S->off[a0 + x], S->len[a0 + x], S->w, S->o.soft_mask != 0, dst[x], seen[(size_t) tid]);
      }
  };
  run_pool(threads, work);
}

// The helper of the NEXT round: its unique words, and -- when the current round cannot trigger a rebuild of the main index even if
// every member founds a cluster -- its ranking against the main index (r03: that ranking is a third of the run and depends on
// nothing the current round decides; only the small delta index has to wait for its centroids).  The thread sees the searcher, the
// main index, main_list (a snapshot that changes only at a main rebuild, never the growing centroid list), the k-mer statistics and
// its own output.  take() joins before it moves the results out, so nothing a later start() writes is readable by a round (the
// hand-off oracle/soak_cluster.py caught in r04, with rounds of three sequences, raced exactly there).
struct Prefetch {
  struct Taken { bool words = false, main = false; WordLists kmers; CandLists cands; std::vector<uint64_t> fallback; };

  ~Prefetch() { if (th.joinable()) th.join(); }

  void start(const vsx_searcher * S, VsxKmerIndex * cix, const std::vector<uint32_t> * main_list, KmerAcct * kacct, uint64_t a0, uint64_t cnt,
             bool main_safe, int threads)
  {
    s0 = a0;
    main_s0 = main_safe ? a0 : UINT64_MAX;
    th = std::thread(&Prefetch::run, this, S, cix, main_list, kacct, a0, cnt, main_safe, threads);
  }

  // what the helper made for the round that starts at `at`; an error of the helper is the caller's
  int take(uint64_t at, Taken & out)
  {
    if (th.joinable()) th.join();
    if (rc != VSX_OK) { vsx_internal_set_error(err.c_str()); return rc; }
    out.words = (s0 == at);
    out.main = (main_s0 == at);                             // the helper already ranked this round against the main index
    if (out.words) out.kmers = std::move(kmers);
    if (out.main) { out.cands = std::move(cands); out.fallback = std::move(fallback); }
    s0 = main_s0 = UINT64_MAX;
    return VSX_OK;
  }

private:
  void run(const vsx_searcher * S, VsxKmerIndex * cix, const std::vector<uint32_t> * main_list, KmerAcct * kacct, uint64_t a0, uint64_t cnt,
           bool main_safe, int threads)
  {
    round_words(S, a0, cnt, kmers, seen, threads);
    if (!main_safe) return;
    cands.assign(cnt, {});
    fallback.clear();
    rc = device_rank(S, cix, main_list, cnt, kmers, (uint32_t) std::max<int64_t>(S->tophits, 1), 1024, true, cands, fallback, *kacct,
                     threads);                                // (runs beside the staged search and the near helper)
    if (rc != VSX_OK) err = vsx_last_error();
  }

  WordLists kmers;
  CandLists cands;                                          // the ranking of the next round against the MAIN centroid index
  std::vector<uint64_t> fallback;
  uint64_t s0 = UINT64_MAX, main_s0 = UINT64_MAX;
  int rc = VSX_OK;
  std::string err;
  std::vector<std::vector<uint64_t>> seen;
  std::thread th;
};

struct Near { uint32_t k, shared; int64_t res; };            // res = index into the speculative results, -1 none

// the state of one round; released as one object (release_round)
struct Round {
  const uint64_t s0, wn;
  std::vector<QState> st;
  WordLists kmers;
  std::vector<uint64_t> fallback;                            // round members the device counters cannot serve
  std::vector<std::vector<Near>> near;                       // per member: earlier members with shared words, ascending
  std::vector<uint32_t> sq, stg;                             // the speculative pairs
  // (the speculative alignments of the fix-up follow the staged search on the same context: aligned by the helper on a second
  //  context beside the search they measured level in r05)
  vsx_results spec;
  std::vector<uint32_t> extras;                              // round members that became centroids, in order
  std::vector<uint8_t> is_extra;
  // the helper of phase 1c (near_device) writes near, sq, stg and these two until it is joined
  int near_rc = VSX_OK;
  std::string near_err;
  std::thread near_thread;
  Round(uint64_t s0_, uint64_t wn_) : s0(s0_), wn(wn_), st(wn_), kmers(wn_), near(wn_), is_extra(wn_, 0) { std::memset(&spec, 0, sizeof spec); }
  ~Round() { if (near_thread.joinable()) near_thread.join(); vsx_results_free(&spec); }
};

struct Scratch { std::vector<uint16_t> counts; std::vector<uint32_t> touched, km; std::vector<uint64_t> seen; };

// One call of vsx_cluster_fast: the state that lives across rounds, one function per phase of a round.  Everything here belongs to
// the calling thread; the helpers are handed what they may touch (Prefetch::start, near_device's Round, the reaper's dead Round).
struct ClusterRun {
  vsx_searcher * const S;
  const uint64_t round, n;
  const double t_begin = now_s();
  const int nth;
  const bool dev_kmer;
  const int64_t hit_capacity;
  IncIndex inc;
  std::vector<uint32_t> clusterno;
  // r06: a member's one reported hit goes straight into the result's record form, in sequence order (a vector of Hit per sequence was
  // 1.2 M small blocks made one by one and released one by one at return)
  std::vector<vsx_hit> kept_rec;
  std::string kept_cigar;
  uint32_t nclusters = 0;
  Acct acct;
  double t_kmer = 0;
  double tm_words = 0, tm_rebuild = 0, tm_rank = 0, tm_stages = 0, tm_near = 0, tm_spec = 0, tm_recon = 0, tm_free = 0;      // VSX_DEBUG_TIMING
  std::vector<Scratch> scratch;
  // device k-mer counting (vsx_kmer.hip): main and delta index over the centroids (main_outgrown), and one over the members of
  // the current round (the intra-round shared-word counts of evaluate_extra_hits)
  IndexPtr cix, dix, rix;
  std::vector<uint32_t> centroid_list;                   // sequence numbers of the centroids, ascending
  std::vector<uint32_t> delta_list;                      // the tail of centroid_list the delta index stands for
  std::vector<uint32_t> main_list;                       // the centroids the main index stands for
  size_t main_n = 0, delta_built = 0;                    // centroids in the main index; centroid count when the delta was last built
  KmerAcct kacct;
  std::vector<std::vector<uint64_t>> main_seen;
  Prefetch pre;                                          // (after everything its thread reads: joined first)
  std::thread reaper;                                    // releases the previous round's host state (release_round)

  ClusterRun(vsx_searcher * S_, uint64_t round_)
    : S(S_), round(round_), n(S_->len.size()), nth(std::max(1, S_->threads)), dev_kmer(device_kmer_subsets_ok(*S_)),
      hit_capacity(std::min<int64_t>(S_->ma + S_->mr - 1, S_->tophits)), clusterno(n, 0), scratch((size_t) nth)
  {
    inc.post.assign(1ull << (2 * S->w), {});
    S->is_centroid.assign(n, 0);
    for (auto & sc : scratch) { sc.counts.assign(n, 0); sc.seen.assign(seen_words(*S), 0); }
  }
  ~ClusterRun() { if (reaper.joinable()) reaper.join(); }

  const char * seq_of(uint64_t seqno) const { return S->blob.data() + S->off[seqno]; }

  // r06: the largest plan of the run is a full round with eight candidates per member: its checkpoint block is reserved now, in one
  // piece -- left to grow with the early rounds' plans (few centroids: few candidates) the context re-allocated multi-GB blocks eight times,
  // 1.1 s of a 6-7 s run (profiles/r06/r06e_cluster_blocks.txt).  Sized for the mean length + 10 % (amplicons), never more than a
  // quarter of the device; a run that outgrows it grows the block as before.
  void reserve_checkpoint_block()
  {
    if (n == 0) return;
    uint64_t tot = 0;
    for (uint64_t i = 0; i < n; ++i) tot += S->len[i];
    const uint32_t typical = (uint32_t) std::min<uint64_t>(65535, tot / n + tot / n / 10 + 1);
    uint64_t want[4] = {vsx_internal_ckpt_bytes_estimate(S->ctx, std::min<uint64_t>(round, n), typical, typical), 0, 0, 0};
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void) hipGetLastError(); free_b = 0; }
    want[0] = std::min<uint64_t>(want[0], (uint64_t) free_b / 4);
    if (want[0] >= (16ull << 20)) (void) vsx_internal_scratch_reserve(S->ctx, want);
  }

  int create_indexes()
  {
    for (IndexPtr * ix : {&cix, &rix, &dix})
      {
        VsxKmerIndex * a = nullptr;
        const int irc = vsx_kmer_index_create_empty(S->ctx, S->dbset, S->w, &a);
        ix->reset(a);
        if (irc != VSX_OK) return irc;
      }
    return VSX_OK;
  }

  // the centroid indexes catch up with the centroids founded since: the main index when the delta has outgrown it, else the delta
  int refresh_indexes(bool have_main)
  {
    const size_t total = centroid_list.size();
    if (total == delta_built) return VSX_OK;
    if (main_outgrown(total, main_n, round))
      {
        if (have_main) return fail(VSX_EHIP, "vsx_cluster_fast: the main index changed under a prefetched ranking");   // (excluded by start_prefetch)
        const int irc = vsx_kmer_index_rebuild(cix.get(), centroid_list.data(), total);       // main: everything
        if (irc != VSX_OK) return irc;
        main_n = total;
        main_list.assign(centroid_list.begin(), centroid_list.end());
        delta_list.clear();
        static const uint32_t none = 0;                                                        // (a null list would mean "the whole set")
        const int drc = vsx_kmer_index_rebuild(dix.get(), &none, 0);
        if (drc != VSX_OK) return drc;
      }
    else
      {
        delta_list.assign(centroid_list.begin() + (long) main_n, centroid_list.end());
        const int drc = vsx_kmer_index_rebuild(dix.get(), delta_list.data(), delta_list.size());
        if (drc != VSX_OK) return drc;
      }
    delta_built = total;
    return VSX_OK;
  }

  // the helper of the round after R; it ranks against the main index only if R cannot outgrow it, whatever R decides
  void start_prefetch(const Round & R)
  {
    const uint64_t a0 = R.s0 + round;
    if (a0 >= n) return;
    const bool main_safe = main_n > 0 && !main_outgrown(centroid_list.size() + R.wn, main_n, round);
    pre.start(S, cix.get(), &main_list, &kacct, a0, std::min<uint64_t>(round, n - a0), main_safe, std::max(1, nth / 2));
  }

  // ---- phase 1a, device: k-mer candidates against the centroid indexes as of the round start (main + delta, merged; the members
  //      the counters cannot serve on the host) ----
  int rank_round(Round & R)
  {
    const uint64_t wn = R.wn;
    const double t0 = now_s();
    Prefetch::Taken pf;
    int krc = pre.take(R.s0, pf);
    if (krc != VSX_OK) return krc;
    if (pf.words) R.kmers = std::move(pf.kmers);
    else round_words(S, R.s0, wn, R.kmers, main_seen, nth);
    tm_words += now_s() - t0;
    const double tb0 = now_s();
    krc = refresh_indexes(pf.main);
    if (krc != VSX_OK) return krc;
    tm_rebuild += now_s() - tb0;
    start_prefetch(R);
    const double tr0 = now_s();
    CandLists cands(wn);
    const uint32_t keep_n = (uint32_t) std::max<int64_t>(S->tophits, 1);
    if (pf.main) { cands.swap(pf.cands); R.fallback.swap(pf.fallback); }
    else krc = device_rank(S, cix.get(), &main_list, wn, R.kmers, keep_n, 1024, true, cands, R.fallback, kacct);
    if (krc != VSX_OK) return krc;
    if (!delta_list.empty())
      {
        CandLists dc(wn);
        std::vector<uint64_t> fb2;
        krc = device_rank(S, dix.get(), &delta_list, wn, R.kmers, keep_n, 1024, true, dc, fb2, kacct);
        if (krc != VSX_OK) return krc;
        // union of the two selections, the heap's total order, the heap's size
        std::atomic<uint64_t> nx {0};
        run_pool(std::min(nth, 8), [&](int) {
          for (;;)
            {
              const uint64_t k = nx.fetch_add(64);
              if (k >= wn) break;
              for (uint64_t x = k; x < std::min<uint64_t>(wn, k + 64); ++x)
                {
                  if (dc[x].empty()) continue;
                  std::vector<Cand> & c = cands[x];
                  c.insert(c.end(), dc[x].begin(), dc[x].end());
                  const size_t kp = std::min<size_t>(c.size(), (size_t) keep_n);
                  std::partial_sort(c.begin(), c.begin() + (long) kp, c.end(), cand_better);
                  c.resize(kp);
                }
            }
        });
      }
    tm_rank += now_s() - tr0;
    for (uint64_t k = 0; k < wn; ++k) R.st[k].cands = std::move(cands[k]);
    if (!R.fallback.empty())
      {
        // the host's growing index is only read here, by the rare queries the device counters cannot serve: it catches up with
        // the centroids founded since its last use (r03: filling it eagerly -- 290 push_backs per centroid -- was a third of the
        // sequential reconcile phase of a 2 M-sequence run)
        std::vector<uint32_t> km;
        std::vector<uint64_t> seen(seen_words(*S), 0);
        for (; inc.indexed < centroid_list.size(); ++inc.indexed)
          {
            const uint32_t c = centroid_list[inc.indexed];
            unique_kmers(seq_of(c), S->len[c], S->w, S->o.soft_mask != 0, km, seen);
            for (uint32_t w2 : km) inc.post[w2].push_back(c);
          }
      }
    for (uint64_t k : R.fallback)
      {
        Scratch & sc = scratch[0];
        candidates_for(*S, seq_of(R.s0 + k), S->len[R.s0 + k], sc.counts, sc.touched, sc.km, sc.seen, R.st[k].cands, &inc);
      }
    return VSX_OK;
  }

  // ---- phase 1a, host: every member against the growing index, on host threads ----
  void rank_round_host(Round & R)
  {
    std::atomic<uint64_t> next {0};
    auto work = [&](int tid) {
      Scratch & sc = scratch[(size_t) tid];
      for (;;)
        {
          const uint64_t k = next.fetch_add(1);
          if (k >= R.wn) break;
          candidates_for(*S, seq_of(R.s0 + k), S->len[R.s0 + k], sc.counts, sc.touched, sc.km, sc.seen, R.st[k].cands, &inc);
          R.kmers[k] = sc.km;
        }
    };
    run_pool(nth, work);
  }

  // member i of the round shares `shared` words with the earlier member k: the fix-up may ask for their alignment
  void note_near(Round & R, uint64_t i, uint32_t k, uint32_t shared, bool enough)
  {
    Near nr {k, shared, -1};
    if (enough && acceptable_unaligned(*S, seq_of(R.s0 + i), S->len[R.s0 + i], (uint32_t) (R.s0 + k), S->meta_of(R.s0 + i)))
      {
        nr.res = (int64_t) R.sq.size();
        R.sq.push_back((uint32_t) (R.s0 + i));
        R.stg.push_back((uint32_t) (R.s0 + k));
      }
    R.near[i].push_back(nr);
  }

  // ---- phase 1c: intra-round shared k-mer counts (unique_count_shared, core/unique.cpp:356-395) and the (member i, earlier member
  //      k) pairs that the fix-up could ask for.  Device (r04): the counts need the round's words only -- nothing the staged search
  //      decides -- so this runs on a helper thread while phase 1b aligns: it rebuilds the round's own index, counts and pairs up the
  //      candidates (k-mer kernels and aligner kernels on their own streams; 1.07 s of a 6.6 s run at 2 M sequences sat behind it) ----
  void near_device(Round & R)
  {
    // the same counting problem on the device: members of the round against an index of the round
    const uint64_t s0 = R.s0, wn = R.wn;
    std::vector<uint32_t> round_list(wn);
    for (uint64_t i = 0; i < wn; ++i) round_list[i] = (uint32_t) (s0 + i);
    R.near_rc = vsx_kmer_index_rebuild(rix.get(), round_list.data(), wn);
    CandLists nc(wn);
    std::vector<uint64_t> none;
    if (R.near_rc == VSX_OK) R.near_rc = device_rank(S, rix.get(), &round_list, wn, R.kmers, 0xffffffffu, 1024, false, nc, none, kacct,
                                                     std::max(1, S->threads / 2));      // (beside the staged search: half the budget)
    if (R.near_rc != VSX_OK) { R.near_err = vsx_last_error(); return; }
    for (uint64_t i = 0; i < wn; ++i)
      for (const Cand & c : nc[i])                              // ascending target
        {
          const uint32_t k = (uint32_t) (c.target - s0);
          if (k >= i) break;                                    // only earlier members can have become centroids
          note_near(R, i, k, c.count, true);
        }
  }
  void near_host(Round & R)
  {
    std::vector<std::vector<uint32_t>> lpost(1ull << (2 * S->w));      // round-local: k-mer -> earlier members
    std::vector<uint16_t> cnt(R.wn, 0);
    std::vector<uint32_t> touched;
    for (uint64_t i = 0; i < R.wn; ++i)
      {
        touched.clear();
        for (uint32_t km : R.kmers[i])
          for (uint32_t k : lpost[km]) { if (cnt[k]++ == 0) touched.push_back(k); }
        std::sort(touched.begin(), touched.end());
        for (uint32_t k : touched)
          {
            const uint32_t shared = cnt[k];
            cnt[k] = 0;
            note_near(R, i, k, shared, enough_kmers(*S, shared, (uint32_t) R.kmers[i].size()));
          }
        for (uint32_t km : R.kmers[i]) lpost[km].push_back((uint32_t) i);
      }
  }

  // the pairs of phase 1c in one GPU batch
  int speculative_align(Round & R)
  {
    if (R.sq.empty()) return VSX_OK;
    const double t0 = now_s();
    const int rc = vsx_align_pairs(S->ctx, S->dbset, S->dbset, R.sq.size(), R.sq.data(), R.stg.data(), &R.spec);
    acct.t_align += now_s() - t0;
    tm_spec += now_s() - t0;
    if (rc != VSX_OK) return rc;
    acct.pairs += R.sq.size();
    return VSX_OK;
  }

  // evaluate_extra_hits (:601-856), first part: this round's new centroids (extras, increasing) with enough shared words enter
  // member i's hit list in the heap's order.  Returns how many did.
  int insert_extras(Round & R, uint64_t i)
  {
    std::vector<Hit> & hits = R.st[i].hits;
    const std::vector<Near> & near = R.near[i];
    int added = 0;
    auto try_insert = [&](uint32_t k, uint32_t shared) {
      if (!enough_kmers(*S, shared, (uint32_t) R.kmers[i].size())) return;
      const uint32_t length = S->len[R.s0 + k];
      int64_t x = (int64_t) hits.size();
      while (x > 0 && ((hits[(size_t) x - 1].count < shared) ||
                       (hits[(size_t) x - 1].count == shared && S->len[hits[(size_t) x - 1].target] > length)))
        --x;
      if (x < hit_capacity)
        {
          if ((int64_t) hits.size() >= hit_capacity) hits.pop_back();
          Hit h;
          h.target = (uint32_t) (R.s0 + k);
          h.count = shared;
          hits.insert(hits.begin() + x, std::move(h));
          ++added;
        }
    };
    // A member with words and a positive threshold can only qualify through a near[] entry (shared >= 1), so walk near[i] (sorted
    // by k) and keep the entries that are extras -- the same subsequence the loop over all extras would visit, without its
    // O(extras) cost; members without words (every extra qualifies: enough_kmers with kmersamplecount 0) take the full loop
    if (!R.kmers[i].empty() && S->minwordmatches > 0)
      {
        for (const Near & nr : near) if (R.is_extra[nr.k]) try_insert(nr.k, nr.shared);
      }
    else
      {
        size_t np = 0;                                           // near[i] is sorted by k, extras is increasing too
        for (uint32_t k : R.extras)
          {
            while (np < near.size() && near[np].k < k) ++np;
            try_insert(k, (np < near.size() && near[np].k == k) ? near[np].shared : 0);
          }
      }
    return added;
  }

  // evaluate_extra_hits, second part: the accept loop re-run from the top over member i's changed hit list
  int rerun_accepts(Round & R, uint64_t i)
  {
    const uint64_t seqno = R.s0 + i;
    QState & q = R.st[i];
    std::vector<Hit> & hits = q.hits;
    const int64_t ql = S->len[seqno];
    q.rejects = 0; q.accepts = 0;
    for (Hit & h : hits) { h.accepted = false; h.rejected = false; }
    for (size_t t = 0; (q.accepts < S->ma) && (q.rejects < S->mr) && (t < hits.size()); ++t)
      {
        Hit & h = hits[t];
        if (!h.aligned)
          {
            if (acceptable_unaligned(*S, seq_of(seqno), ql, h.target, S->meta_of(seqno)))
              {
                // single-target alignment (:743): taken from the speculative batch when it is there
                int64_t ri = -1;
                if (h.target >= R.s0 && h.target < R.s0 + R.wn)
                  for (const Near & nr : R.near[i]) if (nr.k == h.target - R.s0) { ri = nr.res; break; }
                vsx_results one;
                std::memset(&one, 0, sizeof one);
                const vsx_results * rp = &R.spec;
                if (ri < 0)
                  {
                    const uint32_t a = (uint32_t) seqno, b = h.target;
                    const int rc = vsx_align_pairs(S->ctx, S->dbset, S->dbset, 1, &a, &b, &one);
                    if (rc != VSX_OK) return rc;
                    ++acct.pairs;
                    rp = &one; ri = 0;
                  }
                acct.cells += (uint64_t) ql * S->len[h.target];
                const int rc = fill_hit(*S, [&]() { return seq_of(seqno); }, ql, h, *rp, (uint64_t) ri, acct.sentinels);
                vsx_results_free(&one);
                if (rc != VSX_OK) return fail(rc, "vsx_cluster_fast: fallback aligner failed");
              }
            else { h.rejected = true; ++q.rejects; }
          }
        if (!h.rejected)
          {
            if (acceptable_aligned(*S, ql, h, S->abundance(seqno))) ++q.accepts; else ++q.rejects;
          }
      }
    // delete all undetermined hits from the first one on (:841-854)
    size_t cut = hits.size();
    for (size_t t = hits.size(); t-- > 0;)
      if (!hits[t].accepted && !hits[t].rejected) cut = t;
    hits.resize(cut);
    return VSX_OK;
  }

  // search_findbest2_byid / _bysize (searchcore.cpp:960-1025, chosen by --sizeorder, cluster.cpp:1072-1079): first minimum
  // under the comparison, must be accepted
  const Hit * pick_best(const std::vector<Hit> & hits) const
  {
    const Hit * best = nullptr;
    if (S->o.sizeorder) { for (const Hit & h : hits) if (!best || hit_compare_bysize(*S, h, *best) < 0) best = &h; }
    else for (const Hit & h : hits) if (!best || hit_compare_byid(h, *best) < 0) best = &h;
    return (best && best->accepted) ? best : nullptr;
  }

  // ---- phase 2: sequential reconciliation in processing order ----
  int reconcile(Round & R)
  {
    for (uint64_t i = 0; i < R.wn; ++i)
      {
        const uint64_t seqno = R.s0 + i;
        if (insert_extras(R, i) != 0)
          {
            const int rc = rerun_accepts(R, i);
            if (rc != VSX_OK) return rc;
          }
        if (const Hit * best = pick_best(R.st[i].hits))
          {
            clusterno[seqno] = clusterno[best->target];
            kept_rec.emplace_back();
            hit_record(*best, (uint32_t) seqno, kept_cigar.size(), kept_rec.back());
            kept_cigar.append(best->cigar.c_str(), best->cigar.size() + 1);
          }
        else
          {
            clusterno[seqno] = nclusters++;
            R.extras.push_back((uint32_t) i);
            R.is_extra[i] = 1;
            S->is_centroid[seqno] = 1;
            centroid_list.push_back((uint32_t) seqno);
            if (!dev_kmer)
              {
                for (uint32_t km : R.kmers[i]) inc.post[km].push_back((uint32_t) seqno);    // Dbindex::add_sequence (:1009); device path: on demand
                ++inc.indexed;
              }
          }
      }
    return VSX_OK;
  }

  // r06: the round's host state -- 16 384 candidate lists, hit lists, word lists, near lists: ~80 000 heap blocks -- is released on a
  // helper thread beside the next round; on the main thread it was 7.6 ms per round, 0.93 s of a 5.9 s run at 2 M sequences, and in
  // nobody's accounting (profiles/r06/r06g_cluster_phases.txt).
  void release_round(std::unique_ptr<Round> R)
  {
    if (R->near_thread.joinable()) R->near_thread.join();
    if (reaper.joinable()) reaper.join();
    Round * dead = R.release();
    reaper = std::thread([dead]() { delete dead; });
  }

  int run_rounds()
  {
    for (uint64_t s0 = 0; s0 < n; s0 += round)
      {
        std::unique_ptr<Round> Rp(new Round(s0, std::min<uint64_t>(round, n - s0)));
        Round & R = *Rp;
        double t0 = now_s();
        if (dev_kmer)
          {
            const int rc = rank_round(R);
            if (rc != VSX_OK) return rc;
          }
        else rank_round_host(R);
        t_kmer += now_s() - t0;
        const bool near_on_device = dev_kmer && R.fallback.empty();
        if (near_on_device) R.near_thread = std::thread(&ClusterRun::near_device, this, std::ref(R));

        // ---- phase 1b: staged GPU search (queries and targets both live in the database sequence set) ----
        // (no lazy first batches as in vsx_search_batch: a round's plans are latency-bound, and a member whose best centroid fails
        //  pays one more stage -- measured slower in r05)
        const double ts0 = now_s();
        int rc = run_stages(*S, R.st, [&](uint64_t k) { return seq_of(s0 + k); }, [&](uint64_t k) { return seq_of(s0 + k); },
                            [&](uint64_t k) { return (int64_t) S->len[s0 + k]; },
                            [&](uint64_t k) { return (uint32_t) (s0 + k); }, [&](uint64_t k) { return S->meta_of(s0 + k); }, S->dbset, acct, nullptr, false);
        if (rc != VSX_OK) return rc;
        tm_stages += now_s() - ts0;

        t0 = now_s();
        if (near_on_device)
          {
            R.near_thread.join();
            if (R.near_rc != VSX_OK) { vsx_internal_set_error(R.near_err.c_str()); return R.near_rc; }
          }
        else near_host(R);
        t_kmer += now_s() - t0;
        tm_near += now_s() - t0;
        rc = speculative_align(R);
        if (rc != VSX_OK) return rc;

        const double t20 = now_s();
        rc = reconcile(R);
        if (rc != VSX_OK) return rc;
        tm_recon += now_s() - t20;
        const double tf0 = now_s();
        release_round(std::move(Rp));
        tm_free += now_s() - tf0;
      }
    if (reaper.joinable()) reaper.join();
    if (std::getenv("VSX_DEBUG_TIMING"))
      std::fprintf(stderr, "vsx_cluster_fast: words %.2f  centroid-index rebuild %.2f  rank vs centroids %.2f  staged search %.2f (align calls %.2f)  "
                           "intra-round counts %.2f  speculative align %.2f  reconcile %.2f  round state released %.2f  total %.2f s\n",
                   tm_words, tm_rebuild, tm_rank, tm_stages, acct.t_align - tm_spec, tm_near, tm_spec, tm_recon, tm_free, now_s() - t_begin);
    return VSX_OK;
  }

  int marshal(vsx_cluster_out * out)
  {
    vsx_hits * H = &out->hits;
    const int arc = alloc_hits(H, n, kept_rec.size(), kept_cigar.size());
    if (arc != VSX_OK) return arc;
    if (!kept_rec.empty()) std::memcpy(H->hit, kept_rec.data(), kept_rec.size() * sizeof(vsx_hit));
    if (!kept_cigar.empty()) std::memcpy(H->cigar_blob, kept_cigar.data(), kept_cigar.size());
    // the records are in sequence order, at most one per sequence
    uint64_t at = 0;
    for (uint64_t q = 0; q < n; ++q)
      {
        H->first[q] = at;
        if (at < kept_rec.size() && kept_rec[at].query == q) ++at;
      }
    H->first[n] = at;
    if (at != kept_rec.size()) { vsx_hits_free(H); return fail(VSX_EHIP, "vsx_cluster_fast: hit records out of order"); }
    out->n = n;
    out->n_clusters = nclusters;
    out->clusterno = (uint32_t *) std::malloc(std::max<uint64_t>(n, 1) * sizeof(uint32_t));
    if (!out->clusterno) { vsx_hits_free(&out->hits); return fail(VSX_ENOMEM, "vsx_cluster_fast: host allocation failed"); }
    std::memcpy(out->clusterno, clusterno.data(), n * sizeof(uint32_t));
    H->pairs_aligned = acct.pairs; H->cells_aligned = acct.cells; H->stages = acct.stages;
    H->sentinel_pairs = acct.sentinels; H->seconds_kmer = t_kmer; H->seconds_align = acct.t_align;
    H->seconds_total = now_s() - t_begin;
    return VSX_OK;
  }
};

}  // namespace

extern "C" {

int vsx_cluster_fast(vsx_searcher * S, uint64_t round, vsx_cluster_out * out)
{
  if (!S || !out) return fail(VSX_EINVAL, "vsx_cluster_fast: null argument");
  std::memset(out, 0, sizeof *out);
  // (never silently: a caller asking for --strand both must not get plus-strand clusters back)
  if (S->o.strand_both) return fail(VSX_EINVAL, "vsx_cluster_fast: clustering with --strand both is not provided");
  if (S->qmode != S->o.soft_mask) return fail(VSX_EINVAL, "vsx_cluster_fast: clustering masks everything by soft_mask; qmask must be 0");
  // (r03: 4096 before; with the next round's main ranking prefetched, fewer and larger rounds win: 10.4 -> 8.5 s at 2 M sequences)
  ClusterRun run(S, round ? round : 16384);
  run.reserve_checkpoint_block();
  int rc = run.dev_kmer ? run.create_indexes() : VSX_OK;
  if (rc == VSX_OK) rc = run.run_rounds();
  return rc != VSX_OK ? rc : run.marshal(out);
}

void vsx_cluster_out_free(vsx_cluster_out * o)
{
  if (!o) return;
  vsx_hits_free(&o->hits);
  std::free(o->clusterno);
  std::memset(o, 0, sizeof *o);
}

}  // extern "C"
