/*
  vsx_search.h -- C-ABI of the candidate-batch dispatch layer of libvsx: the part of vsearch's search core
  that decides WHICH (query, target) pairs reach the aligner and what happens to the results.

  Replaces (all citations relative to the reference's src/):
    search_onequery        core/searchcore.cpp:884-957   candidate loop, batches of MAXDELAYED = 8
    align_delayed          core/searchcore.cpp:740-881   batch alignment + sequential accept/reject bookkeeping
    search_acceptable_unaligned / _aligned   :541-609 / :664-737
    align_trim             core/searchcore.cpp:343-464   terminal-gap trimming, id0..id4
    search_joinhits / hit_compare_byid       :1028-1052 / :133-179
    search_topscores + unique_count + Dbindex + minheap order   (device: vsx_kmer.hip; host restatement kept as checker)
                           core/searchcore.cpp:260-340, core/unique.cpp:155-352, core/dbindex.cpp:163-255,
                           core/minheap.cpp:82-146
  and mirrors the reference's library entry points search_session_* / search_batch
  (core/search.hpp:88-145): one searcher per (database, options), batches of queries in, hit lists out.

  Control flow: instead of one search16 call of <= 8 targets per query, a WINDOW of queries advances in
  lock step -- every open query contributes its next delayed batch (exactly the targets the reference's
  align_delayed would pass to search16), all batches of the window go to the GPU as one vsx_plan, and the
  accept/reject counters are then replayed per query in the reference's order.  Every hit field is identical to
  the reference's; the set of aligned pairs is the reference's or (vsx_search_batch, r05: lazy first batches) a subset
  of it that leaves out only alignments the reference computes and frees unread.
*/
#ifndef VSX_SEARCH_H
#define VSX_SEARCH_H

#include "vsx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vsx_searcher vsx_searcher;

/* The Parameters fields this path reads (src/vsearch.h:224-540), with the reference's defaults after
   vsearch_apply_defaults_fixups (src/vsearch.cc:186-278).  Fill with vsx_search_opts_default() first. */
typedef struct vsx_search_opts {
  double  id;               /* --id (fraction, e.g. 0.9); required                               */
  double  weak_id;          /* --weak_id; default 10.0, clamped to id                             */
  int64_t maxaccepts;       /* 1;  0 = all                                                        */
  int64_t maxrejects;       /* 32; 0 = all                                                        */
  int64_t wordlength;       /* 8   (3..15)                                                        */
  int64_t minwordmatches;   /* -1 = table minwordmatches_defaults (core/searchcore.hpp:75-76)     */
  int32_t iddef;            /* 2                                                                  */
  int32_t soft_mask;        /* masking before the k-mer stage, of the DATABASE and -- unless qmask says otherwise -- of the queries
                               (--dbmask / --qmask; clustering masks everything by --qmask: pass it here; unique_count masks lower case for
                               every mode but "none", core/unique.cpp:198-199):
                                 0  none  lower case searchable
                                 1  soft  lower-case symbols are left out of the k-mers
                                 2  dust  the reference's DEFAULT: the database is DUST-masked on the device when the
                                          searcher is created (vsx_mask.hip), every query -- each strand on its own -- on the
                                          host threads (core/mask.cpp:79-199, core/search.cpp:294-303), then as 1.
                               All three stay on the device k-mer path (a per-symbol case bitmap beside the 4-bit codes);
                               the alignment itself never reads the case.  See `hardmask` below. */
  int64_t maxsubs, maxgaps, mincols, maxdiffs;
  double  query_cov, target_cov, maxid, mid;
  int32_t leftjust, rightjust;
  double  minqt, maxqt, minsl, maxsl;
  int64_t idprefix, idsuffix;
  int32_t selfid;
  int32_t threads;          /* host threads for the k-mer heuristic; 0 = all usable CPUs          */
  int64_t window;           /* queries advanced together; 0 = default (65536)                     */
  uint32_t gap_infinite;    /* '*' gap penalties (cli.cc:307-384): bit k = penalty k is infinite, k in the order of
                               vsx_scoring after match/mismatch (0..5 open q_l t_l q_i t_i q_r t_r, 6..11 extension);
                               an alignment using a forbidden gap class is rejected (searchcore.cpp:621-660) */
  uint32_t strand_both;     /* 0: --strand plus (default); 1: --strand both -- the reverse complement of every query is
                               searched as well (search.cpp:200-214), hits of both strands are joined (searchcore.cpp:1028-1052) */
  /* abundance-aware part of search_acceptable_unaligned (searchcore.cpp:541-609); abundances arrive through
     struct vsx_seq_meta; the caller resolves --sizein (the ';size=' annotation, or 1) */
  int64_t maxqsize;         /* --maxqsize, default INT64_MAX: query abundance above it -> every target rejected           */
  int64_t mintsize;         /* --mintsize, default 0                                                                    */
  double  minsizeratio;     /* --minsizeratio, default 0: query size >= ratio * target size (abundance_ratio_cmp :480)  */
  double  maxsizeratio;     /* --maxsizeratio, default DBL_MAX                                                          */
  int32_t self;             /* --self: a target whose label equals the query's label is rejected (needs labels)         */
  int32_t sizeorder;        /* --sizeorder (cluster_*): the member joins the most ABUNDANT accepted centroid
                               (hit_compare_bysize / search_findbest2_bysize, searchcore.cpp:182-243, :994-1025)        */
  int32_t cluster_unoise;   /* --cluster_unoise: UNOISE skew rule instead of the --id threshold in
                               search_acceptable_aligned (searchcore.cpp:701-718); weak_id is forced to 0.90 (cli.cc:4153) */
  int32_t qmask;            /* --qmask when it differs from --dbmask: 0 = the queries are masked as soft_mask says (default),
                               otherwise 1 + mode (1 none, 2 soft, 3 dust).  Searching only; clustering uses soft_mask */
  double  unoise_alpha;     /* --unoise_alpha, default 2.0                                                              */
  int32_t hardmask;         /* --hardmask (core/mask.cpp:137-191,248-271; core/search.cpp:294-303; commands/usearch_global.cpp,
                               core/cluster.cpp:1192-1197): masked symbols become 'N' IN THE SEQUENCE -- the k-mer stage and the
                               alignment both see them.  Bit 0: the database text handed to vsx_searcher_create (mode dust: the DUST
                               intervals become 'N' and the text keeps its case; mode soft: every lower-case symbol becomes 'N'; none:
                               nothing); bit 1: the queries, each strand on its own, by the query mask mode.  3 = the reference's command
                               line; 2 = a caller whose database is already hard-masked (the library API, shim/vsx_api_adapter.cpp).
                               Default 0.  Hits, %id and CIGARs then refer to the masked sequences, as in the reference. */
} vsx_search_opts;

void vsx_search_opts_default(vsx_search_opts * o);

/* One reported hit: the fields of `struct hit` (core/searchcore.hpp:78-126) that survive search_joinhits. */
typedef struct vsx_hit {
  uint32_t query;           /* index into the batch                                               */
  uint32_t target;          /* database sequence number                                           */
  uint32_t count;           /* shared unique k-mers (candidate rank key)                          */
  uint8_t  accepted, weak, used_fallback, strand;   /* strand: 0 = plus, 1 = minus (the query's reverse complement matched) */
  int32_t  nwscore, nwdiff, nwgaps, nwindels, nwalignmentlength;
  int32_t  matches, mismatches;
  int32_t  internal_alignmentlength, internal_gaps, internal_indels;
  int32_t  trim_q_left, trim_q_right, trim_t_left, trim_t_right;
  int32_t  shortest, longest;
  double   nwid, id, id0, id1, id2, id3, id4;
  uint64_t cigar_off;       /* into vsx_hits.cigar_blob (NUL-terminated)                          */
} vsx_hit;

typedef struct vsx_hits {
  uint64_t   n_queries;
  uint64_t   n_hits;
  uint64_t * first;         /* n_queries + 1: hits of query q are hit[first[q] .. first[q+1]), best first */
  vsx_hit  * hit;
  char     * cigar_blob;
  uint64_t   cigar_bytes;
  /* accounting.  pairs_aligned / cells_aligned: what reached the aligner.  vsx_search_batch aligns LAZILY since r05 -- a query's first batch is
     as many candidates as it still needs accepts (min(8, maxaccepts)) instead of the reference's 8, later batches are eights -- so the number
     is <= the pairs the reference passes to search16, with identical hits; VSX_SEARCH_LAZY=0 restores the reference's batches.
     allpairs and clustering align exactly the reference's pairs. */
  uint64_t   pairs_aligned, cells_aligned, stages, sentinel_pairs;
  double     seconds_kmer, seconds_align, seconds_total;
} vsx_hits;

/* Database + k-mer index (Database::add + Dbindex::prepare/add_all_sequences): n ASCII sequences.
   The sequences are also mirrored in HBM (vsx_seqset) for the aligner. */
int vsx_searcher_create(vsx_ctx * ctx, vsx_searcher ** out, const vsx_search_opts * opts,
                        uint64_t n, const char * blob, uint64_t blob_bytes,
                        const uint64_t * offsets, const uint32_t * lengths);
void vsx_searcher_destroy(vsx_searcher * s);
/* The database text AS INDEXED AND ALIGNED: the caller's blob with the searcher's masking applied (DUST: upper case with the masked
   A C G T U in lower case -- a masked ambiguity code stays upper case, no step reads its case; --hardmask: the masked symbols as 'N', core/mask.cpp:137-191,248-271).  What the reference prints as the target
   rows of --alnout after dust_all / hardmask_all rewrote the Database (db.hpp:179).  Copies min(cap, blob_bytes) bytes; returns blob_bytes. */
uint64_t vsx_searcher_db_text(const vsx_searcher * s, char * dst, uint64_t cap);

/* Per-sequence annotations the filters above read: Database::getabundance / getheader (core/db.hpp).  Either member may
   be NULL (abundances all 1, no labels).  The arrays are copied. */
typedef struct vsx_seq_meta {
  const uint64_t * abundance;       /* n values                                   */
  const char * const * label;       /* n NUL-terminated headers                   */
} vsx_seq_meta;
/* annotations of the searcher's database sequences (targets; in allpairs / clustering also the queries) */
int vsx_searcher_set_meta(vsx_searcher * s, const vsx_seq_meta * meta);

/* search_batch (core/search.hpp:131-145): every query against the database, --strand plus or both (opts.strand_both).
   Batches above 32 768 queries run as a pipeline of windows -- unique words (host threads) -> device k-mer counting + ranking (two
   workers) -> alignment, accept / reject replay and hit joining (two consumers; the second one on an aligner context of its own
   that the searcher creates on the same device and keeps) -- so one call uses several host threads and two contexts' worth of
   device scratch.  Results do not depend on the window size or the number of workers.  Not re-entrant per searcher. */
int vsx_search_batch(vsx_searcher * s, uint64_t n_queries, const char * qblob, uint64_t qblob_bytes,
                     const uint64_t * qoffsets, const uint32_t * qlengths, vsx_hits * out);
/* the same with the queries' annotations (si->qsize, si->query_head: core/search.cpp:88-94); qmeta may be NULL */
int vsx_search_batch_meta(vsx_searcher * s, uint64_t n_queries, const char * qblob, uint64_t qblob_bytes,
                          const uint64_t * qoffsets, const uint32_t * qlengths, const vsx_seq_meta * qmeta, vsx_hits * out);
void vsx_hits_free(vsx_hits * h);

/* ---- exact sequence search: --search_exact (commands/search_exact.cpp, core/dbhash.cpp; vsx_exact.cpp / vsx_exact.hip) ----
   A query strand matches a database sequence iff the lengths are equal and every position has the same 4-bit code
   (chrmap_4bit, utils/seqcmp.cpp): case-blind, U = T, an ambiguity code equals only itself.  The database is the searcher's text
   as indexed (vsx_searcher_db_text); the queries are masked per strand as vsx_search_batch masks them, which changes a result
   only with --hardmask (masked symbols are 'N').  EVERY match is evaluated: it passes search_acceptable_unaligned with the
   query's annotations and, as a finished hit with id 100, search_acceptable_aligned; the accepted ones are returned, ordered by
   target (a query that matches one target on both strands: plus first).  The hit is fixed: nwscore = qlen x match score,
   alignment length = matches = shortest = longest = qlen, no differences, every identity 100.0, CIGAR "<qlen>M".
   Honoured: strand_both, soft_mask / qmask / hardmask, the unaligned and aligned filters, self, window (queries per device
   window, 0 = 65 536), threads.  Ignored: id, weak_id, maxaccepts, maxrejects, wordlength, minwordmatches.
   The exact index -- code words of the database, their 64-bit hashes, an open-addressing table -- is built on the device by the
   first call and lives in the searcher; the k-mer index is not built.  A zero-length query or database sequence matches nothing.
   Environment: VSX_EXACT=host answers with the host restatement (a std::unordered_multimap over the code strings);
   VSX_EXACT_HASH_BITS=n (1 .. 64, read when the index is built) keeps the low n bits of every hash, so that chains of false
   candidates form and the comparison alone decides (tests).  Not re-entrant per searcher. */
int vsx_search_exact(vsx_searcher * s, uint64_t n_queries, const char * qblob, uint64_t qblob_bytes,
                     const uint64_t * offsets, const uint32_t * lengths, const vsx_seq_meta * meta /* may be NULL */, vsx_hits * out);
/* accounting of the calling thread's last vsx_search_exact */
typedef struct vsx_exact_stats {
  double   seconds_index;        /* index build; non-zero in the call that built it */
  double   seconds_stage;        /* masking and staging of the query windows (host) */
  double   seconds_kernel;       /* hash + probe kernels (device time) */
  double   seconds_marshal;      /* sorting, filters, hit records, the result's arrays */
  double   seconds_total;
  uint64_t windows;
  uint64_t queries_device, queries_host;      /* answered by the kernels / by the host restatement */
  uint64_t strands_probed, slots_visited, candidates_compared;
  uint64_t hits, queries_matched;             /* accepted hits, queries with at least one */
} vsx_exact_stats;
void vsx_search_exact_last_stats(vsx_exact_stats * out);
/* For tests / tooling: the host restatement of the whole call on a database given as text; no device, no context.  The database
   is masked as vsx_searcher_create masks it for --hardmask (without --hardmask no masking changes a match). */
int vsx_internal_search_exact_host(const vsx_scoring * scoring, const vsx_search_opts * opts, uint64_t n, const char * blob,
                                   uint64_t blob_bytes, const uint64_t * offsets, const uint32_t * lengths,
                                   const vsx_seq_meta * db_meta /* may be NULL */, uint64_t n_queries, const char * qblob,
                                   uint64_t qblob_bytes, const uint64_t * qoffsets, const uint32_t * qlengths,
                                   const vsx_seq_meta * qmeta /* may be NULL */, vsx_hits * out);

/* DUST-mask sequences in place, as dust() of the reference does (core/mask.cpp:127-199): everything upper case, the
   low-complexity intervals lower case.  Host threads (threads <= 0: all usable CPUs); sequences must not overlap.  What
   soft_mask = 2 applies to the queries; exported for callers that prepare their own text. */
int vsx_dust_mask(char * blob, uint64_t n, const uint64_t * offsets, const uint32_t * lengths, int32_t threads);

/* Sign of (value - ratio * reference) as the abundance filters compare it (--minsizeratio / --maxsizeratio / abskew;
   core/searchcore.cpp:480-537): the rounded double product while both abundances are below 2^53, exact integer arithmetic on
   the double's stored value beyond.  Host only; exported so that callers and tests can pin the boundary behaviour. */
int vsx_abundance_ratio_cmp(int64_t value, double ratio, int64_t reference);

/* allpairs_global (commands/allpairs_global.cpp:394-527): database sequences [first, first+count) as
   queries, each against every LATER sequence (unaligned filters applied unless acceptall); kept hits are
   those accepted (or all with acceptall), ordered id desc, target asc.  vsx_hit.query is the database
   sequence number.  Callers walk the database in blocks to bound the result size. */
int vsx_allpairs_block(vsx_searcher * s, int32_t acceptall, uint64_t first, uint64_t count, vsx_hits * out);
/* the same for an arbitrary ascending list of query rows -- the multi-GPU form: the triangular pair space is sharded by
   interleaved rows (vsearch_amd/sharding.py shard_allpairs_rows), every rank runs its rows against its DB replica.
   hits.first has count + 1 entries (entry k = rows[k]); vsx_hit.query is the database sequence number. */
int vsx_allpairs_rows(vsx_searcher * s, int32_t acceptall, const uint32_t * rows, uint64_t count, vsx_hits * out);
/* the whole command as one call (r05): rows first .. first + count - 1 in blocks of `block` queries (0 = 1 000), the stages of consecutive
   blocks overlapped -- while block i is on the GPU, block i + 1's pair list is enumerated and block i - 1's hits are completed on host
   threads.  `sink` receives each block's hits (those of vsx_allpairs_block(first + i * block, ...)), in order, from a helper thread, one
   call at a time; the hits belong to the library and are released when the sink returns.  A non-zero return of the sink stops the run
   and becomes the function's result.  The reference's worker threads report each query as it finishes (commands/allpairs_global.cpp:394-527). */
typedef int (*vsx_hits_sink)(void * user, uint64_t first, uint64_t count, const vsx_hits * hits);
int vsx_allpairs_stream(vsx_searcher * s, int32_t acceptall, uint64_t first, uint64_t count, uint64_t block, vsx_hits_sink sink, void * user);

/* ---- multi-device form: several GPUs of one node behind ONE handle (vsx_multi.cpp) ----------------------------------------
   The reference is one process with a pool of worker threads over a shared database (commands/usearch_global.cpp:500-535,
   core/search.cpp:397-508); here the pool is one aligner context + database replica + k-mer index per listed device and one
   host thread per device.  vsx_multi_search_batch cuts the batch into contiguous blocks of queries (one per device), runs
   vsx_search_batch_meta on each concurrently and merges the hit lists in the caller's query order: the result is what a single
   vsx_search_batch_meta of all queries returns, hit for hit (the accounting fields are summed, the times are the slowest
   device's).  vsx_multi_allpairs deals the rows first .. first + count - 1 of the triangular pair space out boustrophedon (balanced
   pairs and cells) and merges per row: the result of vsx_allpairs_block(first, count).  Clustering does not shard (sequential
   centroid dependency): use vsx_multi_searcher_replica(m, 0) with vsx_cluster_fast.  No collective is involved: the multi-PROCESS
   form with an RCCL gather is vsearch_amd/sharding.py.  A device may be listed more than once (several replicas on one GPU). */
typedef struct vsx_multi_searcher vsx_multi_searcher;
int vsx_multi_searcher_create(vsx_multi_searcher ** out, const vsx_scoring * scoring, const int32_t * devices, int32_t n_devices,
                              const vsx_search_opts * opts, uint64_t n, const char * blob, uint64_t blob_bytes,
                              const uint64_t * offsets, const uint32_t * lengths, const vsx_seq_meta * meta /* may be NULL */);
void vsx_multi_searcher_destroy(vsx_multi_searcher * m);
int32_t vsx_multi_searcher_devices(const vsx_multi_searcher * m);
vsx_searcher * vsx_multi_searcher_replica(vsx_multi_searcher * m, int32_t k);       /* owned by m */
int vsx_multi_search_batch(vsx_multi_searcher * m, uint64_t n_queries, const char * qblob, uint64_t qblob_bytes,
                           const uint64_t * qoffsets, const uint32_t * qlengths, const vsx_seq_meta * qmeta /* may be NULL */, vsx_hits * out);
int vsx_multi_allpairs(vsx_multi_searcher * m, int32_t acceptall, uint64_t first, uint64_t count, vsx_hits * out);

/* Candidate list of ONE query exactly as search_topscores + minheap_sort produce it (best first):
   fills up to `cap` (target, count) pairs, returns the number of candidates. For tests / tooling. */
int64_t vsx_search_candidates(vsx_searcher * s, const char * q, uint32_t qlen,
                              uint32_t * targets, uint32_t * counts, uint64_t cap);

/* Candidate lists of a BATCH of queries (search_topscores + heap order, core/searchcore.cpp:260-340,
   core/minheap.cpp:82-146): best first, at most maxaccepts + maxrejects + 8 per query.  device != 0 counts on the GPU
   (vsx_kmer.hip: tiled LDS counters over a device-resident index), 0 on host threads; both give identical lists.
   All arrays are malloc()'d; release with vsx_candidates_free. */
typedef struct vsx_candidates {
  uint64_t   n_queries;
  uint64_t * start;            /* n_queries + 1 */
  uint32_t * target;
  uint32_t * count;
  double     seconds;          /* wall time of the call (host k-mer extraction + counting + ranking) */
  double     kernel_ms;        /* device counting kernel(s), hipEvents; 0 on the host path */
  double     index_build_ms;   /* device index build, paid on first use */
  uint64_t   index_postings;   /* entries of the index */
  uint64_t   postings_streamed;/* counter increments of this call = postings read */
  uint64_t   bytes_streamed;   /* bytes of postings the count kernel read (the index format decides: 2 per posting, 4 tagged, 16 per packed unit) */
} vsx_candidates;
int vsx_search_candidates_batch(vsx_searcher * s, int32_t device, uint64_t n, const char * qblob, uint64_t qbytes,
                                const uint64_t * qoff, const uint32_t * qlen, vsx_candidates * out);
void vsx_candidates_free(vsx_candidates * c);

/* Greedy centroid clustering, --cluster_fast / --cluster_smallmem semantics (core/cluster.cpp:877-1125 with the
   intra-round fix-up evaluate_extra_hits :601-856): the searcher's sequences are processed IN THE GIVEN ORDER
   (sort them first: cluster_fast = length descending, core/db.cpp:433-450); each joins the cluster of its best
   accepted centroid hit or founds a new cluster.  `round` sequences are searched per GPU stage (0 = 16384); the
   result is independent of `round`.  hits.first[s]..first[s+1] holds the one hit of a member (target = its
   centroid) and is empty for centroids; clusterno[s] is the 0-based cluster number in creation order. */
typedef struct vsx_cluster_out {
  uint64_t   n;
  uint64_t   n_clusters;
  uint32_t * clusterno;
  vsx_hits   hits;
} vsx_cluster_out;
int vsx_cluster_fast(vsx_searcher * s, uint64_t round, vsx_cluster_out * out);
void vsx_cluster_out_free(vsx_cluster_out * o);

/* Star multiple alignment / profile / consensus of ONE cluster from the members' CIGARs (core/msa.cpp:569-613;
   no DP).  seqs[0] is the centroid (cigars[0] ignored), members follow with the CIGAR of (query = member,
   target = centroid) exactly as vsx_cluster_fast reports it.  rows: n_rows = n + 1 NUL-terminated strings of alnlen
   columns each (centroid, members, then the consensus row with '+' outside the centroid and '-' where gaps win);
   profile: alnlen x 6 counts in the order A C G T N gap (msa.cpp:92-141); consensus: the un-gapped majority sequence. */
typedef struct vsx_msa_out {
  uint64_t   alnlen, n_rows, conslen;
  char     * rows;
  char     * consensus;
  uint64_t * profile;
} vsx_msa_out;
int vsx_msa(uint32_t n, const char * const * seqs, const uint32_t * lens, const char * const * cigars,
            const uint64_t * abundances /* NULL = all 1 */, vsx_msa_out * out);
void vsx_msa_out_free(vsx_msa_out * o);
/* The same on the device (vsx_msa.hip), for one cluster or for many in one pass: cluster c owns entries
   cluster_start[c] .. cluster_start[c+1]-1 of seqs/lens/cigars/abundances (first entry = its centroid, whose cigar is
   ignored); outs[c] receives what vsx_msa would return for it (byte-identical; free each with vsx_msa_out_free).
   The CIGAR text is parsed and max-insertions/column offsets are computed on the host (O(runs)); the O(rows x alnlen)
   work -- row fill, profile, consensus row -- runs in three kernels.  Fails (VSX_EINVAL) on what vsx_msa rejects and on
   two adjacent 'D' runs; no CPU fallback. */
int vsx_msa_device(vsx_ctx * ctx, uint32_t n, const char * const * seqs, const uint32_t * lens, const char * const * cigars,
                   const uint64_t * abundances /* NULL = all 1 */, vsx_msa_out * out);
int vsx_msa_device_batch(vsx_ctx * ctx, uint32_t n_clusters, const uint64_t * cluster_start /* n_clusters + 1 */,
                         const char * const * seqs, const uint32_t * lens, const char * const * cigars,
                         const uint64_t * abundances /* NULL = all 1 */, vsx_msa_out * outs /* n_clusters */);

/* ---- reference-based chimera detection: --uchime_ref with the default UCHIME algorithm (vsx_chimera.cpp / vsx_chimera.hip) ----
   Per query (chimera_process_query, core/chimera.cpp:2003-2170): the query is cut into 4 parts (partition_query :1930-1955), every
   part is searched like a --usearch_global query (id 0.55, maxaccepts 4, maxrejects 16; each part masked on its own), the ACCEPTED
   hits of the parts -- part by part, best first, repeated targets dropped -- are the candidate parents, the whole query is aligned
   globally with each of them, and find_best_parents (:627-751) + eval_parents (:1245-1700) pick two parents and score the query.
   Parent selection and scoring run in one kernel (one workgroup per query) that reads the alignments' run words where the
   traceback left them; queries above VSX_CHIMERA_MAX_QLEN, and queries with a candidate the 16-bit aligner refused (realigned with
   vsx_lma_align), are answered by a host restatement of the same two functions.  Plus strand only (the reference refuses
   --strand both here).  The de novo forms (--uchime_denovo / uchime2 / uchime3) are vsx_uchime_denovo below, the long-read
   detector --chimeras_denovo is vsx_chimeras_denovo.  The --uchimealns text of the records of vsx_uchime_ref / vsx_uchime_denovo is
   a call of its own, declared in vsx_chimalns.h.  Not covered: the --alnout text of --chimeras_denovo. */
typedef struct vsx_chimera_opts {
  vsx_search_opts search;   /* the searcher's options: masking, hardmask, wordlength, threads, window (of the part search) and the
                               detection parameters id = weak_id = 0.55, maxaccepts 4, maxrejects 16.  As in the reference, the
                               query parts are searched as given: qmask dust / soft mask their lower-case symbols for the k-mers,
                               none does not, and neither DUST nor --hardmask rewrites a query (search_onequery, chimera.cpp:2023) */
  double  minh;             /* --minh,     default 0.28 */
  double  mindiv;           /* --mindiv,   default 0.8  */
  int64_t mindiffs;         /* --mindiffs, default 3    */
  double  xn;               /* --xn,       default 8.0  */
  double  dn;               /* --dn,       default 1.4  */
  int64_t window;           /* queries per chimera window (parts searched, aligned and evaluated together); 0 = 16 384 */
} vsx_chimera_opts;
/* the defaults of src/vsearch.h:420-484 and the detection parameters of chimera_detection_parameters (chimera.cpp:2805-2824) */
void vsx_chimera_opts_default(vsx_chimera_opts * o);

#define VSX_CHIMERA_MAX_QLEN 4096   /* longest query the evaluation kernel takes (its LDS layout); longer ones: host restatement */

#define VSX_CHIMERA_NO_PARENTS   0  /* fewer than two parents found: Status::no_parents                          */
#define VSX_CHIMERA_NO_ALIGNMENT 1  /* two parents, but no column gave an h score: Status::no_alignment          */
#define VSX_CHIMERA_SCORED       2  /* scored: flag is 'Y' (chimeric), '?' (suspicious) or 'N' (low score)        */
/* The fields of chimera_result_s (core/chimera.hpp:72-87) with parents as database indices (UINT32_MAX = none); the caller resolves
   labels.  Unless status == VSX_CHIMERA_SCORED the record is zero except status, flag 'N' and the parents found. */
typedef struct vsx_chimera_result {
  double   score;                                     /* h */
  uint32_t parent_a, parent_b, closest;
  int32_t  status;
  double   id_query_model, id_query_a, id_query_b, id_a_b, id_query_top;   /* QM QA QB AB QT, percent */
  int32_t  left_yes, left_no, left_abstain;
  int32_t  right_yes, right_no, right_abstain;
  double   divergence;                                /* QM - QT */
  char     flag;                                      /* 'Y', 'N' or '?' */
  char     pad[7];
} vsx_chimera_result;

/* n queries (ASCII) against the searcher's database; out[k] = query k.  The searcher must have been created from
   vsx_chimera_opts_default's `search` (id = weak_id = 0.55, maxaccepts 4, maxrejects 16, plus strand): VSX_EINVAL otherwise.
   VSX_CHIMERA=host in the environment answers every query with the host restatement (A/B, tests). */
int vsx_uchime_ref(vsx_searcher * s, const vsx_chimera_opts * opts, uint64_t n, const char * qblob, uint64_t qbytes,
                   const uint64_t * qoff, const uint32_t * qlen, vsx_chimera_result * out);
/* accounting of the calling thread's last vsx_uchime_ref */
typedef struct vsx_chimera_stats {
  double   seconds_search, seconds_align, seconds_eval, seconds_total;   /* part search / whole-query alignment / selection + scoring */
  uint64_t windows, parts, pairs_aligned, sentinel_pairs;
  uint64_t queries_kernel, queries_host;              /* answered by the evaluation kernel / the host restatement */
} vsx_chimera_stats;
void vsx_chimera_last_stats(vsx_chimera_stats * out);

/* ---- de novo chimera detection: --uchime_denovo, --uchime2_denovo, --uchime3_denovo (vsx_chimera.cpp) ----
   The searcher's own sequences are both the queries and the database, processed IN THE GIVEN ORDER: sort them first as
   Database::sortbyabundance does (abundance descending, then strcmp of the header, then input order; core/db.cpp:471-485) and mask
   them through the searcher's soft_mask / hardmask the way --qmask / --hardmask mask the de novo input (chimera.cpp:2546-2555).
   Abundances and labels come from vsx_searcher_set_meta (abundances are required; labels drive --self).  Query i is searched
   against the sequences before it that were neither chimeric nor borderline (chimera.cpp:2365-2372), with the detection
   parameters plus self = selfid = 1 and maxsizeratio = 1 / abskew (a candidate less than abskew times as abundant as the query is
   rejected unaligned, and still takes a slot of the candidate loop).  The verdict is the UCHIME rule for variant 1 and, for
   variants 2 and 3, 'Y' iff the model matches the query on every column and the closest parent does not (chimera.cpp:1633-1640).
   The queries run in windows (base.window, 0 = 4 096) of speculative passes with an in-order fix-up; the result does not depend
   on the window.  Word lengths 3..8 only (the growing index is a pair of device subset indexes); plus strand only. */
typedef struct vsx_chimera_denovo_opts {
  vsx_chimera_opts base;    /* minh, mindiv, mindiffs, xn, dn, window (queries per speculative window) and the searcher's options */
  int32_t variant;          /* 1 = --uchime_denovo, 2 = --uchime2_denovo, 3 = --uchime3_denovo */
  double  abskew;           /* >= 1.0 */
} vsx_chimera_denovo_opts;
/* vsx_chimera_opts_default + abskew 2 / 2 / 16 (cli.cc:4478-4492), search.self = search.selfid = 1 and
   search.maxsizeratio = 1 / abskew (chimera_detection_parameters, chimera.cpp:2805-2824) */
void vsx_chimera_denovo_opts_default(vsx_chimera_denovo_opts * o, int32_t variant);
/* out[k] = the searcher's sequence k (one record per sequence).  VSX_EINVAL: a searcher not created with the options above
   (maxsizeratio must equal 1 / abskew), --strand both, no abundances, a word length above 8, a variant outside 1..3, abskew < 1.
   VSX_CHIMERA=host answers every query with the host restatement. */
int vsx_uchime_denovo(vsx_searcher * s, const vsx_chimera_denovo_opts * opts, vsx_chimera_result * out);
/* accounting of the calling thread's last vsx_uchime_denovo */
typedef struct vsx_chimera_denovo_stats {
  double   seconds_rank;                /* parts ranked against the committed non-chimeras (device main + delta indexes) */
  double   seconds_members;             /* parts counted against the window's own members (device window index) */
  double   seconds_search;              /* staged accept / reject replay of the parts */
  double   seconds_align;               /* whole queries against their candidate parents */
  double   seconds_eval;                /* parent selection + scoring (kernel and host restatement) */
  double   seconds_reconcile;           /* merging the candidate lists, in-order validation */
  double   seconds_total;
  uint64_t windows, passes, passes_max; /* passes over all windows, and the most of one window */
  uint64_t queries_reevaluated;         /* queries searched and evaluated more than once */
  uint64_t parts, pairs_searched, pairs_aligned, sentinel_pairs;   /* part-target pairs of the search, whole-query pairs */
  uint64_t queries_kernel, queries_host;                           /* evaluations by the kernel / the host restatement */
} vsx_chimera_denovo_stats;
void vsx_chimera_denovo_last_stats(vsx_chimera_denovo_stats * out);

/* ---- de novo chimera detection in long, high-quality reads: --chimeras_denovo (vsx_chimera.cpp / vsx_chimera_long.hip) ----
   The loop is vsx_uchime_denovo's (abundance-sorted input, growing index of the queries that were not chimeric, windows of
   speculative passes), with three differences (chimera_process_query, core/chimera.cpp:2003-2170):
     parts       (length + 99) / 100, or `parts` when given, clamped to 2 .. 100 (realloc_arrays :285-299); a query shorter than its
                 part count is not searched.  The candidates are the accepted hits of all parts, repeated targets dropped: up to
                 maxaccepts x parts of them
     selection   find_best_parents_long (:505-624): up to parents_max rounds; each round takes, over the candidates in list order,
                 the longest stretch of still unused query positions, uninterrupted by an insertion, in which the candidate matches
                 (a non-zero AND of the 4-bit codes) with at most diff_pct percent mismatches; it must reach length_min.  The query
                 is chimeric iff at least two such regions were found and they cover every position
     evaluation  eval_parents_long (:995-1242): the identity of the query with each parent over the columns of the multiple
                 alignment (query length + the longest insertion in front of each position), equal 4-bit codes counting as matches
   Selection and evaluation run in one kernel (one workgroup per query) over the run words the traceback left in HBM.
   The kernel takes a query iff
     - its length is at most VSX_CHIMERAS_LONG_MAX_QLEN and it has at most VSX_CHIMERAS_LONG_MAX_CAND candidates,
     - the 16-bit aligner refused none of its candidates, and
     - diff_pct * 2^13 is an integer (0, 1, 2.5, 0.125, ...; not 0.1).  The reference scans a segment with sums of doubles, diff_pct
       per match and diff_pct - 100 per mismatch; for such a percentage every partial sum over <= 2 048 positions is a multiple of
       2^-13 below 2^18, exactly representable, so the kernel forms the same sums as 32-bit integers in units of 2^-13 (they stay
       below 2^31) and the order of addition cannot matter.  With diff_pct = 0 a region is simply a run of matching positions.
       For any other percentage the sums are formed in the reference's order by the host restatement only.
   Every other query is answered by the host restatement of the same two functions (also under VSX_CHIMERA=host). */
#define VSX_CHIMERAS_LONG_MAX_PARENTS 20    /* maxparents (chimera.cpp:111) */
#define VSX_CHIMERAS_LONG_MAX_QLEN    2048  /* longest query the long-read kernel takes (its LDS layout) */
#define VSX_CHIMERAS_LONG_MAX_CAND    64    /* most candidates of one query the long-read kernel takes (its LDS layout) */
#define VSX_CHIMERA_CHIMERIC          3     /* vsx_chimeras_long_result.status: Status::chimeric (the other value is NO_PARENTS) */
typedef struct vsx_chimeras_long_opts {
  vsx_search_opts search;   /* as vsx_chimera_denovo_opts.base.search: id = weak_id = 0.55, maxaccepts 4, maxrejects 16, self = selfid = 1,
                               maxsizeratio = 1 / abskew */
  int32_t parts;            /* --chimeras_parts: 0 = by length, else 2 .. 100 */
  int32_t parents_max;      /* --chimeras_parents_max: 2 .. 20, default 3 */
  int32_t length_min;       /* --chimeras_length_min: >= 1, default 10 */
  int32_t pad;
  double  diff_pct;         /* --chimeras_diff_pct: 0.0 .. 50.0, default 0.0 */
  double  abskew;           /* --abskew: >= 1.0, default 1.0 for this command (cli.cc:4481-4484) */
  int64_t window;           /* queries per speculative window; 0 = 4 096 */
} vsx_chimeras_long_opts;
void vsx_chimeras_long_opts_default(vsx_chimeras_long_opts * o);
/* One record per sequence.  parent / start / len [0 .. n_parents) are the regions found, sorted by start (database indices; the same
   sequence may appear twice); they are filled for a query that is not chimeric, too (fewer than two regions, or a position left
   uncovered).  The identities, alnlen and the divergence are set for chimeric queries only. */
typedef struct vsx_chimeras_long_result {
  int32_t  status;                                           /* VSX_CHIMERA_NO_PARENTS or VSX_CHIMERA_CHIMERIC */
  char     flag;                                             /* 'Y' or 'N' */
  char     pad[3];
  int32_t  n_parents;
  int32_t  alnlen;                                           /* query length + the longest insertion in front of each position */
  uint32_t parent[VSX_CHIMERAS_LONG_MAX_PARENTS];
  int32_t  start[VSX_CHIMERAS_LONG_MAX_PARENTS];
  int32_t  len[VSX_CHIMERAS_LONG_MAX_PARENTS];
  double   id_query_parent[VSX_CHIMERAS_LONG_MAX_PARENTS];   /* QA, QB, QC, ...: 100 * equal columns / alnlen */
  double   id_query_top;                                     /* QT = the largest of them */
  double   divergence;                                       /* 100 * (100 - QT) / QT */
} vsx_chimeras_long_result;
/* out[k] = the searcher's sequence k.  Preconditions as vsx_uchime_denovo: sequences pre-sorted by abundance, abundances set, word
   length <= 8, plus strand.  VSX_EINVAL: an option outside its range (cli.cc:4390-4411: length_min < 1, parents_max outside 2 .. 20,
   diff_pct outside 0 .. 50, parts neither 0 nor 2 .. 100), abskew < 1, a searcher not created with the options above.
   VSX_CHIMERA=host answers every query with the host restatement. */
int vsx_chimeras_denovo(vsx_searcher * s, const vsx_chimeras_long_opts * opts, vsx_chimeras_long_result * out);
/* accounting of the calling thread's last vsx_chimeras_denovo (the fields of vsx_uchime_denovo's) */
void vsx_chimeras_denovo_last_stats(vsx_chimera_denovo_stats * out);
/* For tests / tooling: the host restatement on ONE query and nc candidates given as text with their alignments (CIGAR text, query
   against candidate, as vsx_lma_align writes it); no device.  The record's parents are candidate numbers 0 .. nc - 1.  Only the
   selection and evaluation options of `opts` are read (and range-checked as above). */
int vsx_internal_chimeras_long_host(const char * q, uint32_t qlen, uint32_t nc, const char * const * t, const uint32_t * tlen,
                                    const char * const * cigars, const vsx_chimeras_long_opts * opts, vsx_chimeras_long_result * out);

/* The scalar fallback the callers run on the SHRT_MAX sentinel: LinearMemoryAligner::align + alignstats
   (core/linmemalign.cpp:694-808; call sites core/searchcore.cpp:806-832, commands/allpairs_global.cpp:447-473).
   Host CPU, int64 arithmetic, linear memory, the reference's tie-breaks; uses the UNclamped scoring values
   (scoring_from_options, linmemalign.cpp:99-118).  *cigar is malloc'ed. */
int vsx_lma_align(const vsx_scoring * scoring, const char * q, uint64_t qlen, const char * t, uint64_t tlen,
                  int64_t * score, int64_t * alnlen, int64_t * matches, int64_t * mismatches,
                  int64_t * gaps, char ** cigar);

#ifdef __cplusplus
}
#endif
#endif
