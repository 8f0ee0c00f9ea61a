// vsx_fetch.cpp -- host side of libvsx, result marshalling: settle a plan's run and text buffers, fetch (plain and ranked), the
// exports into device memory, run words -> CIGAR text.  See vsx_context.cpp for the layout of the host layer.
#include "vsx_host_internal.h"

using vsxp::fail;
using namespace vsxh;

static void append_cigar(std::string & s, const uint32_t * runs, uint32_t n)
{
  // runs are in traceback order (last column first); the text runs left to right,
  // count omitted when 1 (pushop/finishop, align_simd.cpp:1013-1049)
  static const char ops[4] = {'M', 'I', 'D', '?'};
  char buf[16];
  for (uint32_t k = n; k-- > 0;)
    {
      const uint32_t len = runs[k] >> 2;
      if (len > 1) { int w = snprintf(buf, sizeof buf, "%u", len); s.append(buf, (size_t) w); }
      s.push_back(ops[runs[k] & 3]);
    }
}

// wait for a plan's kernels; run the whole plan again if its run buffer overflowed (the fetches and the exports share this)
static int settle_runs(vsx_plan * pl, unsigned long long & used, unsigned long long & text_used)
{
  vsx_ctx * ctx = pl->ctx;
  if (!pl->ran) { int rc = vsx_plan_run(pl); if (rc != VSX_OK) return rc; }
  int rc = vsx_plan_sync(pl, nullptr);
  if (rc != VSX_OK) return rc;
  VSX_HIP(hipSetDevice(ctx->device));
  used = pl->h_cursor[0]; text_used = pl->h_cursor[1];
  if (used > pl->runs_capacity)
    {
      // the dense run buffer was sized for typical alignments; size it exactly and run again
      pl->runs_capacity = used + 1;
      VSX_HIP(pl->d_runs.alloc(&pl->ctx->pool, pl->runs_capacity));
      ctx->settle_counts[0].fetch_add(1);
      if ((rc = vsx_plan_run(pl)) != VSX_OK) return rc;
      if ((rc = vsx_plan_sync(pl, nullptr)) != VSX_OK) return rc;
      used = pl->h_cursor[0]; text_used = pl->h_cursor[1];
      if (used > pl->runs_capacity) return fail(VSX_EHIP, "vsx_plan: run buffer overflow after resize");          // (fetches and exports alike)
    }
  return VSX_OK;
}

// settle_runs(), then the same for the text buffer: only the formatting kernel runs again
static int settle(vsx_plan * pl, unsigned long long & used, unsigned long long & text_used)
{
  vsx_ctx * ctx = pl->ctx;
  int rc = settle_runs(pl, used, text_used);
  if (rc != VSX_OK) return rc;
  hipStream_t st = ctx->stream;
  if (text_used > pl->text_capacity)
    {
      // same for the text: only the formatting kernel runs again
      pl->text_capacity = text_used + 16;
      VSX_HIP(pl->d_text.alloc(&pl->ctx->pool, pl->text_capacity));
      ctx->settle_counts[1].fetch_add(1);
      VSX_HIP(hipMemsetAsync(pl->d_cursor.p + 1, 0, sizeof(unsigned long long), st));
      VSX_HIP(vsx_launch_cigar_text(pl->d_out.p, pl->d_pair_ids.p, (uint32_t) pl->pair_ids.size(), pl->d_runs.p, pl->runs_capacity,
                                   pl->d_text.p, pl->text_capacity, pl->d_cursor.p + 1, pl->soa, st));
      VSX_HIP(hipMemcpyAsync(pl->h_cursor, pl->d_cursor.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
      VSX_HIP(hipStreamSynchronize(st));
      text_used = pl->h_cursor[1];
      if (text_used > pl->text_capacity) return fail(VSX_EHIP, "vsx_plan_fetch: text buffer overflow after resize");
    }
  return VSX_OK;
}

// pinned staging of at least `need` bytes (caller holds ctx->stage_mu)
static int stage_reserve(vsx_ctx * ctx, uint64_t need)
{
  if (need <= ctx->stage_bytes) return VSX_OK;
  if (ctx->stage) { (void) hipHostFree(ctx->stage); ctx->stage = nullptr; ctx->stage_bytes = 0; }
  const uint64_t want = need + need / 4 + (1u << 20);
  if (hipHostMalloc(reinterpret_cast<void **>(&ctx->stage), want, hipHostMallocDefault) != hipSuccess)
    { (void) hipGetLastError(); return fail(VSX_ENOMEM, "vsx_plan_fetch: pinned staging allocation failed"); }
  ctx->stage_bytes = want;
  return VSX_OK;
}

int vsxh::fetch_core(vsx_plan * pl, const FetchDest & D)
{
  vsx_ctx * ctx = pl->ctx;
  unsigned long long used = 0, text_used = 0;
  int rc = settle(pl, used, text_used);
  if (rc != VSX_OK) return rc;

  const uint64_t n = pl->n_pairs;
  // the rare pairs answered on the host get their strings behind the device text
  uint64_t tail = 0;
  for (size_t h = 0, hc = 0; h < pl->host_pairs.size(); ++h)
    {
      ++tail;
      if (hc < pl->host_cigar_pair.size() && pl->host_cigar_pair[hc] == pl->host_pairs[h]) tail += pl->host_cigar[hc++].size();
    }
  const uint64_t base = *D.blob_used;
  {
    char * nb = (char *) std::realloc(*D.blob, std::max<uint64_t>(base + text_used + tail, 1));
    if (!nb) return fail(VSX_ENOMEM, "vsx_plan_fetch: host allocation failed");
    *D.blob = nb;
  }
  char * const blob = *D.blob;

  {
    // one PCIe crossing into pinned memory (arrays + text), then host threads spread it over the result arrays
    std::lock_guard<std::mutex> lk(ctx->stage_mu);
    if ((rc = stage_reserve(ctx, pl->soa_bytes + ((text_used + 15) & ~15ull))) != VSX_OK) return rc;
    hipError_t e = hipSuccess;
    // (the plan's kernels are done -- vsx_plan_sync above -- so the copies need no ordering against `stream`, where the next
    //  slice of a pipeline may already be running)
    if (n) e = hipMemcpyAsync(ctx->stage, pl->d_soa.p, pl->soa_bytes, hipMemcpyDeviceToHost, ctx->stream_dn);
    if (e == hipSuccess && text_used) e = hipMemcpyAsync(ctx->stage + pl->soa_bytes, pl->d_text.p, text_used, hipMemcpyDeviceToHost, ctx->stream_dn);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream_dn);
    if (e != hipSuccess) return fail(VSX_EHIP, "vsx_plan_fetch: %s", hipGetErrorString(e));
    const uint8_t * sg = ctx->stage;
    const int nth = copy_threads(n * 19 + text_used);
    run_threads(nth, [&](int t) {
      const auto [lo, hi] = slice_of(n, t, nth);
      if (hi > lo)
        {
          std::memcpy(D.score + lo, sg + pl->soa_off[0] + 2 * lo, 2 * (hi - lo));
          std::memcpy(D.aligned + lo, sg + pl->soa_off[1] + 2 * lo, 2 * (hi - lo));
          std::memcpy(D.matches + lo, sg + pl->soa_off[2] + 2 * lo, 2 * (hi - lo));
          std::memcpy(D.mismatches + lo, sg + pl->soa_off[3] + 2 * lo, 2 * (hi - lo));
          std::memcpy(D.gaps + lo, sg + pl->soa_off[4] + 2 * lo, 2 * (hi - lo));
          if (D.verdict) std::memcpy(D.verdict + lo, sg + pl->soa_off[5] + lo, hi - lo);
          const uint64_t * so = reinterpret_cast<const uint64_t *>(sg + pl->soa_off[6]);
          for (uint64_t k = lo; k < hi; ++k) D.cigar_off[k] = so[k] + base;
        }
      const auto [blo, bhi] = slice_of(text_used, t, nth);
      if (bhi > blo) std::memcpy(blob + base + blo, sg + pl->soa_bytes + blo, bhi - blo);
    });
  }
  uint64_t at = base + text_used;
  for (size_t h = 0, hc = 0; h < pl->host_pairs.size(); ++h)
    {
      const uint32_t k = pl->host_pairs[h];
      const VsxPairOut & o = pl->host_out[h];
      D.score[k] = o.score; D.aligned[k] = o.aligned; D.matches[k] = o.matches;
      D.mismatches[k] = o.mismatches; D.gaps[k] = o.gaps;
      if (D.verdict) D.verdict[k] = (uint8_t) VSX_VERDICT_UNDECIDED;
      D.cigar_off[k] = at;
      if (hc < pl->host_cigar_pair.size() && pl->host_cigar_pair[hc] == k)
        {
          std::memcpy(blob + at, pl->host_cigar[hc].data(), pl->host_cigar[hc].size());
          at += pl->host_cigar[hc++].size();
        }
      blob[at++] = '\0';
    }
  *D.blob_used = at;
  return VSX_OK;
}

// r06: the ranked fetch from the lists the traceback's epilogue wrote.  Kept pairs arrive in arbitrary order: their fields are gathered
// as they lie, cross PCIe, and the HOST puts the few of them in report order -- per run of equal query keys (runs in pair order; the
// pairs of a query are documented to be contiguous, so a run is a query), identity descending, pair index ascending among equals.
static int fetch_ranked_lists(vsx_plan * pl, uint64_t first, const uint32_t * qkey, RankedSink & S, unsigned long long text_used)
{
  vsx_ctx * ctx = pl->ctx;
  hipStream_t st = ctx->stream_dn;
  const uint64_t n = pl->n_pairs;
  uint32_t counts[2] = {0, 0};
  VSX_HIP(hipMemcpyAsync(counts, pl->d_rank_counts.p, sizeof counts, hipMemcpyDeviceToHost, st));
  VSX_HIP(hipStreamSynchronize(st));
  const uint32_t kept = counts[0], n_refused = counts[1];
  if (kept > n || n_refused > n) return fail(VSX_EHIP, "vsx_align_pairs_ranked: the kept / refused lists are corrupt");
  if (n_refused)
    {
      // (include/vsx.h: a pair the 16-bit aligner refused is `undecided`, never silently dropped)
      std::vector<uint32_t> rf(n_refused);
      VSX_HIP(hipMemcpy(rf.data(), pl->d_refused_pair.p, (size_t) n_refused * 4, hipMemcpyDeviceToHost));
      std::sort(rf.begin(), rf.end());
      for (uint32_t k : rf) S.undecided.push_back((uint32_t) (first + k));
    }
  if (!kept) return VSX_OK;
  const uint64_t width[9] = {4, 8, 8, 2, 2, 2, 2, 2, 1};
  uint64_t off[9], at = 0;
  for (int x = 0; x < 9; ++x) { off[x] = at; at += ((uint64_t) kept * width[x] + 15) & ~15ull; }
  const uint64_t rank_bytes = at;
  PoolBuf<uint8_t> d_rank;
  VSX_HIP(d_rank.alloc(&ctx->pool, rank_bytes));
  VsxRankedOut R;
  R.pair = reinterpret_cast<uint32_t *>(d_rank.p + off[0]);
  R.id = reinterpret_cast<double *>(d_rank.p + off[1]);
  R.text_off = reinterpret_cast<uint64_t *>(d_rank.p + off[2]);
  R.score = reinterpret_cast<int16_t *>(d_rank.p + off[3]);
  R.aligned = reinterpret_cast<uint16_t *>(d_rank.p + off[4]);
  R.matches = reinterpret_cast<uint16_t *>(d_rank.p + off[5]);
  R.mismatches = reinterpret_cast<uint16_t *>(d_rank.p + off[6]);
  R.gaps = reinterpret_cast<uint16_t *>(d_rank.p + off[7]);
  R.verdict = d_rank.p + off[8];
  VSX_HIP(vsx_rank_gather_list(pl->d_kept_pair.p, pl->d_kept_id.p, kept, pl->d_out.p, pl->soa.text_off, R, st));
  std::lock_guard<std::mutex> lk(ctx->stage_mu);
  int rc = stage_reserve(ctx, rank_bytes + ((text_used + 15) & ~15ull));
  if (rc != VSX_OK) return rc;
  VSX_HIP(hipMemcpyAsync(ctx->stage, d_rank.p, rank_bytes, hipMemcpyDeviceToHost, st));
  if (text_used) VSX_HIP(hipMemcpyAsync(ctx->stage + rank_bytes, pl->d_text.p, text_used, hipMemcpyDeviceToHost, st));
  VSX_HIP(hipStreamSynchronize(st));
  const uint8_t * sg = ctx->stage;
  const char * text = reinterpret_cast<const char *>(sg + rank_bytes);
  const uint32_t * h_pair = reinterpret_cast<const uint32_t *>(sg + off[0]);
  const double * h_id = reinterpret_cast<const double *>(sg + off[1]);
  const uint64_t * h_toff = reinterpret_cast<const uint64_t *>(sg + off[2]);
  const int16_t * h_score = reinterpret_cast<const int16_t *>(sg + off[3]);
  const uint16_t * h_al = reinterpret_cast<const uint16_t *>(sg + off[4]), * h_ma = reinterpret_cast<const uint16_t *>(sg + off[5]);
  const uint16_t * h_mi = reinterpret_cast<const uint16_t *>(sg + off[6]), * h_ga = reinterpret_cast<const uint16_t *>(sg + off[7]);
  const uint8_t * h_vd = sg + off[8];
  std::vector<uint32_t> order;
  order.reserve(kept);
  for (uint32_t j = 0; j < kept; ++j)
    {
      if (h_pair[j] >= n) return fail(VSX_EHIP, "vsx_align_pairs_ranked: a kept pair is out of range");
      if (h_vd[j] == 1u || (S.keep_weak && h_vd[j] == 2u)) order.push_back(j);
    }
  // segment of each plan-local pair: a new one wherever the query key changes (a strict weak order for every key list)
  std::vector<uint32_t> seg((size_t) n);
  for (uint64_t k = 1; k < n; ++k) seg[k] = seg[k - 1] + (qkey[k] != qkey[k - 1] ? 1u : 0u);
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    const uint32_t pa = h_pair[a], pb = h_pair[b];
    if (seg[pa] != seg[pb]) return seg[pa] < seg[pb];
    if (h_id[a] != h_id[b]) return h_id[a] > h_id[b];
    return pa < pb;
  });
  const size_t m = order.size(), base = S.pair.size();
  S.pair.resize(base + m); S.id.resize(base + m); S.cigar_off.resize(base + m);
  S.score.resize(base + m); S.aligned.resize(base + m); S.matches.resize(base + m);
  S.mismatches.resize(base + m); S.gaps.resize(base + m); S.verdict.resize(base + m);
  uint64_t need = 0;
  std::vector<uint32_t> slen(m);
  for (size_t x = 0; x < m; ++x) { slen[x] = (uint32_t) std::strlen(text + h_toff[order[x]]) + 1; need += slen[x]; }
  char * nb = (char *) std::realloc(S.blob, std::max<uint64_t>(S.blob_used + need, 1));
  if (!nb) return fail(VSX_ENOMEM, "vsx_align_pairs_ranked: host allocation failed");
  S.blob = nb;
  for (size_t x = 0; x < m; ++x)
    {
      const uint32_t j = order[x];
      S.pair[base + x] = (uint32_t) (first + h_pair[j]);
      S.id[base + x] = h_id[j];
      S.score[base + x] = h_score[j]; S.aligned[base + x] = h_al[j]; S.matches[base + x] = h_ma[j];
      S.mismatches[base + x] = h_mi[j]; S.gaps[base + x] = h_ga[j]; S.verdict[base + x] = h_vd[j];
      S.cigar_off[base + x] = S.blob_used;
      std::memcpy(S.blob + S.blob_used, text + h_toff[j], slen[x]);
      S.blob_used += slen[x];
    }
  return VSX_OK;
}

// `first` = index of the plan's pair 0 in the caller's list; `qkey` = the caller's query index per pair (plan-local view)
int vsxh::fetch_ranked_core(vsx_plan * pl, uint64_t first, const uint32_t * qkey, RankedSink & S)
{
  unsigned long long used = 0, text_used = 0;
  int rc = settle(pl, used, text_used);
  if (rc != VSX_OK) return rc;
  const uint64_t n = pl->n_pairs;
  for (uint32_t k : pl->host_pairs) S.undecided.push_back((uint32_t) (first + k));
  if (n == 0) return VSX_OK;
  // (every ranked plan has its lists: vsx_align_pairs_ranked requires the filter, plan_set_ranked() follows it)
  if (!pl->filter.rank_counts) return fail(VSX_EINVAL, "vsx_align_pairs_ranked: the plan has no ranking lists");
  return fetch_ranked_lists(pl, first, qkey, S, text_used);
}

// result arrays for n pairs (the blob starts empty and grows with every fetched plan)
int vsxh::results_alloc(vsx_results * out, uint64_t n, bool with_verdict)
{
  std::memset(out, 0, sizeof *out);
  const uint64_t n1 = std::max<uint64_t>(n, 1);
  out->n_pairs = n;
  out->score = (int16_t *) std::malloc(n1 * 2);
  out->aligned = (uint16_t *) std::malloc(n1 * 2);
  out->matches = (uint16_t *) std::malloc(n1 * 2);
  out->mismatches = (uint16_t *) std::malloc(n1 * 2);
  out->gaps = (uint16_t *) std::malloc(n1 * 2);
  out->cigar_off = (uint64_t *) std::malloc(n1 * 8);
  out->verdict = with_verdict ? (uint8_t *) std::malloc(n1) : nullptr;
  out->cigar_blob = (char *) std::malloc(1);
  if (!out->score || !out->aligned || !out->matches || !out->mismatches || !out->gaps || !out->cigar_off || !out->cigar_blob ||
      (with_verdict && !out->verdict))
    { vsx_results_free(out); return fail(VSX_ENOMEM, "vsx_plan_fetch: host allocation failed"); }
  return VSX_OK;
}

FetchDest vsxh::dest_at(vsx_results * out, uint64_t first)
{
  return FetchDest {out->score + first, out->aligned + first, out->matches + first, out->mismatches + first, out->gaps + first,
                    out->cigar_off + first, out->verdict ? out->verdict + first : nullptr, &out->cigar_blob, &out->cigar_bytes};
}

extern "C" {

int vsx_plan_fetch(vsx_plan * pl, vsx_results * out)
{
  if (!pl || !out) return fail(VSX_EINVAL, "vsx_plan_fetch: null argument");
  int rc = results_alloc(out, pl->n_pairs, pl->filter.enabled != 0);
  if (rc != VSX_OK) return rc;
  rc = fetch_core(pl, dest_at(out, 0));
  if (rc != VSX_OK) vsx_results_free(out);      // (it leaves the error text alone)
  return rc;
}

int vsx_plan_export_hits(vsx_plan * pl, void * d_dst, uint64_t dst_bytes)
{
  static_assert(sizeof(VsxPairOut) == VSX_HIT_RECORD_BYTES, "hit record layout");
  if (!pl || !d_dst) return fail(VSX_EINVAL, "vsx_plan_export_hits: null argument");
  if (!pl->ran) return fail(VSX_EINVAL, "vsx_plan_export_hits: plan has not been run");
  if (dst_bytes < pl->n_pairs * sizeof(VsxPairOut)) return fail(VSX_EINVAL, "vsx_plan_export_hits: destination too small");
  // the records are written on the traceback stream; a plan whose run buffer overflowed runs again first (their run offsets
  // would point past the buffer)
  unsigned long long used = 0, text_used = 0;
  const int src = settle_runs(pl, used, text_used);
  if (src != VSX_OK) return src;
  hipStream_t st = pl->ctx->stream;
  if (!pl->host_patched)
    {
      // pairs answered without DP live on the host: patch them into the device array once; their CIGARs (the Q == 0 closed
      // form, one 'I' run) follow the device runs in the exported run buffer (vsx_plan_export_runs)
      for (size_t h = 0, hc = 0; h < pl->host_pairs.size(); ++h)
        {
          VsxPairOut o = pl->host_out[h];
          if (hc < pl->host_cigar_pair.size() && pl->host_cigar_pair[hc] == pl->host_pairs[h]) { o.nruns = 1; o.run_off = used + hc; ++hc; }
          VSX_HIP(hipMemcpy(pl->d_out.p + pl->host_pairs[h], &o, sizeof(VsxPairOut), hipMemcpyHostToDevice));
        }
      pl->host_patched = true;
    }
  VSX_HIP(hipMemcpyAsync(d_dst, pl->d_out.p, pl->n_pairs * sizeof(VsxPairOut), hipMemcpyDeviceToDevice, st));
  VSX_HIP(hipStreamSynchronize(st));
  return VSX_OK;
}

int vsx_plan_export_runs(vsx_plan * pl, void * d_dst, uint64_t dst_bytes, uint64_t * n_runs)
{
  if (!pl || !n_runs) return fail(VSX_EINVAL, "vsx_plan_export_runs: null argument");
  if (!pl->ran) return fail(VSX_EINVAL, "vsx_plan_export_runs: plan has not been run");
  unsigned long long used = 0, text_used = 0;
  const int src = settle_runs(pl, used, text_used);          // (an overflowed run buffer: resized, the plan runs again)
  if (src != VSX_OK) return src;
  const uint64_t extra = pl->host_cigar_run.size();          // run words of the pairs answered on the host, behind the device's
  *n_runs = used + extra;
  if (!d_dst) return VSX_OK;                     // size query
  if (dst_bytes < (used + extra) * 4) return fail(VSX_EINVAL, "vsx_plan_export_runs: destination too small");
  if (used) VSX_HIP(hipMemcpyAsync(d_dst, pl->d_runs.p, used * 4, hipMemcpyDeviceToDevice, pl->ctx->stream));
  if (extra) VSX_HIP(hipMemcpyAsync(static_cast<uint32_t *>(d_dst) + used, pl->host_cigar_run.data(), extra * 4, hipMemcpyHostToDevice, pl->ctx->stream));
  VSX_HIP(hipStreamSynchronize(pl->ctx->stream));
  return VSX_OK;
}

// test hook (tests/test_gpu_marshal.py): both exports in the order a rank of the gather makes them -- records, size query, run
// words -- into device scratch of the plan's context, then copied to the host.  rec_out: n_pairs records; runs_out: room for
// runs_cap words (nullptr: only *n_runs is reported).
int vsx_internal_export_host(vsx_plan * pl, void * rec_out, uint32_t * runs_out, uint64_t runs_cap, uint64_t * n_runs)
{
  if (!pl || !rec_out || !n_runs) return fail(VSX_EINVAL, "vsx_internal_export_host: null argument");
  VSX_HIP(hipSetDevice(pl->ctx->device));
  PoolBuf<uint8_t> d_rec;
  PoolBuf<uint32_t> d_runs;
  const uint64_t rec_bytes = pl->n_pairs * sizeof(VsxPairOut);
  VSX_HIP(d_rec.alloc(&pl->ctx->pool, rec_bytes));
  int rc = pl->n_pairs ? vsx_plan_export_hits(pl, d_rec.p, rec_bytes) : VSX_OK;
  if (rc == VSX_OK) rc = vsx_plan_export_runs(pl, nullptr, 0, n_runs);
  if (rc != VSX_OK) return rc;
  if (rec_bytes) VSX_HIP(hipMemcpy(rec_out, d_rec.p, rec_bytes, hipMemcpyDeviceToHost));
  if (!runs_out || *n_runs == 0) return VSX_OK;
  if (runs_cap < *n_runs) return fail(VSX_EINVAL, "vsx_internal_export_host: destination too small");
  VSX_HIP(d_runs.alloc(&pl->ctx->pool, *n_runs));
  if ((rc = vsx_plan_export_runs(pl, d_runs.p, *n_runs * 4, n_runs)) != VSX_OK) return rc;
  VSX_HIP(hipMemcpy(runs_out, d_runs.p, *n_runs * 4, hipMemcpyDeviceToHost));
  return VSX_OK;
}

int64_t vsx_cigar_from_runs(const uint32_t * runs, uint32_t n, char * dst, uint64_t cap)
{
  if (n && !runs) { (void) fail(VSX_EINVAL, "vsx_cigar_from_runs: null argument"); return VSX_EINVAL; }
  std::string s;
  append_cigar(s, runs, n);
  if (dst && cap > s.size()) std::memcpy(dst, s.c_str(), s.size() + 1);
  return (int64_t) s.size() + 1;
}

void vsx_ranked_free(vsx_ranked * r)
{
  if (!r) return;
  std::free(r->pair); std::free(r->score); std::free(r->aligned); std::free(r->matches); std::free(r->mismatches); std::free(r->gaps);
  std::free(r->verdict); std::free(r->id); std::free(r->cigar_off); std::free(r->cigar_blob); std::free(r->undecided);
  std::memset(r, 0, sizeof *r);
}

void vsx_results_free(vsx_results * r)
{
  if (!r) return;
  std::free(r->score); std::free(r->aligned); std::free(r->matches); std::free(r->mismatches);
  std::free(r->gaps); std::free(r->cigar_off); std::free(r->cigar_blob); std::free(r->verdict);
  std::memset(r, 0, sizeof *r);
}

}  // extern "C"
