// vsx_sortby.cpp -- host side of vsx_sortby (include/vsx_sortby.h): the checks, the routes, the rounds around the kernels of
// vsx_sortby.hip and the host restatement.
//
//   device    headers, lengths and abundances go up once.  The numeric round and up to max_rounds label rounds run the step of
//             vsx_sortby_internal.h; after each the host waits for one number, the records still open.  Groups still open at the
//             cap come down as (group start, item) lists and are finished by the host comparator on the headers (host_long_prefix).
//             Median and topn are taken on the host from the downloaded order.
//   host      the reference's comparator, literally, under std::stable_sort over the deck in input order; above 65 536 records
//             stable runs on the library's threads and a stable merge tree.  Routes: no context, VSX_SORTBY=host, more records
//             than the 32-bit device arrays hold, arrays that do not fit the device; each with its counter.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/vsx_sortby.h"
#include "vsx_private.h"
#include "vsx_sortby_internal.h"

using vsxp::env_u64;
using vsxp::fail;
using vsxp::host_array;
using vsxp::now_s;
using vsxp::Scratch;

namespace {

constexpr const char * WHO = "vsx_sortby";
constexpr uint64_t COUNT_LIMIT = (uint64_t) UINT32_MAX - 1;
constexpr int HOST_THREADS = 16;
constexpr uint64_t HOST_RUN_MIN = 65536;                         // records per stable run of the host restatement

thread_local vsx_sortby_stats g_stats {};

struct Plan {
  uint64_t n = 0;
  int order = 0;
  const unsigned char * blob = nullptr;
  uint64_t blob_bytes = 0;
  const uint64_t * off = nullptr;
  const uint32_t * len = nullptr;
  const uint32_t * seqlen = nullptr;
  const uint32_t * size = nullptr;
  int64_t minsize = 0, maxsize = INT64_MAX;
  uint64_t topn = 0;
  uint32_t max_rounds = VSX_SORTBY_MAX_ROUNDS;
  int nth = 1;
  bool kept(uint64_t i) const { return order != VSX_SORTBY_SIZE || ((int64_t) size[i] >= minsize && (int64_t) size[i] <= maxsize); }
  // what the median is taken over
  uint32_t key(uint64_t i) const { return order == VSX_SORTBY_SIZE ? size[i] : seqlen[i]; }
  // strcmp of two headers without a NUL: unsigned bytes, a proper prefix first
  int label_cmp(uint64_t a, uint64_t b) const
  {
    const uint32_t la = len[a], lb = len[b];
    const int c = std::memcmp(blob + off[a], blob + off[b], std::min(la, lb));
    return c ? c : (la < lb ? -1 : la > lb ? 1 : 0);
  }
  // the reference's comparators (commands/sortbysize.cpp:110-123, commands/sortbylength.cpp:108-128, core/db.cpp:452-469)
  bool less(uint64_t a, uint64_t b) const
  {
    if (order != VSX_SORTBY_SIZE && seqlen[a] != seqlen[b]) return order == VSX_SORTBY_LENGTH ? seqlen[a] > seqlen[b] : seqlen[a] < seqlen[b];
    if (size[a] != size[b]) return size[a] > size[b];
    return label_cmp(a, b) < 0;
  }
};

void release(vsx_sortby_out * out)
{
  std::free(out->order);
  std::memset(out, 0, sizeof *out);
}

// stable sort of v by less(): stable runs on the threads, then a stable merge tree
template <typename T, typename Less>
void stable_sort_parallel(std::vector<T> & v, int nth, Less less)
{
  const uint64_t m = v.size();
  const int runs = (int) std::max<uint64_t>(1, std::min<uint64_t>((uint64_t) nth, m / HOST_RUN_MIN));
  if (runs <= 1) { std::stable_sort(v.begin(), v.end(), less); return; }
  std::vector<uint64_t> cut((size_t) runs + 1);
  for (int t = 0; t <= runs; ++t) cut[(size_t) t] = m * (uint64_t) t / (uint64_t) runs;
  vsxp::run_pool(runs, [&](int t) { std::stable_sort(v.begin() + (ptrdiff_t) cut[(size_t) t], v.begin() + (ptrdiff_t) cut[(size_t) t + 1], less); });
  std::vector<T> other(m);
  std::vector<T> * from = &v, * to = &other;
  for (int width = 1; width < runs; width *= 2)
    {
      const int pairs = (runs + 2 * width - 1) / (2 * width);
      vsxp::run_pool(pairs, [&](int p) {
        const int lo = p * 2 * width, mid = std::min(runs, lo + width), hi = std::min(runs, lo + 2 * width);
        std::merge(from->begin() + (ptrdiff_t) cut[(size_t) lo], from->begin() + (ptrdiff_t) cut[(size_t) mid], from->begin() + (ptrdiff_t) cut[(size_t) mid],
                   from->begin() + (ptrdiff_t) cut[(size_t) hi], to->begin() + (ptrdiff_t) cut[(size_t) lo], less);       // equal: the left run first
      });
      std::swap(from, to);
    }
  if (from != &v) v.swap(other);
}

// n_kept, median, topn and the widened order from the sorted deck
template <typename T>
int finish(const Plan & P, const std::vector<T> & deck, vsx_sortby_out & out)
{
  const uint64_t kept = deck.size();
  out.n_kept = kept;
  out.median = 0.0;
  if (kept)
    {
      // find_median_abundance / find_median_length: the middle key, or the lower of the two middle keys plus half their distance
      const uint64_t mid = kept / 2;
      if (kept % 2) out.median = P.key(deck[mid]) * 1.0;
      else
        {
          const uint32_t a = P.key(deck[mid - 1]), b = P.key(deck[mid]), lo = std::min(a, b), hi = std::max(a, b);
          out.median = lo + ((hi - lo) * 0.5);
        }
    }
  out.n_out = std::min<uint64_t>(kept, P.topn);
  out.order = host_array<uint64_t>(out.n_out);
  if (!out.order) return fail(VSX_ENOMEM, "%s: out of memory", WHO);
  for (uint64_t x = 0; x < out.n_out; ++x) out.order[x] = deck[x];
  g_stats.kept = kept;
  return VSX_OK;
}

// ---- the host restatement ---------------------------------------------------------------------------------------------------------
int host_route(const Plan & P, vsx_sortby_out & out)
{
  const vsxp::Stopwatch watch(g_stats.seconds_output);
  std::vector<uint64_t> deck;
  deck.reserve(P.n);
  for (uint64_t i = 0; i < P.n; ++i) if (P.kept(i)) deck.push_back(i);
  stable_sort_parallel(deck, P.nth, [&P](uint64_t a, uint64_t b) { return P.less(a, b); });
  return finish(P, deck, out);
}

// ---- the device route -----------------------------------------------------------------------------------------------------------
struct DeviceBufs {
  Scratch<uint8_t> blob;
  Scratch<uint64_t> off;
  Scratch<uint32_t> len, seqlen, size, flag, slot, item, g, idx0, idx1, g1, g2, idx2, item2, first, first_at, mark, ng, order;
  Scratch<unsigned long long> key, key_sorted, key2;
  std::vector<std::unique_ptr<Scratch<uint8_t>>> temps;       // rocPRIM's temporary storage, kept until the round's kernels are through
};

// a rocPRIM call: the first call sizes the temporary storage, the second runs
template <typename F>
int with_temp(vsx_ctx * ctx, DeviceBufs & B, F && call)
{
  size_t bytes = 0;
  VSX_HIP_AS(WHO, call(nullptr, &bytes));
  B.temps.emplace_back(new Scratch<uint8_t>());
  VSX_HIP_AS(WHO, B.temps.back()->alloc(ctx, bytes));
  VSX_HIP_AS(WHO, call(B.temps.back()->p, &bytes));
  return VSX_OK;
}

uint64_t device_bytes(const Plan & P, uint64_t label_bytes) { return label_bytes + 160 * (P.n + 1) + ((uint64_t) 64 << 20); }

// One step over the m active records (item, g, key): the new order of the group members in d_order, the records still open in
// (item, g), their number in *m_next.  Waits for the stream.
int step(vsx_ctx * ctx, hipStream_t st, DeviceBufs & B, uint32_t m, bool label_round, uint32_t key_bits, uint32_t g_bits, uint32_t * m_next)
{
  int rc;
  VSX_HIP_AS(WHO, vsx_launch_sortby_iota(m, B.idx0.p, st));
  if ((rc = with_temp(ctx, B, [&](void * t, size_t * b) { return vsx_launch_sortby_sort64(t, b, B.key.p, B.key_sorted.p, B.idx0.p, B.idx1.p, m, key_bits, st); })) != VSX_OK) return rc;
  const uint32_t * g2 = B.g.p, * idx2 = B.idx1.p;                  // the numeric round: one group, g = 0 throughout
  if (label_round)
    {
      VSX_HIP_AS(WHO, vsx_launch_sortby_gather32(m, B.g.p, B.idx1.p, B.g1.p, st));
      if ((rc = with_temp(ctx, B, [&](void * t, size_t * b) { return vsx_launch_sortby_sort32(t, b, B.g1.p, B.g2.p, B.idx1.p, B.idx2.p, m, g_bits, st); })) != VSX_OK) return rc;
      g2 = B.g2.p; idx2 = B.idx2.p;
    }
  VSX_HIP_AS(WHO, vsx_launch_sortby_gather(m, idx2, B.key.p, B.item.p, g2, B.key2.p, B.item2.p, B.first.p, st));
  if ((rc = with_temp(ctx, B, [&](void * t, size_t * b) { return vsx_launch_sortby_scan_max(t, b, B.first.p, B.first_at.p, m, st); })) != VSX_OK) return rc;
  VSX_HIP_AS(WHO, vsx_launch_sortby_place(m, g2, B.first_at.p, B.key2.p, B.item2.p, B.order.p, B.mark.p, st));
  if ((rc = with_temp(ctx, B, [&](void * t, size_t * b) { return vsx_launch_sortby_scan_max(t, b, B.mark.p, B.ng.p, m, st); })) != VSX_OK) return rc;
  VSX_HIP_AS(WHO, vsx_launch_sortby_open(m, label_round ? 1 : 0, B.ng.p, B.key2.p, B.flag.p, st));
  VSX_HIP_AS(WHO, hipMemsetAsync(B.flag.p + m, 0, sizeof(uint32_t), st));
  if ((rc = with_temp(ctx, B, [&](void * t, size_t * b) { return vsx_launch_sortby_scan_sum(t, b, B.flag.p, B.slot.p, (uint64_t) m + 1, st); })) != VSX_OK) return rc;
  uint32_t open = 0;
  VSX_HIP_AS(WHO, hipMemcpyAsync(&open, B.slot.p + m, sizeof open, hipMemcpyDeviceToHost, st));
  VSX_HIP_AS(WHO, vsx_launch_sortby_compact(m, B.flag.p, B.slot.p, B.item2.p, B.ng.p, B.item.p, B.g.p, st));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  B.temps.clear();
  if (open > m) return fail(VSX_EHIP, "%s: the scan counts %u open records of %u", WHO, open, m);
  *m_next = open;
  return VSX_OK;
}

// groups still open at the round cap: every run of equal group start in (g, item) through the host comparator, into its places
void finish_groups(const Plan & P, const std::vector<uint32_t> & g, std::vector<uint32_t> & item, std::vector<uint32_t> & order)
{
  std::vector<size_t> start;
  for (size_t a = 0; a < g.size(); ++a) if (a == 0 || g[a] != g[a - 1]) start.push_back(a);
  start.push_back(g.size());
  const size_t groups = start.size() - 1;
  const int nth = (int) std::max<size_t>(1, std::min<size_t>((size_t) P.nth, groups));
  vsxp::run_pool(nth, [&](int t) {
    for (size_t k = (size_t) t; k < groups; k += (size_t) nth)
      {
        std::stable_sort(item.begin() + (ptrdiff_t) start[k], item.begin() + (ptrdiff_t) start[k + 1],
                         [&P](uint32_t a, uint32_t b) { return P.label_cmp(a, b) < 0; });
        for (size_t a = start[k]; a < start[k + 1]; ++a) order[(size_t) g[start[k]] + (a - start[k])] = item[a];
      }
  });
}

int device_run(vsx_ctx * ctx, hipStream_t st, const Plan & P, uint64_t label_bytes, uint64_t blob_first, DeviceBufs & B, vsx_sortby_out & out)
{
  const uint32_t n = (uint32_t) P.n;
  int rc;

  // ---- headers and keys
  double t0 = now_s();
  std::vector<uint64_t> off((size_t) n);
  for (uint32_t i = 0; i < n; ++i) off[i] = P.len[i] ? P.off[i] - blob_first : 0;          // (an empty header may point anywhere)
  VSX_HIP_AS(WHO, B.blob.upload(ctx, P.blob + blob_first, label_bytes, st));
  VSX_HIP_AS(WHO, B.off.upload(ctx, off.data(), n, st));
  VSX_HIP_AS(WHO, B.len.upload(ctx, P.len, n, st));
  VSX_HIP_AS(WHO, B.seqlen.upload(ctx, P.seqlen, n, st));
  VSX_HIP_AS(WHO, B.size.upload(ctx, P.size, n, st));
  for (Scratch<uint32_t> * a : { &B.flag, &B.slot, &B.item, &B.g, &B.idx0, &B.idx1, &B.g1, &B.g2, &B.idx2, &B.item2, &B.first, &B.first_at, &B.mark, &B.ng, &B.order })
    VSX_HIP_AS(WHO, a->alloc(ctx, (size_t) n + 1));
  for (Scratch<unsigned long long> * a : { &B.key, &B.key_sorted, &B.key2 }) VSX_HIP_AS(WHO, a->alloc(ctx, (size_t) n + 1));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  g_stats.seconds_h2d += now_s() - t0;

  // ---- selection, numeric keys, tie groups
  t0 = now_s();
  VSX_HIP_AS(WHO, vsx_launch_sortby_select(n, P.order, P.minsize, P.maxsize, B.size.p, B.flag.p, st));
  VSX_HIP_AS(WHO, hipMemsetAsync(B.flag.p + n, 0, sizeof(uint32_t), st));
  if ((rc = with_temp(ctx, B, [&](void * t, size_t * b) { return vsx_launch_sortby_scan_sum(t, b, B.flag.p, B.slot.p, (uint64_t) n + 1, st); })) != VSX_OK) return rc;
  uint32_t kept = 0;
  VSX_HIP_AS(WHO, hipMemcpyAsync(&kept, B.slot.p + n, sizeof kept, hipMemcpyDeviceToHost, st));
  VSX_HIP_AS(WHO, vsx_launch_sortby_keys(n, P.order, B.seqlen.p, B.size.p, B.flag.p, B.slot.p, B.item.p, B.key.p, B.g.p, st));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  B.temps.clear();
  if (kept > n) return fail(VSX_EHIP, "%s: the scan keeps %u records of %u", WHO, kept, n);
  uint32_t g_bits = 1;
  while (g_bits < 32 && ((uint64_t) 1 << g_bits) < kept) ++g_bits;
  uint32_t m = 0;
  if (kept && (rc = step(ctx, st, B, kept, false, P.order == VSX_SORTBY_SIZE ? 32u : 64u, g_bits, &m)) != VSX_OK) return rc;
  g_stats.active_numeric = m;
  g_stats.seconds_numeric += now_s() - t0;

  // ---- label rounds
  t0 = now_s();
  uint32_t round = 0;
  for (; m > 0 && round < P.max_rounds; ++round)
    {
      VSX_HIP_AS(WHO, vsx_launch_sortby_chunk(m, round, B.blob.p, B.off.p, B.len.p, B.item.p, B.key.p, st));
      if ((rc = step(ctx, st, B, m, true, 64u, g_bits, &m)) != VSX_OK) return rc;
      if (round < VSX_SORTBY_STAT_ROUNDS) g_stats.active[round] = m;
    }
  g_stats.rounds = round;
  g_stats.seconds_refine += now_s() - t0;

  // ---- the order, and what the cap left
  t0 = now_s();
  std::vector<uint32_t> order, g, item;
  VSX_HIP_AS(WHO, vsxp::download(order, B.order.p, kept, st));
  if (m) { VSX_HIP_AS(WHO, vsxp::download(g, B.g.p, m, st)); VSX_HIP_AS(WHO, vsxp::download(item, B.item.p, m, st)); }
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  g_stats.seconds_output += now_s() - t0;
  if (m)
    {
      t0 = now_s();
      for (uint32_t a = 0; a < m; ++a)
        if (item[a] >= n || g[a] >= kept || (a && g[a] < g[a - 1])) return fail(VSX_EHIP, "%s: an open group list is out of range", WHO);
      finish_groups(P, g, item, order);
      g_stats.host_long_prefix = 1;
      g_stats.capped_items = m;
      g_stats.seconds_host_finish += now_s() - t0;
    }
  t0 = now_s();
  for (uint32_t x = 0; x < kept; ++x) if (order[x] >= n) return fail(VSX_EHIP, "%s: the order names record %u of %u", WHO, order[x], n);
  rc = finish(P, order, out);
  g_stats.seconds_output += now_s() - t0;
  return rc;
}

int device_route(vsx_ctx * ctx, const Plan & P, uint64_t label_bytes, uint64_t blob_first, vsx_sortby_out & out)
{
  hipStream_t st = vsx_internal_stream(ctx);
  DeviceBufs B;
  const int rc = device_run(ctx, st, P, label_bytes, blob_first, B, out);
  (void) hipStreamSynchronize(st);                             // nothing of this call runs on once its blocks go back to the pool
  return rc;
}

int run(vsx_ctx * ctx, const vsx_sortby_opts * o, uint64_t n, const char * blob, uint64_t blob_bytes, const uint64_t * offsets,
        const uint32_t * lengths, const uint32_t * seq_lengths, const uint32_t * sizes, vsx_sortby_out * out)
{
  g_stats = vsx_sortby_stats {};
  const double t_begin = now_s();
  if (!o || !out) return fail(VSX_EINVAL, "%s: null argument", WHO);
  std::memset(out, 0, sizeof *out);
  if (n && (!offsets || !lengths || !seq_lengths || !sizes || (!blob && blob_bytes))) return fail(VSX_EINVAL, "%s: null argument", WHO);
  if (o->order != VSX_SORTBY_SIZE && o->order != VSX_SORTBY_LENGTH && o->order != VSX_SORTBY_LENGTH_ASC) return fail(VSX_EINVAL, "%s: unknown order %d", WHO, o->order);
  if (o->topn < 0 || o->threads < 0) return fail(VSX_EINVAL, "%s: topn and threads cannot be negative", WHO);
  const uint64_t max_rounds = env_u64("VSX_SORTBY_MAX_ROUNDS", VSX_SORTBY_MAX_ROUNDS);
  if (max_rounds > VSX_SORTBY_MAX_ROUNDS) return fail(VSX_EINVAL, "%s: VSX_SORTBY_MAX_ROUNDS must be 0 .. %d", WHO, VSX_SORTBY_MAX_ROUNDS);
  Plan P;
  P.n = n; P.order = o->order; P.blob = reinterpret_cast<const unsigned char *>(blob); P.blob_bytes = blob_bytes;
  P.off = offsets; P.len = lengths; P.seqlen = seq_lengths; P.size = sizes;
  P.minsize = o->minsize; P.maxsize = o->maxsize; P.topn = (uint64_t) o->topn; P.max_rounds = (uint32_t) max_rounds;
  P.nth = std::max(1, std::min(o->threads > 0 ? o->threads : vsxp::usable_cpus(), HOST_THREADS));
  // the span of the blob the headers use: only that goes up
  if (const int rc = vsxp::check_spans(WHO, "a header", n, offsets, lengths, blob_bytes)) return rc;
  uint64_t first = blob_bytes, last = 0, label_bytes = 0;
  for (uint64_t i = 0; i < n; ++i)
    {
      if (sizes[i] == 0) return fail(VSX_EINVAL, "%s: record %llu has abundance 0", WHO, (unsigned long long) i);
      if (!lengths[i]) continue;
      if (std::memchr(blob + offsets[i], 0, lengths[i])) return fail(VSX_EINVAL, "%s: the header of record %llu holds a NUL byte", WHO, (unsigned long long) i);
      first = std::min(first, offsets[i]); last = std::max(last, offsets[i] + lengths[i]);
      label_bytes += lengths[i];
    }
  const uint64_t span = last > first ? last - first : 0;
  if (span == 0) first = 0;
  out->n = n;
  g_stats.items = n; g_stats.label_bytes = label_bytes; g_stats.max_rounds = max_rounds;
  g_stats.seconds_stage += now_s() - t_begin;

  // ---- the route
  bool host = true;
  const uint64_t count_limit = std::min<uint64_t>(COUNT_LIMIT, env_u64("VSX_SORTBY_DEVICE_COUNT", COUNT_LIMIT));
  if (!ctx) g_stats.host_no_context = 1;
  else if (vsxp::env_is_host("VSX_SORTBY")) g_stats.host_environment = 1;
  else if (n > count_limit) g_stats.host_count = 1;
  else host = false;
  int rc = VSX_OK;
  if (!host && n)
    {
      const uint64_t need = env_u64("VSX_SORTBY_PRETEND_BYTES", device_bytes(P, span));
      bool fit = false;
      if ((rc = vsxp::device_fits(ctx, WHO, need, nullptr, &fit)) != VSX_OK) { release(out); return rc; }
      if (!fit) { host = true; g_stats.host_memory = 1; }
    }
  if (!host && n) rc = device_route(ctx, P, span, first, *out);
  else rc = host_route(P, *out);
  if (rc != VSX_OK) { release(out); return rc; }
  out->n = n;
  g_stats.seconds_total = now_s() - t_begin;
  return VSX_OK;
}

}  // namespace

extern "C" {

void vsx_sortby_opts_default(vsx_sortby_opts * o)
{
  std::memset(o, 0, sizeof *o);
  o->order = VSX_SORTBY_SIZE;
  o->maxsize = INT64_MAX;
  o->topn = INT64_MAX;
}

void vsx_sortby_last_stats(vsx_sortby_stats * out) { if (out) *out = g_stats; }

void vsx_sortby_out_free(vsx_sortby_out * out) { if (out) release(out); }

int vsx_sortby(vsx_ctx * ctx, const vsx_sortby_opts * opts, uint64_t n, const char * label_blob, uint64_t blob_bytes,
               const uint64_t * label_offsets, const uint32_t * label_lengths, const uint32_t * seq_lengths, const uint32_t * sizes,
               vsx_sortby_out * out)
{
  return run(ctx, opts, n, label_blob, blob_bytes, label_offsets, label_lengths, seq_lengths, sizes, out);
}

}  // extern "C"
