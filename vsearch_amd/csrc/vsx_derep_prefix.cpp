// vsx_derep_prefix.cpp -- prefix dereplication (include/vsx_derep_prefix.h: vsx_derep_prefix), the host side of vsx_derep_prefix.hip.
//
// Restated from the reference (src/, v2.31.0): commands/derep_prefix.cpp: derep_prefix() -- the walk over the length-sorted
// database with its exact / prefix / no match cases, derep_compare_prefix's order, the median, the selection -- and
// core/db.cpp: Database::sortbylength_shortest_first.  The walk is not restated as a walk: both routes apply the one-pass rule
// (a node is absorbed by the lowest-ranked node that properly extends it; DESIGN, "Prefix dereplication").
//
// Both routes name a read by its rank (its position in the sorted order) and end in the same intermediate form (Groups): the
// clusters ascending by their lowest rank, every cluster's members in rank order, a flag per rank that tells the heads of the
// nodes from their duplicates, a top and a size per cluster.  finish() turns it into the caller's output.
//
//   device   the kept reads are staged in rank order, window by window (the slots and items of the exact search's plan), turned
//            into code words by vsx_launch_exact_hash, scanned, grouped, claimed, resolved, accounted and sorted by the kernels
//            of vsx_derep_prefix.hip and vsx_derep.hip.
//   host     host_links below: FNV-1a over the codes gives every prefix's hash in one pass per node, an open-addressing table of
//            the nodes answers the probes, the claims of the nodes run on the library's worker pool with a compare-and-swap
//            minimum.  Written from the rule and not from the kernels.  VSX_DEREP_PREFIX=host, a missing context, more than
//            UINT32_MAX - 1 kept reads or buffers that do not fit the device send the whole call through it.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "../../include/vsx_derep_prefix.h"
#include "vsx_derep_prefix_internal.h"
#include "vsx_private.h"

using vsxp::array_of;
using vsxp::fail;
using vsxp::now_s;
using vsxp::upload;
using vsxp::DevBuf;
using vsxp::PinnedBuf;
using vsxp::ensure_pinned;
using vsxp::map4;

namespace {

constexpr const char * WHO = "vsx_derep_prefix";
constexpr uint64_t WINDOW_READS = 65536;
constexpr uint64_t SIZE_LIMIT = 1ull << 32;                 // the reference's 32-bit cluster size: not restated, refused
constexpr uint64_t NONE = UINT64_MAX;
constexpr int HOST_THREADS = 16;                               // what the sort and the host restatement take of the worker pool at most

thread_local vsx_derep_prefix_stats g_stats {};

// ---- the input as both routes read it: by rank -------------------------------------------------------------------------------
struct Input {
  const vsx_derep_prefix_opts * o;
  const vsx_fastx_reads * reads;
  const char * label_blob;
  const uint64_t * label_off;
  std::vector<uint64_t> order;       // order[r]: input index of the kept read of rank r
  std::vector<uint32_t> lengths;     // the distinct lengths, ascending
  const char * seq(uint64_t r) const { return reads->seq + reads->off[order[r]]; }
  uint32_t len(uint64_t r) const { return reads->len[order[r]]; }
  uint64_t size(uint64_t r) const { return (o->sizein && reads->abundance) ? reads->abundance[order[r]] : 1; }
  const char * label(uint64_t r) const { return label_blob + label_off[order[r]]; }
  uint64_t label_len(uint64_t r) const { return label_off[order[r] + 1] - label_off[order[r]]; }
};

// strcmp of two labels that carry no terminator
inline int label_cmp(const char * a, uint64_t la, const char * b, uint64_t lb)
{
  const int cmp = std::memcmp(a, b, std::min(la, lb));
  if (cmp != 0) return cmp;
  return la < lb ? -1 : (la > lb ? 1 : 0);
}

// Database::sortbylength_shortest_first: length ascending, abundance descending, label, input order.  The abundance is the
// header's annotation whether or not it is summed.  Length and abundance are one integer key and the label's first eight bytes
// another (big-endian, zero-padded: it orders as strcmp does until it ties); the slices of the worker pool are sorted side by
// side and merged pairwise.
void rank_reads(Input & in, const std::vector<uint64_t> & kept)
{
  struct Key { uint64_t key, prefix, index; };
  const vsx_fastx_reads & R = *in.reads;
  const uint64_t K = kept.size();
  std::vector<Key> keys(K);
  const int nth = K < 32768 ? 1 : std::max(1, std::min(vsxp::usable_cpus(), HOST_THREADS));
  std::vector<uint64_t> bound((size_t) nth + 1);
  for (int t = 0; t <= nth; ++t) bound[(size_t) t] = K * (uint64_t) t / (uint64_t) nth;
  auto less = [&](const Key & a, const Key & b) {
    if (a.key != b.key) return a.key < b.key;
    if (a.prefix != b.prefix) return a.prefix < b.prefix;
    const int cmp = label_cmp(in.label_blob + in.label_off[a.index], in.label_off[a.index + 1] - in.label_off[a.index],
                              in.label_blob + in.label_off[b.index], in.label_off[b.index + 1] - in.label_off[b.index]);
    if (cmp != 0) return cmp < 0;
    return a.index < b.index;
  };
  vsxp::run_pool(nth, [&](int t) {
    for (uint64_t k = bound[(size_t) t]; k < bound[(size_t) t + 1]; ++k)
      {
        const uint64_t i = kept[k], ab = R.abundance ? R.abundance[i] : 1;            // below 2^32: checked by the caller
        const unsigned char * l = reinterpret_cast<const unsigned char *>(in.label_blob) + in.label_off[i];
        const uint64_t ll = in.label_off[i + 1] - in.label_off[i];
        uint64_t prefix = 0;
        for (uint64_t b = 0; b < 8; ++b) prefix = (prefix << 8) | (b < ll ? l[b] : 0u);
        keys[k] = Key { ((uint64_t) R.len[i] << 32) | (0xFFFFFFFFull - ab), prefix, i };
      }
    std::sort(keys.begin() + (std::ptrdiff_t) bound[(size_t) t], keys.begin() + (std::ptrdiff_t) bound[(size_t) t + 1], less);
  });
  for (int width = 1; width < nth; width *= 2)
    vsxp::run_pool(nth, [&](int t) {
      if (t % (2 * width) != 0 || t + width >= nth) return;
      const auto at = [&](int u) { return keys.begin() + (std::ptrdiff_t) bound[(size_t) std::min(u, nth)]; };
      std::inplace_merge(at(t), at(t + width), at(t + 2 * width), less);
    });
  in.order.resize(K);
  for (uint64_t r = 0; r < K; ++r)
    {
      in.order[r] = keys[r].index;
      const uint32_t L = R.len[keys[r].index];
      if (in.lengths.empty() || in.lengths.back() != L) in.lengths.push_back(L);
    }
}

// clusters ascending by lowest rank; members are ranks
struct Groups {
  std::vector<uint64_t> cstart;      // clusters + 1
  std::vector<uint64_t> member;      // kept: a cluster's members in rank order
  std::vector<uint64_t> top;         // clusters: the head of the chain's longest node (the representative)
  std::vector<uint64_t> size;        // clusters
  std::vector<uint8_t> head;         // kept, by rank: 1 when the read is its node's head
};

// ---- the host restatement ------------------------------------------------------------------------------------------------------
constexpr uint64_t FNV_BASIS = 14695981039346656037ull, FNV_PRIME = 1099511628211ull;

inline void atomic_min(uint64_t * p, uint64_t v)
{
  uint64_t cur = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (v < cur && !__atomic_compare_exchange_n(p, &cur, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
}

// node[r]: the head of r's node; top[r]: the head of the longest node of r's chain
void host_links(const Input & in, std::vector<uint64_t> & node, std::vector<uint64_t> & top)
{
  const uint64_t K = in.order.size();
  const int nth = std::max(1, std::min(vsxp::usable_cpus(), HOST_THREADS));
  // the codes and every read's hash at its own length
  std::vector<uint64_t> coff(K + 1, 0), hash(K);
  for (uint64_t r = 0; r < K; ++r) coff[r + 1] = coff[r] + in.len(r);
  std::vector<uint8_t> codes(coff[K] + 1);
  vsxp::run_pool(nth, [&](int t) {
    for (uint64_t r = (uint64_t) t; r < K; r += (uint64_t) nth)
      {
        const char * s = in.seq(r);
        uint8_t * c = codes.data() + coff[r];
        uint64_t h = FNV_BASIS;
        for (uint32_t i = 0, L = in.len(r); i < L; ++i) { c[i] = map4((unsigned char) s[i]); h = (h ^ c[i]) * FNV_PRIME; }
        hash[r] = h;
      }
  });
  // the nodes: find-or-insert in rank order, so a node's owner is its head
  const uint64_t table_size = vsxe::table_size_for(K), mask = table_size - 1;
  std::vector<uint64_t> table(table_size, NONE);
  node.assign(K, 0);
  uint64_t nodes = 0;
  for (uint64_t r = 0; r < K; ++r)
    {
      const uint32_t L = in.len(r);
      uint64_t j = vsxsym::mix64(hash[r]) & mask;
      for (;; j = (j + 1) & mask)
        {
          const uint64_t o = table[j];
          if (o == NONE) { table[j] = r; node[r] = r; ++nodes; break; }
          if (hash[o] == hash[r] && in.len(o) == L && std::memcmp(codes.data() + coff[o], codes.data() + coff[r], L) == 0) { node[r] = o; break; }
        }
    }
  g_stats.nodes = nodes;
  // the claims: every head against the nodes that are proper prefixes of it, at the lengths that occur
  const uint32_t longest = in.lengths.empty() ? 0 : in.lengths.back();
  std::vector<uint8_t> occurs((size_t) longest + 1, 0);
  for (uint32_t L : in.lengths) occurs[L] = 1;
  std::vector<uint64_t> holder(K, NONE), probes((size_t) nth, 0), compared((size_t) nth, 0);
  vsxp::run_pool(nth, [&](int t) {
    uint64_t np = 0, nc = 0;
    for (uint64_t r = (uint64_t) t; r < K; r += (uint64_t) nth)
      {
        if (node[r] != r) continue;
        const uint8_t * c = codes.data() + coff[r];
        const uint32_t L = in.len(r);
        uint64_t h = FNV_BASIS;
        for (uint32_t l = 0; l < L; h = (h ^ c[l]) * FNV_PRIME, ++l)
          {
            if (!occurs[l]) continue;
            for (uint64_t j = vsxsym::mix64(h) & mask;; j = (j + 1) & mask)
              {
                const uint64_t o = table[j];
                ++np;
                if (o == NONE) break;
                if (hash[o] != h || in.len(o) != l) continue;
                ++nc;
                if (std::memcmp(codes.data() + coff[o], c, l) != 0) continue;
                atomic_min(&holder[o], r);
                break;
              }
          }
      }
    probes[(size_t) t] = np; compared[(size_t) t] = nc;
  });
  for (int t = 0; t < nth; ++t) { g_stats.probes += probes[(size_t) t]; g_stats.candidates_compared += compared[(size_t) t]; }
  // the tops: a holder has a higher rank than what it holds, a head a lower one than its duplicates
  top.assign(K, 0);
  for (uint64_t r = K; r-- > 0;)
    if (node[r] == r) top[r] = holder[r] == NONE ? r : top[holder[r]];
  for (uint64_t r = 0; r < K; ++r)
    if (node[r] != r) top[r] = top[node[r]];
  g_stats.reads_host = K;
}

void host_groups(const Input & in, Groups & G)
{
  const uint64_t K = in.order.size();
  std::vector<uint64_t> node, top;
  host_links(in, node, top);
  std::vector<uint64_t> cluster_of_top(K, NONE), count;
  for (uint64_t r = 0; r < K; ++r)
    {
      uint64_t & c = cluster_of_top[top[r]];
      if (c == NONE) { c = G.top.size(); G.top.push_back(top[r]); G.size.push_back(0); count.push_back(0); }
      G.size[c] += in.size(r);
      ++count[c];
    }
  const uint64_t C = G.top.size();
  G.cstart.assign(C + 1, 0);
  for (uint64_t c = 0; c < C; ++c) G.cstart[c + 1] = G.cstart[c] + count[c];
  G.member.resize(K); G.head.resize(K);
  std::vector<uint64_t> at(G.cstart.begin(), G.cstart.end() - 1);
  for (uint64_t r = 0; r < K; ++r) { G.member[at[cluster_of_top[top[r]]]++] = r; G.head[r] = node[r] == r; }
}

// ---- the device route ------------------------------------------------------------------------------------------------------------
struct Events {
  hipEvent_t a = nullptr, b = nullptr, c = nullptr;
  ~Events() { for (hipEvent_t e : { a, b, c }) if (e) (void) hipEventDestroy(e); }
};

// bytes the device route keeps resident for K reads of W code words
uint64_t device_bytes(uint64_t K, uint64_t W, uint64_t T, uint64_t D)
{
  return W * 16 + K * 128 + T * 4 + D * 4 + ((uint64_t) 64 << 20);
}

int device_groups(vsx_ctx * ctx, const Input & in, uint64_t W, Groups & G)
{
  const vsx_derep_prefix_opts & o = *in.o;
  const uint64_t K = in.order.size(), D = in.lengths.size();
  VSX_HIP_AS(WHO, hipSetDevice(vsx_internal_device(ctx)));
  hipStream_t st = vsx_internal_stream(ctx);
  Events ev;
  for (hipEvent_t * e : { &ev.a, &ev.b, &ev.c }) VSX_HIP_AS(WHO, hipEventCreate(e));
  const uint64_t hash_mask = vsxe::hash_mask_from_env("VSX_DEREP_PREFIX_HASH_BITS");
  const uint64_t window = o.window > 0 ? (uint64_t) o.window : WINDOW_READS;

  // ---- stage in rank order, window by window: the words stay on the device; their own hash is not used
  DevBuf<uint64_t> d_words, d_sums, d_hash, d_unused;
  DevBuf<uint8_t> d_text;
  DevBuf<VsxExactItem> d_items;
  PinnedBuf<char> h_text;
  PinnedBuf<VsxExactItem> h_items;
  VSX_HIP_AS(WHO, d_words.alloc(W + 2));
  VSX_HIP_AS(WHO, d_sums.alloc(W + 2));
  VSX_HIP_AS(WHO, d_hash.alloc(K));
  VSX_HIP_AS(WHO, d_unused.alloc(std::min(window, K)));
  std::vector<uint64_t> woff(K);
  std::vector<uint32_t> len(K), length_index(K);
  uint64_t wbase = 0;
  for (uint64_t w0 = 0; w0 < K; w0 += window)
    {
      const double t0 = now_s();
      const uint64_t wn = std::min(window, K - w0);
      VSX_HIP_AS(WHO, ensure_pinned(h_items, wn));
      const vsxe::Plan P = vsxe::plan_items(wn, [&](uint64_t k) { return in.len(w0 + k); }, false, false, h_items.p);
      VSX_HIP_AS(WHO, ensure_pinned(h_text, P.text_bytes));
      for (uint64_t k = 0; k < wn; ++k)
        {
          VsxExactItem & it = h_items.p[k];
          it.woff += wbase;
          woff[w0 + k] = it.woff; len[w0 + k] = it.len;
          if (it.len) std::memcpy(h_text.p + it.off, in.seq(w0 + k), it.len);
        }
      wbase += P.words;
      g_stats.seconds_stage += now_s() - t0;
      VSX_HIP_AS(WHO, d_text.ensure(P.text_bytes));
      VSX_HIP_AS(WHO, d_items.ensure(wn));
      VSX_HIP_AS(WHO, hipEventRecord(ev.a, st));
      VSX_HIP_AS(WHO, hipMemcpyAsync(d_text.p, h_text.p, P.text_bytes, hipMemcpyHostToDevice, st));
      VSX_HIP_AS(WHO, hipMemcpyAsync(d_items.p, h_items.p, wn * sizeof(VsxExactItem), hipMemcpyHostToDevice, st));
      VSX_HIP_AS(WHO, hipEventRecord(ev.b, st));
      VSX_HIP_AS(WHO, vsx_launch_exact_hash(d_items.p, (uint32_t) wn, d_text.p, hash_mask, d_words.p, d_unused.p, st));
      VSX_HIP_AS(WHO, hipEventRecord(ev.c, st));
      VSX_HIP_AS(WHO, hipStreamSynchronize(st));               // the pinned window is staged again
      float ms = 0.f;
      VSX_HIP_AS(WHO, hipEventElapsedTime(&ms, ev.a, ev.b));
      g_stats.seconds_h2d += ms * 1e-3;
      VSX_HIP_AS(WHO, hipEventElapsedTime(&ms, ev.b, ev.c));
      g_stats.seconds_hash += ms * 1e-3;
      ++g_stats.windows;
    }
  if (wbase != W) return fail(VSX_EHIP, "%s: the windows' words do not add up", WHO);
  d_text.release(); d_items.release(); d_unused.release();

  // ---- the per-read arrays
  double t0 = now_s();
  std::vector<uint64_t> ab;
  if (o.sizein && in.reads->abundance) { ab.resize(K); for (uint64_t r = 0; r < K; ++r) ab[r] = in.size(r); }
  for (uint64_t r = 0, d = 0; r < K; ++r)
    {
      while (in.lengths[d] != len[r]) ++d;                     // the reads ascend by length
      length_index[r] = (uint32_t) d;
    }
  g_stats.seconds_stage += now_s() - t0;
  t0 = now_s();
  DevBuf<uint32_t> d_len, d_lidx, d_lengths, d_table, d_root, d_rep, d_count, d_node, d_holder, d_next_a, d_next_b;
  DevBuf<uint64_t> d_woff, d_ab, d_size, d_keys_a, d_keys_b;
  DevBuf<uint8_t> d_temp;
  DevBuf<VsxDerepCounters> d_gcounters;
  DevBuf<VsxDerepPrefixCounters> d_counters;
  int rc;
  VSX_HIP_AS(WHO, upload(d_len, len.data(), K, st));
  VSX_HIP_AS(WHO, upload(d_lidx, length_index.data(), K, st));
  VSX_HIP_AS(WHO, upload(d_lengths, in.lengths.data(), D, st));
  VSX_HIP_AS(WHO, upload(d_woff, woff.data(), K, st));
  if (!ab.empty()) VSX_HIP_AS(WHO, upload(d_ab, ab.data(), K, st));
  const uint64_t table_size = vsxe::table_size_for(K);
  VSX_HIP_AS(WHO, d_table.alloc(table_size));
  VSX_HIP_AS(WHO, d_root.alloc(K)); VSX_HIP_AS(WHO, d_rep.alloc(K)); VSX_HIP_AS(WHO, d_count.alloc(K)); VSX_HIP_AS(WHO, d_size.alloc(K));
  VSX_HIP_AS(WHO, d_node.alloc(K)); VSX_HIP_AS(WHO, d_holder.alloc(K)); VSX_HIP_AS(WHO, d_next_a.alloc(K)); VSX_HIP_AS(WHO, d_next_b.alloc(K));
  VSX_HIP_AS(WHO, d_keys_a.alloc(K)); VSX_HIP_AS(WHO, d_keys_b.alloc(K));
  VSX_HIP_AS(WHO, d_gcounters.alloc(1)); VSX_HIP_AS(WHO, d_counters.alloc(1));
  auto reset_account = [&]() -> int {
    VSX_HIP_AS(WHO, hipMemsetAsync(d_rep.p, 0xFF, K * sizeof(uint32_t), st));
    VSX_HIP_AS(WHO, hipMemsetAsync(d_count.p, 0, K * sizeof(uint32_t), st));
    VSX_HIP_AS(WHO, hipMemsetAsync(d_size.p, 0, K * sizeof(uint64_t), st));
    return VSX_OK;
  };
  VSX_HIP_AS(WHO, hipMemsetAsync(d_table.p, 0xFF, table_size * sizeof(uint32_t), st));
  VSX_HIP_AS(WHO, hipMemsetAsync(d_holder.p, 0xFF, K * sizeof(uint32_t), st));
  VSX_HIP_AS(WHO, hipMemsetAsync(d_gcounters.p, 0, sizeof(VsxDerepCounters), st));
  VSX_HIP_AS(WHO, hipMemsetAsync(d_counters.p, 0, sizeof(VsxDerepPrefixCounters), st));
  if ((rc = reset_account()) != VSX_OK) return rc;

  // ---- scan, group, heads
  VSX_HIP_AS(WHO, hipEventRecord(ev.a, st));
  VSX_HIP_AS(WHO, vsx_launch_derep_prefix_scan((uint32_t) K, d_len.p, d_woff.p, d_words.p, hash_mask, d_sums.p, d_hash.p, st));
  VSX_HIP_AS(WHO, hipEventRecord(ev.b, st));
  VsxDerepReads R {};
  R.n = (uint32_t) K; R.len = d_len.p; R.hash_plus = d_hash.p; R.woff_plus = d_woff.p; R.words = d_words.p;
  VSX_HIP_AS(WHO, vsx_launch_derep_group(R, d_hash.p, d_woff.p, d_table.p, table_size, d_root.p, d_gcounters.p, st));
  VSX_HIP_AS(WHO, vsx_launch_derep_account((uint32_t) K, d_root.p, nullptr, d_rep.p, d_size.p, d_count.p, st));
  VSX_HIP_AS(WHO, vsx_launch_derep_prefix_nodes((uint32_t) K, d_root.p, d_rep.p, d_node.p, st));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  float ms = 0.f;
  VSX_HIP_AS(WHO, hipEventElapsedTime(&ms, ev.a, ev.b));
  g_stats.seconds_hash += ms * 1e-3;
  g_stats.seconds_group += now_s() - t0;

  // ---- claim
  t0 = now_s();
  VsxDerepPrefixClaim Q {};
  Q.n = (uint32_t) K; Q.n_lengths = (uint32_t) D; Q.len = d_len.p; Q.length_index = d_lidx.p; Q.lengths = d_lengths.p; Q.woff = d_woff.p;
  Q.words = d_words.p; Q.sums = d_sums.p; Q.hash = d_hash.p; Q.node = d_node.p; Q.table = d_table.p; Q.table_size = table_size;
  Q.hash_mask = hash_mask; Q.holder = d_holder.p; Q.counters = d_counters.p;
  VSX_HIP_AS(WHO, vsx_launch_derep_prefix_claim(Q, st));
  VsxDerepPrefixCounters counters {};
  VSX_HIP_AS(WHO, hipMemcpyAsync(&counters, d_counters.p, sizeof counters, hipMemcpyDeviceToHost, st));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  g_stats.probes = counters.probes;
  g_stats.candidates_compared = counters.candidates_compared;
  g_stats.seconds_claim += now_s() - t0;

  // ---- resolve: the longest path (duplicate -> head -> holder -> ...) has at most D links
  t0 = now_s();
  VSX_HIP_AS(WHO, vsx_launch_derep_prefix_link((uint32_t) K, d_node.p, d_holder.p, d_next_a.p, st));
  uint32_t * from = d_next_a.p, * to = d_next_b.p;
  for (uint64_t reach = 1; reach < D + 1; reach *= 2)
    {
      VSX_HIP_AS(WHO, vsx_launch_derep_prefix_jump((uint32_t) K, from, to, st));
      std::swap(from, to);
    }
  const uint32_t * const d_top = from;
  if ((rc = reset_account()) != VSX_OK) return rc;
  size_t temp_bytes = 0;
  VSX_HIP_AS(WHO, vsx_launch_derep_members((uint32_t) K, d_top, d_rep.p, d_keys_a.p, d_keys_b.p, nullptr, &temp_bytes, st));
  VSX_HIP_AS(WHO, d_temp.alloc(temp_bytes));
  VSX_HIP_AS(WHO, vsx_launch_derep_account((uint32_t) K, d_top, ab.empty() ? nullptr : d_ab.p, d_rep.p, d_size.p, d_count.p, st));
  VSX_HIP_AS(WHO, vsx_launch_derep_members((uint32_t) K, d_top, d_rep.p, d_keys_a.p, d_keys_b.p, d_temp.p, &temp_bytes, st));
  std::vector<uint64_t> keys(K), csize(K);
  std::vector<uint32_t> top(K), node(K), ccount(K);
  VSX_HIP_AS(WHO, hipMemcpyAsync(keys.data(), d_keys_b.p, K * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  VSX_HIP_AS(WHO, hipMemcpyAsync(csize.data(), d_size.p, K * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  VSX_HIP_AS(WHO, hipMemcpyAsync(top.data(), d_top, K * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  VSX_HIP_AS(WHO, hipMemcpyAsync(node.data(), d_node.p, K * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  VSX_HIP_AS(WHO, hipMemcpyAsync(ccount.data(), d_count.p, K * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  G.member.resize(K); G.head.resize(K);
  uint64_t nodes = 0;
  for (uint64_t p = 0; p < K; ++p)
    {
      const uint64_t low = keys[p] >> 32, r = keys[p] & 0xFFFFFFFFull;
      if (low >= K || r >= K || top[r] >= K || node[r] > r || top[r] < node[r] || node[top[r]] != top[r] || top[top[r]] != top[r])
        return fail(VSX_EHIP, "%s: the member list names a read that is not there", WHO);
      if (p == 0 || low != keys[p - 1] >> 32)
        {
          if (r != low) return fail(VSX_EHIP, "%s: a cluster does not begin with its lowest rank", WHO);
          G.cstart.push_back(p);
          G.top.push_back(top[r]);
          G.size.push_back(csize[top[r]]);
        }
      else if (top[r] != G.top.back()) return fail(VSX_EHIP, "%s: a cluster has two tops", WHO);
      G.member[p] = r;
      G.head[r] = node[r] == r;
      nodes += node[r] == r;
    }
  G.cstart.push_back(K);
  for (uint64_t c = 0; c + 1 < G.cstart.size(); ++c)
    if (ccount[G.top[c]] != G.cstart[c + 1] - G.cstart[c]) return fail(VSX_EHIP, "%s: a cluster's count differs from its member list", WHO);
  g_stats.nodes = nodes;
  g_stats.seconds_resolve += now_s() - t0;
  return VSX_OK;
}

// ---- the caller's output -----------------------------------------------------------------------------------------------------------
void release(vsx_derep_prefix_out * out)
{
  std::free(out->rep); std::free(out->size); std::free(out->count); std::free(out->member_start); std::free(out->member); std::free(out->rank);
  std::memset(out, 0, sizeof *out);
}


int finish(const Input & in, const Groups & G, vsx_derep_prefix_out & out)
{
  const vsx_derep_prefix_opts & o = *in.o;
  const uint64_t K = in.order.size(), C = G.top.size();
  // derep_compare_prefix: size descending, strcmp of the representatives' labels, the representative's place in the sorted order
  std::vector<uint64_t> order(C);
  std::iota(order.begin(), order.end(), (uint64_t) 0);
  std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
    if (G.size[a] != G.size[b]) return G.size[a] > G.size[b];
    const int cmp = label_cmp(in.label(G.top[a]), in.label_len(G.top[a]), in.label(G.top[b]), in.label_len(G.top[b]));
    if (cmp != 0) return cmp < 0;
    return G.top[a] < G.top[b];
  });
  out.n_clusters = C;
  out.rep = array_of<uint64_t>(C); out.size = array_of<uint64_t>(C); out.count = array_of<uint64_t>(C);
  out.member_start = array_of<uint64_t>(C + 1); out.member = array_of<uint64_t>(K); out.rank = array_of<uint64_t>(out.n);
  if (!out.rep || !out.size || !out.count || !out.member_start || !out.member || !out.rank) return fail(VSX_ENOMEM, "%s: out of memory", WHO);
  for (uint64_t k = 0; k < out.n; ++k) out.rank[k] = UINT64_MAX;
  for (uint64_t r = 0; r < K; ++r) out.rank[in.order[r]] = r;
  uint64_t at = 0, in_range = 0;
  for (uint64_t i = 0; i < C; ++i)
    {
      const uint64_t c = order[i], first = G.cstart[c], members = G.cstart[c + 1] - first;
      out.rep[i] = in.order[G.top[c]]; out.size[i] = G.size[c]; out.count[i] = members;
      out.member_start[i] = at;
      // the --uc order: the heads of the chain's nodes from the longest down, then the duplicates as the walk met them
      for (uint64_t m = members; m-- > 0;)
        if (G.head[G.member[first + m]]) out.member[at++] = in.order[G.member[first + m]];
      for (uint64_t m = 0; m < members; ++m)
        if (!G.head[G.member[first + m]]) out.member[at++] = in.order[G.member[first + m]];
      if (out.member[out.member_start[i]] != out.rep[i]) return fail(VSX_EHIP, "%s: a cluster does not begin with its representative", WHO);
      out.sumsize += G.size[c];
      out.maxsize = std::max(out.maxsize, G.size[c]);
      if ((int64_t) G.size[c] >= o.minuniquesize && (int64_t) G.size[c] <= o.maxuniquesize) ++in_range;
    }
  out.member_start[C] = at;
  out.selected = std::min<uint64_t>(in_range, o.topn < 0 ? 0 : (uint64_t) o.topn);
  if (C == 0) out.median = 0.0;
  else if (C % 2) out.median = (double) out.size[(C - 1) / 2];
  else out.median = (double) (out.size[C / 2 - 1] + out.size[C / 2]) / 2.0;
  return VSX_OK;
}

}  // namespace

extern "C" {

void vsx_derep_prefix_opts_default(vsx_derep_prefix_opts * o)
{
  std::memset(o, 0, sizeof *o);
  o->minseqlength = 32; o->maxseqlength = 50000;
  o->minuniquesize = 1; o->maxuniquesize = INT64_MAX; o->topn = INT64_MAX;
}

void vsx_derep_prefix_last_stats(vsx_derep_prefix_stats * out) { if (out) *out = g_stats; }

void vsx_derep_prefix_out_free(vsx_derep_prefix_out * out) { if (out) release(out); }

int vsx_derep_prefix(vsx_ctx * ctx, const vsx_derep_prefix_opts * opts, uint64_t n, const vsx_fastx_reads * reads, const char * label_blob,
                     const uint64_t * label_off, vsx_derep_prefix_out * out)
{
  g_stats = vsx_derep_prefix_stats {};
  const double t_begin = now_s();
  if (!opts || !out || !reads || (n && (!reads->seq || !reads->off || !reads->len || !label_blob || !label_off)))
    return fail(VSX_EINVAL, "%s: null argument", WHO);
  std::memset(out, 0, sizeof *out);
  const vsx_derep_prefix_opts & o = *opts;
  if (o.window < 0) return fail(VSX_EINVAL, "%s: window cannot be negative", WHO);

  // ---- the discards, the counts of the first log line, the refusals
  Input in { opts, reads, label_blob, label_off, {}, {} };
  std::vector<uint64_t> kept;
  out->n = n;
  uint64_t shortest = UINT64_MAX, W = 0, sum = 0;
  for (uint64_t k = 0; k < n; ++k)
    {
      if (reads->off[k] > reads->bytes || reads->len[k] > reads->bytes - reads->off[k]) return fail(VSX_EINVAL, "%s: a read exceeds its blob", WHO);
      if (label_off[k + 1] < label_off[k]) return fail(VSX_EINVAL, "%s: the label offsets decrease", WHO);
      const int64_t L = reads->len[k];
      if (L < o.minseqlength) { ++out->discarded_short; continue; }
      if (L > o.maxseqlength) { ++out->discarded_long; continue; }
      const uint64_t ab = reads->abundance ? reads->abundance[k] : 1;
      if (ab == 0) return fail(VSX_EINVAL, "%s: read %llu has abundance 0", WHO, (unsigned long long) k);
      if (ab >= SIZE_LIMIT) return fail(VSX_EINVAL, "%s: read %llu has an abundance of 2^32 or more", WHO, (unsigned long long) k);
      if ((sum += o.sizein ? ab : 1) >= SIZE_LIMIT)
        return fail(VSX_EINVAL, "%s: the sizes sum to 2^32 or more (the reference's 32-bit cluster size would wrap)", WHO);
      kept.push_back(k);
      out->nucleotides += (uint64_t) L;
      shortest = std::min<uint64_t>(shortest, (uint64_t) L);
      out->longest = std::max<uint64_t>(out->longest, (uint64_t) L);
      W += vsxe::words_of((uint32_t) L);
    }
  const uint64_t K = kept.size();
  out->kept = K;
  out->shortest = K ? shortest : 0;
  double t0 = now_s();
  rank_reads(in, kept);
  g_stats.seconds_rank = now_s() - t0;
  g_stats.distinct_lengths = in.lengths.size();

  // ---- the route
  const uint64_t most_reads = (uint64_t) UINT32_MAX - 1;                                  // testing aid: a lower limit of the device route
  const uint64_t device_reads = std::min(most_reads, vsxp::env_u64("VSX_DEREP_PREFIX_DEVICE_READS", most_reads, true));
  bool host_all = true;
  if (!ctx) g_stats.host_no_context = 1;
  else if (vsxp::env_is_host("VSX_DEREP_PREFIX")) g_stats.host_environment = 1;
  else if (K > device_reads) g_stats.host_read_count = 1;
  else host_all = false;
  Groups G;
  int rc = VSX_OK;
  if (!host_all && K)
    {
      bool fits = false;                                                                  // (the testing aid: what the words are taken to need)
      rc = vsxp::device_fits(ctx, WHO, device_bytes(K, W, vsxe::table_size_for(K), in.lengths.size()), "VSX_DEREP_PREFIX_PRETEND_BYTES", &fits);
      if (rc != VSX_OK) return rc;
      if (!fits) { host_all = true; g_stats.host_memory = 1; }      // the host, as a whole
    }
  if (host_all || K == 0) host_groups(in, G);
  else rc = device_groups(ctx, in, W, G);
  if (rc == VSX_OK)
    {
      t0 = now_s();
      rc = finish(in, G, *out);
      g_stats.seconds_output += now_s() - t0;
    }
  if (rc != VSX_OK) { release(out); return rc; }
  g_stats.seconds_total = now_s() - t_begin;
  return VSX_OK;
}

}  // extern "C"
