// vsx_otutab.cpp -- the OTU table (include/vsx_otutab.h: vsx_otutab), the host side of vsx_otutab.hip and the host restatement.
//
// Restated from the reference (src/, v2.31.0): core/otutable.cpp: otutable_add() -- the three annotations and their fallbacks, the
// sets, the counts, the taxonomy map -- and the calls of it in commands/usearch_global.cpp, commands/search_exact.cpp and
// core/cluster.cpp, which the caller folds into (q_target, t_matched).
//
// Both routes end in the same intermediate form (Mid): the distinct names as spans of the caller's blobs in memcmp order, a rank per
// query and per target that takes part, the cells as sorted (OTU << 32 | sample, sum) pairs, a taxonomy span per OTU.  finish() turns
// it into the caller's result.
//
//   device   scan -> sort by hash -> head flags -> prefix sum -> one representative per group to the host, which sorts and merges
//            them and sends a rank per group back -> keys -> sort -> sums per cell, last tax= add per OTU (vsx_otutab.hip).  All
//            device memory comes from the context's scratch pool; every buffer a kernel reads was written by this call.
//   host     scan_name / scan_tax below (memchr and memcmp, no regular expression), the distinct names through per-thread hash
//            maps whose keys are sorted once, the cells through per-thread maps merged in key order, the taxonomy through a
//            compare-and-swap maximum of the add numbers.  Written from the rule and not from the kernels.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string_view>
#include <unordered_map>

#include "../../include/vsx_otutab.h"
#include "vsx_otutab_internal.h"
#include "vsx_private.h"

using vsxp::fail;
using vsxp::array_of;
using vsxp::download;
using vsxp::now_s;
using vsxp::Scratch;

namespace {

constexpr const char * WHO = "vsx_otutab";
constexpr uint32_t NONE = VSX_OTUTAB_NONE;
constexpr uint64_t LABEL_LIMIT = (uint64_t) UINT32_MAX - 1;
constexpr int HOST_THREADS = 16;

thread_local vsx_otutab_stats g_stats {};

struct Span { uint64_t off; uint32_t len; };

struct Mid {
  std::vector<Span> samples, otus;            // sorted; spans of the query blob / the target blob
  std::vector<Span> tax;                      // per OTU: span of the target blob, len NONE without a taxonomy
  std::vector<uint32_t> q_sample, t_otu;
  std::vector<uint64_t> cell_key, cell_sum;   // ascending keys: OTU rank << 32 | sample rank
};

struct Input {
  const vsx_labels * Q, * T;
  const uint64_t * q_ab;
  const uint32_t * q_target;
  const uint8_t * t_matched;
  int nth;
  uint64_t nq() const { return Q->n; }
  uint64_t nt() const { return T->n; }
  uint64_t ab(uint64_t k) const { return q_ab ? q_ab[k] : 1; }
};

inline int threads_for(const Input & in, uint64_t n) { return (int) std::max<uint64_t>(1, std::min<uint64_t>((uint64_t) in.nth, n / 4096 + 1)); }

// ---- the label scan of the host --------------------------------------------------------------------------------------------------
// the leftmost p with (p == 0 or s[p - 1] == ';') at which one of the keywords stands: its value, up to the next ';' or the end
template <size_t NK>
bool scan_value(const unsigned char * s, uint64_t L, const std::string_view (&kw)[NK], uint64_t & vstart, uint64_t & vlen)
{
  for (uint64_t p = 0;;)
    {
      for (const std::string_view & k : kw)
        if (k.size() <= L - p && std::memcmp(s + p, k.data(), k.size()) == 0)
          {
            vstart = p + k.size();
            const void * e = std::memchr(s + vstart, ';', L - vstart);
            vlen = (e ? (uint64_t) (static_cast<const unsigned char *>(e) - s) : L) - vstart;
            return true;
          }
      const void * semi = std::memchr(s + p, ';', L - p);
      if (!semi) return false;
      p = (uint64_t) (static_cast<const unsigned char *>(semi) - s) + 1;
    }
}

constexpr std::string_view KW_SAMPLE[2] = { "sample=", "barcodelabel=" }, KW_OTU[1] = { "otu=" }, KW_TAX[1] = { "tax=" };

inline bool word_byte(unsigned char c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') || c == '_'; }

Span sample_of(const vsx_labels & Q, uint64_t k)
{
  const unsigned char * s = reinterpret_cast<const unsigned char *>(Q.blob) + Q.offsets[k];
  const uint64_t L = Q.lengths[k];
  uint64_t a = 0, n = 0;
  if (scan_value(s, L, KW_SAMPLE, a, n)) return Span { Q.offsets[k] + a, (uint32_t) n };
  while (n < L && word_byte(s[n])) ++n;
  return Span { Q.offsets[k], (uint32_t) n };
}

Span otu_of(const vsx_labels & T, uint64_t k)
{
  const unsigned char * s = reinterpret_cast<const unsigned char *>(T.blob) + T.offsets[k];
  const uint64_t L = T.lengths[k];
  uint64_t a = 0, n = 0;
  if (scan_value(s, L, KW_OTU, a, n)) return Span { T.offsets[k] + a, (uint32_t) n };
  const void * e = std::memchr(s, ';', L);
  return Span { T.offsets[k], (uint32_t) (e ? (uint64_t) (static_cast<const unsigned char *>(e) - s) : L) };
}

Span tax_of(const vsx_labels & T, uint64_t k)
{
  const unsigned char * s = reinterpret_cast<const unsigned char *>(T.blob) + T.offsets[k];
  uint64_t a = 0, n = 0;
  if (scan_value(s, T.lengths[k], KW_TAX, a, n)) return Span { T.offsets[k] + a, (uint32_t) n };
  return Span { 0, NONE };
}

inline std::string_view view(const char * blob, const Span & s) { return std::string_view(blob + s.off, s.len); }

// the distinct names among the spans with len != NONE, in memcmp order (the shorter first on a tie: std::string's order), and the
// rank of every such span
void rank_names(const Input & in, const char * blob, const std::vector<Span> & spans, std::vector<Span> & sorted, std::vector<uint32_t> & rank)
{
  const uint64_t n = spans.size();
  const int nth = threads_for(in, n);
  rank.assign(n, NONE);
  std::vector<std::vector<Span>> keys((size_t) nth);
  vsxp::run_pool(nth, [&](int t) {
    std::unordered_map<std::string_view, uint32_t> seen;
    for (uint64_t i = n * (uint64_t) t / (uint64_t) nth, e = n * (uint64_t) (t + 1) / (uint64_t) nth; i < e; ++i)
      {
        if (spans[i].len == NONE) continue;
        const auto it = seen.emplace(view(blob, spans[i]), (uint32_t) keys[(size_t) t].size());
        if (it.second) keys[(size_t) t].push_back(spans[i]);
        rank[i] = it.first->second;                            // the thread's own number of the name, for now
      }
  });
  for (const auto & k : keys) sorted.insert(sorted.end(), k.begin(), k.end());
  const auto less = [&](const Span & a, const Span & b) { return view(blob, a) < view(blob, b); };      // char_traits<char>: unsigned bytes
  std::sort(sorted.begin(), sorted.end(), less);
  sorted.erase(std::unique(sorted.begin(), sorted.end(), [&](const Span & a, const Span & b) { return view(blob, a) == view(blob, b); }), sorted.end());
  vsxp::run_pool(nth, [&](int t) {
    std::vector<uint32_t> global(keys[(size_t) t].size());
    for (size_t j = 0; j < global.size(); ++j)
      global[j] = (uint32_t) (std::lower_bound(sorted.begin(), sorted.end(), keys[(size_t) t][j], less) - sorted.begin());
    for (uint64_t i = n * (uint64_t) t / (uint64_t) nth, e = n * (uint64_t) (t + 1) / (uint64_t) nth; i < e; ++i)
      if (rank[i] != NONE) rank[i] = global[rank[i]];
  });
}

inline void atomic_max(uint64_t * p, uint64_t v)
{
  uint64_t cur = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (v > cur && !__atomic_compare_exchange_n(p, &cur, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
}

// takes[t]: target t stands in an add (the first hit of a query, or the unmatched pass)
void targets_in_adds(const Input & in, std::vector<uint8_t> & takes)
{
  takes.assign(in.nt(), 0);
  for (uint64_t k = 0; k < in.nq(); ++k) if (in.q_target[k] != NONE) takes[in.q_target[k]] = 1;
  if (in.t_matched) for (uint64_t t = 0; t < in.nt(); ++t) if (!in.t_matched[t]) takes[t] = 1;
}

int host_mid(const Input & in, Mid & M)
{
  const uint64_t nq = in.nq(), nt = in.nt();
  double t0 = now_s();
  std::vector<uint8_t> takes;
  targets_in_adds(in, takes);
  g_stats.seconds_stage += now_s() - t0;
  // scan
  t0 = now_s();
  std::vector<Span> qs(nq), ts(nt), tt(nt);
  vsxp::run_pool(threads_for(in, nq), [&](int t) {
    const uint64_t nth = (uint64_t) threads_for(in, nq);
    for (uint64_t k = nq * (uint64_t) t / nth, e = nq * (uint64_t) (t + 1) / nth; k < e; ++k) qs[k] = sample_of(*in.Q, k);
  });
  for (uint64_t t = 0; t < nt; ++t)
    {
      ts[t] = takes[t] ? otu_of(*in.T, t) : Span { 0, NONE };
      tt[t] = takes[t] ? tax_of(*in.T, t) : Span { 0, NONE };
      g_stats.targets_in_adds += takes[t];
    }
  g_stats.seconds_scan += now_s() - t0;
  // names
  t0 = now_s();
  rank_names(in, in.Q->blob, qs, M.samples, M.q_sample);
  rank_names(in, in.T->blob, ts, M.otus, M.t_otu);
  g_stats.seconds_rank += now_s() - t0;
  if (M.samples.size() > LABEL_LIMIT || M.otus.size() > LABEL_LIMIT) return fail(VSX_EINVAL, "%s: more than 2^32 - 2 distinct names", WHO);
  // cells, and per OTU the number (+ 1) of the last add whose target carries tax=
  t0 = now_s();
  const int nth = threads_for(in, nq);
  std::vector<uint64_t> last(M.otus.size(), 0);
  std::vector<std::unordered_map<uint64_t, uint64_t>> part((size_t) nth);
  vsxp::run_pool(nth, [&](int t) {
    auto & cells = part[(size_t) t];
    for (uint64_t k = nq * (uint64_t) t / (uint64_t) nth, e = nq * (uint64_t) (t + 1) / (uint64_t) nth; k < e; ++k)
      {
        const uint32_t tg = in.q_target[k];
        if (tg == NONE) continue;
        if (tt[tg].len != NONE) atomic_max(&last[M.t_otu[tg]], k + 1);
        if (in.ab(k)) cells[((uint64_t) M.t_otu[tg] << 32) | M.q_sample[k]] += in.ab(k);
      }
  });
  if (in.t_matched)
    for (uint64_t t = 0; t < nt; ++t)
      if (!in.t_matched[t] && tt[t].len != NONE) last[M.t_otu[t]] = std::max(last[M.t_otu[t]], nq + t + 1);
  std::vector<std::pair<uint64_t, uint64_t>> all;
  for (const auto & cells : part) all.insert(all.end(), cells.begin(), cells.end());
  std::sort(all.begin(), all.end(), [](const auto & a, const auto & b) { return a.first < b.first; });
  for (const auto & c : all)
    if (!M.cell_key.empty() && M.cell_key.back() == c.first) M.cell_sum.back() += c.second;
    else { M.cell_key.push_back(c.first); M.cell_sum.push_back(c.second); }
  M.tax.assign(M.otus.size(), Span { 0, NONE });
  for (uint64_t r = 0; r < M.otus.size(); ++r)
    if (last[r]) M.tax[r] = tt[last[r] <= nq ? in.q_target[last[r] - 1] : last[r] - 1 - nq];
  g_stats.seconds_accumulate += now_s() - t0;
  g_stats.labels_host = nq + g_stats.targets_in_adds;
  return VSX_OK;
}

// ---- the device route ------------------------------------------------------------------------------------------------------------
uint64_t device_bytes(const Input & in) { return in.Q->bytes + in.T->bytes + 200 * (in.nq() + in.nt()) + ((uint64_t) 64 << 20); }

// the buffers of one grouping, sized for the larger side and used by both in turn
struct GroupBufs {
  Scratch<uint32_t> idx_in, idx_out, flag, incl, rep_item, rep_len, rank;
  Scratch<uint64_t> hash_sorted, rep_off;
  Scratch<uint8_t> temp;
  size_t temp_bytes = 0;
};

struct DeviceBufs {
  Scratch<uint8_t> qblob, tblob;
  Scratch<uint64_t> qoff, toff, qab, q_name_off, t_name_off, q_hash, t_hash, t_tax_off;
  Scratch<uint32_t> qlen, tlen, qtarget, tlist, unmatched, q_name_len, t_name_len, t_tax_len, q_group, t_group, q_sample, t_item_rank, t_otu;
  GroupBufs G;
  Scratch<uint64_t> keys_in, keys_out, count, ukeys, usum;
  Scratch<uint32_t> vals_in, vals_out, otu, taxseq, uotu, umax, n_unique;
  Scratch<uint8_t> temp;
};

// sort the items by hash, flag the heads, number the groups, fetch one representative each; the host sorts and merges the
// representatives' names and sends rank[group] back; item_rank (and label_rank through the list) receive the ranks
int group_side(vsx_ctx * ctx, hipStream_t st, const Input & in, GroupBufs & G, uint32_t n, const uint8_t * d_blob, const char * h_blob, uint64_t h_bytes,
               const uint64_t * d_hash, const uint64_t * d_name_off, const uint32_t * d_name_len, uint32_t end_bit, uint32_t * d_group, const uint32_t * d_list,
               uint32_t * d_item_rank, uint32_t * d_label_rank, std::vector<Span> & sorted, uint64_t & groups)
{
  groups = 0;
  if (n == 0) return VSX_OK;
  double t0 = now_s();
  size_t sort_bytes = 0, sum_bytes = 0;
  VSX_HIP_AS(WHO, vsx_launch_otutab_sort(nullptr, &sort_bytes, nullptr, nullptr, nullptr, nullptr, n, end_bit, st));
  VSX_HIP_AS(WHO, vsx_launch_otutab_flagsum(nullptr, &sum_bytes, nullptr, nullptr, n, st));
  if (!G.temp.p || std::max(sort_bytes, sum_bytes) > G.temp_bytes)
    {
      G.temp_bytes = std::max(sort_bytes, sum_bytes);
      VSX_HIP_AS(WHO, G.temp.alloc(ctx, G.temp_bytes));
    }
  VSX_HIP_AS(WHO, vsx_launch_otutab_iota(n, G.idx_in.p, st));
  VSX_HIP_AS(WHO, vsx_launch_otutab_sort(G.temp.p, &G.temp_bytes, d_hash, G.hash_sorted.p, G.idx_in.p, G.idx_out.p, n, end_bit, st));
  VSX_HIP_AS(WHO, vsx_launch_otutab_heads(n, G.hash_sorted.p, G.idx_out.p, d_blob, d_name_off, d_name_len, G.flag.p, st));
  VSX_HIP_AS(WHO, vsx_launch_otutab_flagsum(G.temp.p, &G.temp_bytes, G.flag.p, G.incl.p, n, st));
  VSX_HIP_AS(WHO, vsx_launch_otutab_groups(n, G.flag.p, G.incl.p, G.idx_out.p, d_name_off, d_name_len, d_group, G.rep_item.p, G.rep_off.p, G.rep_len.p, st));
  uint32_t ng = 0;
  VSX_HIP_AS(WHO, hipMemcpyAsync(&ng, G.incl.p + (n - 1), sizeof ng, hipMemcpyDeviceToHost, st));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  g_stats.seconds_group += now_s() - t0;
  if (ng == 0 || ng > n) return fail(VSX_EHIP, "%s: the grouping counts %u groups of %u items", WHO, ng, n);
  // ---- rank: O(groups) on the host
  t0 = now_s();
  std::vector<uint64_t> off;
  std::vector<uint32_t> len;
  VSX_HIP_AS(WHO, download(off, G.rep_off.p, ng, st));
  VSX_HIP_AS(WHO, download(len, G.rep_len.p, ng, st));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  std::vector<Span> reps(ng);
  for (uint32_t g = 0; g < ng; ++g)
    {
      if (off[g] > h_bytes || len[g] > h_bytes - off[g]) return fail(VSX_EHIP, "%s: a representative's name lies outside the blob", WHO);
      reps[g] = Span { off[g], len[g] };
    }
  std::vector<uint32_t> rank;
  Input small = in;
  small.nth = ng < 65536 ? 1 : in.nth;
  rank_names(small, h_blob, reps, sorted, rank);
  VSX_HIP_AS(WHO, hipMemcpyAsync(G.rank.p, rank.data(), (size_t) ng * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  VSX_HIP_AS(WHO, vsx_launch_otutab_assign(n, d_group, G.rank.p, d_list, d_item_rank, d_label_rank, st));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));                   // `rank` is pageable and leaves scope
  g_stats.seconds_rank += now_s() - t0;
  groups = ng;
  return VSX_OK;
}

inline uint32_t bits_for(uint64_t v) { uint32_t b = 0; while (b < 64 && (v >> b)) ++b; return b; }

int device_mid_run(vsx_ctx * ctx, hipStream_t st, const Input & in, DeviceBufs & B, Mid & M)
{
  const vsx_labels & Q = *in.Q, & T = *in.T;
  const uint32_t nq = (uint32_t) Q.n, nt = (uint32_t) T.n;
  uint64_t hash_mask = ~0ull;
  uint32_t hash_bits = 64;
  if (const char * env = std::getenv("VSX_OTUTAB_HASH_BITS"))      // (not vsxp::env_u64: a signed value, used only within 1 .. 63)
    {
      const long b = std::strtol(env, nullptr, 10);
      if (b >= 1 && b < 64) { hash_bits = (uint32_t) b; hash_mask = (1ull << b) - 1; }
    }
  // ---- stage: who takes part, the uploads
  double t0 = now_s();
  std::vector<uint8_t> takes;
  targets_in_adds(in, takes);
  std::vector<uint32_t> tlist, unmatched;
  for (uint32_t t = 0; t < nt; ++t)
    {
      if (takes[t]) tlist.push_back(t);
      if (in.t_matched && !in.t_matched[t]) unmatched.push_back(t);
    }
  const uint32_t np = (uint32_t) tlist.size(), nu = (uint32_t) unmatched.size(), ne = nq + nu, nmax = std::max(nq, np);
  g_stats.targets_in_adds = np;
  g_stats.adds_sorted = ne;
  VSX_HIP_AS(WHO, B.qblob.upload(ctx, reinterpret_cast<const uint8_t *>(Q.blob), Q.bytes, st));
  VSX_HIP_AS(WHO, B.qoff.upload(ctx, Q.offsets, nq, st));
  VSX_HIP_AS(WHO, B.qlen.upload(ctx, Q.lengths, nq, st));
  VSX_HIP_AS(WHO, B.qtarget.upload(ctx, in.q_target, nq, st));
  if (in.q_ab) VSX_HIP_AS(WHO, B.qab.upload(ctx, in.q_ab, nq, st));
  VSX_HIP_AS(WHO, B.tblob.upload(ctx, reinterpret_cast<const uint8_t *>(T.blob), T.bytes, st));
  VSX_HIP_AS(WHO, B.toff.upload(ctx, T.offsets, nt, st));
  VSX_HIP_AS(WHO, B.tlen.upload(ctx, T.lengths, nt, st));
  VSX_HIP_AS(WHO, B.tlist.upload(ctx, tlist.data(), np, st));
  VSX_HIP_AS(WHO, B.unmatched.upload(ctx, unmatched.data(), nu, st));
  VSX_HIP_AS(WHO, B.q_name_off.alloc(ctx, nq)); VSX_HIP_AS(WHO, B.q_name_len.alloc(ctx, nq)); VSX_HIP_AS(WHO, B.q_hash.alloc(ctx, nq));
  VSX_HIP_AS(WHO, B.t_name_off.alloc(ctx, np)); VSX_HIP_AS(WHO, B.t_name_len.alloc(ctx, np)); VSX_HIP_AS(WHO, B.t_hash.alloc(ctx, np));
  VSX_HIP_AS(WHO, B.t_tax_off.alloc(ctx, nt)); VSX_HIP_AS(WHO, B.t_tax_len.alloc(ctx, nt));
  VSX_HIP_AS(WHO, B.q_group.alloc(ctx, nq)); VSX_HIP_AS(WHO, B.t_group.alloc(ctx, np));
  VSX_HIP_AS(WHO, B.q_sample.alloc(ctx, nq)); VSX_HIP_AS(WHO, B.t_item_rank.alloc(ctx, np)); VSX_HIP_AS(WHO, B.t_otu.alloc(ctx, nt));
  GroupBufs & G = B.G;
  for (Scratch<uint32_t> * b : { &G.idx_in, &G.idx_out, &G.flag, &G.incl, &G.rep_item, &G.rep_len, &G.rank }) VSX_HIP_AS(WHO, b->alloc(ctx, nmax));
  VSX_HIP_AS(WHO, G.hash_sorted.alloc(ctx, nmax)); VSX_HIP_AS(WHO, G.rep_off.alloc(ctx, nmax));
  // the targets outside every add keep NONE; their taxonomy spans are never read
  VSX_HIP_AS(WHO, hipMemsetAsync(B.t_otu.p, 0xFF, std::max<size_t>(nt, 1) * sizeof(uint32_t), st));
  VSX_HIP_AS(WHO, hipMemsetAsync(B.t_tax_len.p, 0xFF, std::max<size_t>(nt, 1) * sizeof(uint32_t), st));
  VSX_HIP_AS(WHO, hipMemsetAsync(B.t_tax_off.p, 0, std::max<size_t>(nt, 1) * sizeof(uint64_t), st));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  g_stats.seconds_stage += now_s() - t0;

  // ---- scan
  t0 = now_s();
  VsxOtutabScan S {};
  S.n = nq; S.list = nullptr; S.blob = B.qblob.p; S.off = B.qoff.p; S.len = B.qlen.p; S.hash_mask = hash_mask;
  S.name_off = B.q_name_off.p; S.name_len = B.q_name_len.p; S.hash = B.q_hash.p;
  VSX_HIP_AS(WHO, vsx_launch_otutab_scan(S, 0, st));
  S.n = np; S.list = B.tlist.p; S.blob = B.tblob.p; S.off = B.toff.p; S.len = B.tlen.p;
  S.name_off = B.t_name_off.p; S.name_len = B.t_name_len.p; S.hash = B.t_hash.p; S.tax_off = B.t_tax_off.p; S.tax_len = B.t_tax_len.p;
  VSX_HIP_AS(WHO, vsx_launch_otutab_scan(S, 1, st));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  g_stats.seconds_scan += now_s() - t0;
  g_stats.labels_device = (uint64_t) nq + np;

  // ---- group and rank, side by side
  int rc;
  if ((rc = group_side(ctx, st, in, G, nq, B.qblob.p, Q.blob, Q.bytes, B.q_hash.p, B.q_name_off.p, B.q_name_len.p, hash_bits, B.q_group.p, nullptr,
                       B.q_sample.p, nullptr, M.samples, g_stats.query_groups)) != VSX_OK) return rc;
  if ((rc = group_side(ctx, st, in, G, np, B.tblob.p, T.blob, T.bytes, B.t_hash.p, B.t_name_off.p, B.t_name_len.p, hash_bits, B.t_group.p, B.tlist.p,
                       B.t_item_rank.p, B.t_otu.p, M.otus, g_stats.target_groups)) != VSX_OK) return rc;
  const uint32_t n_otus = (uint32_t) M.otus.size();

  // ---- accumulate
  t0 = now_s();
  std::vector<uint32_t> uotu, umax;
  std::vector<uint64_t> ukeys, usum;
  if (ne)
    {
      for (Scratch<uint64_t> * p : { &B.keys_in, &B.keys_out, &B.count, &B.ukeys, &B.usum }) VSX_HIP_AS(WHO, p->alloc(ctx, ne));
      for (Scratch<uint32_t> * p : { &B.vals_in, &B.vals_out, &B.otu, &B.taxseq, &B.uotu, &B.umax }) VSX_HIP_AS(WHO, p->alloc(ctx, ne));
      VSX_HIP_AS(WHO, B.n_unique.alloc(ctx, 2));
      size_t ta = 0, tb = 0, tc = 0;
      VSX_HIP_AS(WHO, vsx_launch_otutab_sort(nullptr, &ta, nullptr, nullptr, nullptr, nullptr, ne, 32 + bits_for(n_otus), st));
      VSX_HIP_AS(WHO, vsx_launch_otutab_reduce_cells(nullptr, &tb, nullptr, nullptr, ne, nullptr, nullptr, nullptr, st));
      VSX_HIP_AS(WHO, vsx_launch_otutab_reduce_tax(nullptr, &tc, nullptr, nullptr, ne, nullptr, nullptr, nullptr, st));
      size_t temp_bytes = std::max(ta, std::max(tb, tc));
      VSX_HIP_AS(WHO, B.temp.alloc(ctx, temp_bytes));
      VsxOtutabAdds A {};
      A.nq = nq; A.nu = nu; A.n_otus = n_otus; A.q_target = B.qtarget.p; A.q_ab = in.q_ab ? B.qab.p : nullptr; A.q_sample = B.q_sample.p;
      A.unmatched = B.unmatched.p; A.t_otu = B.t_otu.p; A.t_tax_len = B.t_tax_len.p;
      VSX_HIP_AS(WHO, vsx_launch_otutab_keys(A, B.keys_in.p, B.vals_in.p, st));
      VSX_HIP_AS(WHO, vsx_launch_otutab_sort(B.temp.p, &temp_bytes, B.keys_in.p, B.keys_out.p, B.vals_in.p, B.vals_out.p, ne, 32 + bits_for(n_otus), st));
      VSX_HIP_AS(WHO, vsx_launch_otutab_gather(A, B.keys_out.p, B.vals_out.p, B.count.p, B.otu.p, B.taxseq.p, st));
      VSX_HIP_AS(WHO, vsx_launch_otutab_reduce_cells(B.temp.p, &temp_bytes, B.keys_out.p, B.count.p, ne, B.ukeys.p, B.usum.p, B.n_unique.p, st));
      VSX_HIP_AS(WHO, vsx_launch_otutab_reduce_tax(B.temp.p, &temp_bytes, B.otu.p, B.taxseq.p, ne, B.uotu.p, B.umax.p, B.n_unique.p + 1, st));
      uint32_t nun[2] = { 0, 0 };
      VSX_HIP_AS(WHO, hipMemcpyAsync(nun, B.n_unique.p, sizeof nun, hipMemcpyDeviceToHost, st));
      VSX_HIP_AS(WHO, hipStreamSynchronize(st));
      if (nun[0] > ne || nun[1] > ne) return fail(VSX_EHIP, "%s: more cells than adds", WHO);
      VSX_HIP_AS(WHO, download(ukeys, B.ukeys.p, nun[0], st));
      VSX_HIP_AS(WHO, download(usum, B.usum.p, nun[0], st));
      VSX_HIP_AS(WHO, download(uotu, B.uotu.p, nun[1], st));
      VSX_HIP_AS(WHO, download(umax, B.umax.p, nun[1], st));
    }
  std::vector<uint64_t> tax_off;
  std::vector<uint32_t> tax_len;
  VSX_HIP_AS(WHO, download(M.q_sample, B.q_sample.p, nq, st));
  VSX_HIP_AS(WHO, download(M.t_otu, B.t_otu.p, nt, st));
  VSX_HIP_AS(WHO, download(tax_off, B.t_tax_off.p, nt, st));
  VSX_HIP_AS(WHO, download(tax_len, B.t_tax_len.p, nt, st));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  // what came back is checked before it is used as an index
  for (uint32_t k = 0; k < nq; ++k) if (M.q_sample[k] >= M.samples.size()) return fail(VSX_EHIP, "%s: a query has no sample rank", WHO);
  for (uint32_t t = 0; t < nt; ++t)
    if (takes[t] ? M.t_otu[t] >= n_otus : M.t_otu[t] != NONE) return fail(VSX_EHIP, "%s: a target's OTU rank is out of range", WHO);
  for (size_t c = 0; c < ukeys.size(); ++c)
    {
      const uint64_t otu = ukeys[c] >> 32, sample = ukeys[c] & 0xFFFFFFFFull;
      if (c && ukeys[c] <= ukeys[c - 1]) return fail(VSX_EHIP, "%s: the cells do not ascend", WHO);
      if (sample == VSX_OTUTAB_NO) continue;                    // no cell: abundance 0, no hit, the unmatched pass
      if (otu >= n_otus || sample >= M.samples.size()) return fail(VSX_EHIP, "%s: a cell is out of range", WHO);
      M.cell_key.push_back(ukeys[c]); M.cell_sum.push_back(usum[c]);
    }
  M.tax.assign(n_otus, Span { 0, NONE });
  for (size_t c = 0; c < uotu.size(); ++c)
    {
      if (uotu[c] >= n_otus || umax[c] == 0) continue;          // the run of the queries without a hit; an OTU nobody gave a taxonomy
      const uint64_t e = umax[c] - 1;
      if (e >= ne) return fail(VSX_EHIP, "%s: a taxonomy names an add that is not there", WHO);
      const uint32_t t = e < nq ? in.q_target[e] : unmatched[e - nq];
      if (t >= nt || tax_len[t] == NONE || tax_off[t] > T.bytes || tax_len[t] > T.bytes - tax_off[t])
        return fail(VSX_EHIP, "%s: a taxonomy span lies outside the blob", WHO);
      M.tax[uotu[c]] = Span { tax_off[t], tax_len[t] };
    }
  g_stats.seconds_accumulate += now_s() - t0;
  return VSX_OK;
}

int device_mid(vsx_ctx * ctx, const Input & in, Mid & M)
{
  VSX_HIP_AS(WHO, hipSetDevice(vsx_internal_device(ctx)));
  hipStream_t st = vsx_internal_stream(ctx);
  DeviceBufs B;
  const int rc = device_mid_run(ctx, st, in, B, M);
  (void) hipStreamSynchronize(st);                             // nothing of this call runs on once its blocks go back to the pool
  return rc;
}

// ---- the caller's output -----------------------------------------------------------------------------------------------------------
void release(vsx_otutab_result * out)
{
  std::free(out->sample_blob); std::free(out->sample_off); std::free(out->sample_len);
  std::free(out->otu_blob); std::free(out->otu_off); std::free(out->otu_len);
  std::free(out->tax_blob); std::free(out->tax_off); std::free(out->tax_len);
  std::free(out->nz_otu); std::free(out->nz_sample); std::free(out->nz_count); std::free(out->q_sample); std::free(out->t_otu);
  std::memset(out, 0, sizeof *out);
}


// the spans' bytes one after the other; a span of length NONE takes none
bool pack(const char * blob, const std::vector<Span> & spans, char *& out_blob, uint64_t & out_bytes, uint64_t *& out_off, uint32_t *& out_len)
{
  uint64_t total = 0;
  for (const Span & s : spans) if (s.len != NONE) total += s.len;
  out_blob = array_of<char>(total); out_off = array_of<uint64_t>(spans.size()); out_len = array_of<uint32_t>(spans.size());
  if (!out_blob || !out_off || !out_len) return false;
  uint64_t at = 0;
  for (size_t r = 0; r < spans.size(); ++r)
    {
      out_off[r] = at; out_len[r] = spans[r].len;
      if (spans[r].len != NONE && spans[r].len) { std::memcpy(out_blob + at, blob + spans[r].off, spans[r].len); at += spans[r].len; }
    }
  out_bytes = total;
  return true;
}

int finish(const Input & in, const Mid & M, vsx_otutab_result & out)
{
  out.n_queries = in.nq(); out.n_targets = in.nt();
  out.n_samples = M.samples.size(); out.n_otus = M.otus.size();
  for (const Span & s : M.tax) if (s.len != NONE) out.has_tax = 1;
  const uint64_t nc = M.cell_key.size();
  out.n_cells = nc;
  out.nz_otu = array_of<uint32_t>(nc); out.nz_sample = array_of<uint32_t>(nc); out.nz_count = array_of<uint64_t>(nc);
  out.q_sample = array_of<uint32_t>(in.nq()); out.t_otu = array_of<uint32_t>(in.nt());
  if (!pack(in.Q->blob, M.samples, out.sample_blob, out.sample_bytes, out.sample_off, out.sample_len) ||
      !pack(in.T->blob, M.otus, out.otu_blob, out.otu_bytes, out.otu_off, out.otu_len) ||
      !pack(in.T->blob, M.tax, out.tax_blob, out.tax_bytes, out.tax_off, out.tax_len) ||
      !out.nz_otu || !out.nz_sample || !out.nz_count || !out.q_sample || !out.t_otu) return fail(VSX_ENOMEM, "%s: out of memory", WHO);
  for (uint64_t c = 0; c < nc; ++c)
    {
      out.nz_otu[c] = (uint32_t) (M.cell_key[c] >> 32); out.nz_sample[c] = (uint32_t) M.cell_key[c]; out.nz_count[c] = M.cell_sum[c];
    }
  if (in.nq()) std::memcpy(out.q_sample, M.q_sample.data(), in.nq() * sizeof(uint32_t));
  if (in.nt()) std::memcpy(out.t_otu, M.t_otu.data(), in.nt() * sizeof(uint32_t));
  return VSX_OK;
}

// the refusals of both routes
int check(const vsx_otutab_opts * opts, const vsx_labels * Q, const uint32_t * q_target, const vsx_labels * T, vsx_otutab_result * out)
{
  if (!opts || !out || !Q || !T) return fail(VSX_EINVAL, "%s: null argument", WHO);
  if ((Q->n && (!Q->offsets || !Q->lengths || !q_target)) || (T->n && (!T->offsets || !T->lengths)) || (Q->bytes && !Q->blob) || (T->bytes && !T->blob))
    return fail(VSX_EINVAL, "%s: null argument", WHO);
  if (opts->threads < 0) return fail(VSX_EINVAL, "%s: threads cannot be negative", WHO);
  for (const vsx_labels * S : { Q, T })
    for (uint64_t k = 0; k < S->n; ++k)
      if (S->offsets[k] > S->bytes || S->lengths[k] > S->bytes - S->offsets[k])
        return fail(VSX_EINVAL, "%s: %s label %llu lies outside its blob", WHO, S == Q ? "query" : "target", (unsigned long long) k);
  for (uint64_t k = 0; k < Q->n; ++k)
    if (q_target[k] != NONE && q_target[k] >= T->n)
      return fail(VSX_EINVAL, "%s: query %llu names target %u of %llu", WHO, (unsigned long long) k, q_target[k], (unsigned long long) T->n);
  return VSX_OK;
}

enum Route { ROUTE_CALLER, ROUTE_HOST_ONLY };

int run(vsx_ctx * ctx, Route route, const vsx_otutab_opts * opts, const vsx_labels * Q, const uint64_t * q_ab, const uint32_t * q_target,
        const vsx_labels * T, const uint8_t * t_matched, vsx_otutab_result * out)
{
  g_stats = vsx_otutab_stats {};
  const double t_begin = now_s();
  double t0 = t_begin;
  int rc = check(opts, Q, q_target, T, out);
  if (rc != VSX_OK) return rc;
  std::memset(out, 0, sizeof *out);
  Input in { Q, T, q_ab, q_target, t_matched, opts->threads > 0 ? opts->threads : std::max(1, std::min(vsxp::usable_cpus(), HOST_THREADS)) };
  g_stats.seconds_stage += now_s() - t0;

  bool host_all = true;
  if (route == ROUTE_HOST_ONLY) {}
  else
    {
      // testing aid: a lower limit of the device route
      const uint64_t device_labels = std::min<uint64_t>(LABEL_LIMIT, vsxp::env_u64("VSX_OTUTAB_DEVICE_LABELS", LABEL_LIMIT, true));
      if (!ctx) g_stats.host_no_context = 1;
      else if (vsxp::env_is_host("VSX_OTUTAB")) g_stats.host_environment = 1;
      else if (Q->n > device_labels || T->n > device_labels || Q->n + T->n > device_labels) g_stats.host_label_count = 1;
      else host_all = false;
      if (!host_all)
        {
          bool fits = false;                                                                   // (the testing aid: what the call is taken to need)
          if ((rc = vsxp::device_fits(ctx, WHO, device_bytes(in), "VSX_OTUTAB_PRETEND_BYTES", &fits)) != VSX_OK) return rc;
          if (!fits) { host_all = true; g_stats.host_memory = 1; }
        }
    }
  Mid M;
  rc = host_all ? host_mid(in, M) : device_mid(ctx, in, M);
  if (rc == VSX_OK)
    {
      t0 = now_s();
      rc = finish(in, M, *out);
      g_stats.seconds_output += now_s() - t0;
    }
  if (rc != VSX_OK) { release(out); return rc; }
  g_stats.seconds_total = now_s() - t_begin;
  return VSX_OK;
}

}  // namespace

extern "C" {

void vsx_otutab_opts_default(vsx_otutab_opts * o) { std::memset(o, 0, sizeof *o); }

void vsx_otutab_last_stats(vsx_otutab_stats * out) { if (out) *out = g_stats; }

void vsx_otutab_result_free(vsx_otutab_result * out) { if (out) release(out); }

int vsx_otutab(vsx_ctx * ctx, const vsx_otutab_opts * opts, const vsx_labels * queries, const uint64_t * q_abundance, const uint32_t * q_target,
               const vsx_labels * targets, const uint8_t * t_matched, vsx_otutab_result * out)
{
  return run(ctx, ROUTE_CALLER, opts, queries, q_abundance, q_target, targets, t_matched, out);
}

int vsx_internal_otutab_host(const vsx_otutab_opts * opts, const vsx_labels * queries, const uint64_t * q_abundance, const uint32_t * q_target,
                             const vsx_labels * targets, const uint8_t * t_matched, vsx_otutab_result * out)
{
  return run(nullptr, ROUTE_HOST_ONLY, opts, queries, q_abundance, q_target, targets, t_matched, out);
}

}  // extern "C"
