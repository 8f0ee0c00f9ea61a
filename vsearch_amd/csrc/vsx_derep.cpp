// vsx_derep.cpp -- full-length dereplication (include/vsx_derep.h: vsx_derep), the host side of vsx_derep.hip.
//
// Restated from the reference (src/, v2.31.0): core/derep.cpp: derep() -- the discards, the find-or-insert loop over both
// strands, the size-weighted quality merge, derep_compare_full's order, find_median_size, count_selected.
//
// Both routes end in the same intermediate form (Groups): the clusters ascending by representative, every cluster's members in
// input order, a strand per member, a size per cluster and -- with want_quality -- a merged quality string per cluster.  finish()
// turns it into the caller's output: the cluster order (size, label, index), the CSR member list, the counts of the log lines.
//
//   device   the kept reads are staged window by window (the slots and items of the exact search's plan, vsx_exact_internal.h),
//            hashed on both strands by vsx_launch_exact_hash into one word buffer that stays on the device, then keyed, grouped,
//            accounted and sorted by the kernels of vsx_derep.hip.  The quality blob is uploaded as it stands.
//   host     host_groups below is the reference's loop over a std::unordered_map of code strings, written from the specification
//            and not from the kernels; it evaluates trunc(-10 log10 p) directly.  VSX_DEREP=host, a missing context, more than
//            UINT32_MAX - 1 kept reads or buffers that do not fit the device send the whole call through it.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <unordered_map>

#include "../../include/vsx_derep.h"
#include "vsx_derep_internal.h"
#include "vsx_private.h"

#pragma clang fp contract(off)

using vsxp::array_of;
using vsxp::fail;
using vsxp::now_s;
using vsxp::upload;
using vsxp::DevBuf;
using vsxp::PinnedBuf;
using vsxp::ensure_pinned;
using vsxp::map4;

namespace {

constexpr const char * WHO = "vsx_derep";
constexpr uint64_t WINDOW_READS = 65536;
constexpr uint64_t SIZE_LIMIT = 1ull << 32;                 // the reference's 32-bit cluster size: not restated, refused

thread_local vsx_derep_stats g_stats {};

// ---- the quality tables ------------------------------------------------------------------------------------------------------
// convert_quality_symbol_to_probability, by symbol
void build_prob(int64_t ascii, double * prob)
{
  for (int sym = 0; sym < 128; ++sym)
    {
      const int q = sym - (int) ascii;
      prob[sym] = q < 2 ? 0.75 : std::pow(10.0, -q / 10.0);
    }
}

inline int64_t quality_value(double p) { return (int64_t) std::trunc(-10.0 * std::log10(p)); }

// T[v]: the largest double p with trunc(-10 log10 p) >= v, by bisection over the bit patterns of the positive doubles with the
// host's own log10 (which is monotone around every threshold: tests/test_derep_host.py checks the table against math.log10)
void build_thresholds(double * T)
{
  for (int v = 0; v < VSX_DEREP_THRESHOLDS; ++v)
    {
      double lo_d = DBL_MIN, hi_d = 2.0;                      // true at lo, false at hi
      uint64_t lo, hi;
      std::memcpy(&lo, &lo_d, 8); std::memcpy(&hi, &hi_d, 8);
      while (hi - lo > 1)
        {
          const uint64_t mid = lo + (hi - lo) / 2;
          double p;
          std::memcpy(&p, &mid, 8);
          if (quality_value(p) >= v) lo = mid; else hi = mid;
        }
      std::memcpy(&T[v], &lo, 8);
    }
}

// convert_probability_to_quality_symbol
inline int quality_symbol(double p, const vsx_derep_opts & o)
{
  int64_t v = quality_value(p);
  v = std::min(v, o.qmaxout);
  v = std::max(v, o.qminout);
  return (int) (v + o.asciiout);
}

// ---- the input as both routes read it ----------------------------------------------------------------------------------------
struct Input {
  const vsx_derep_opts * o;
  const vsx_fastx_reads * reads;
  const char * label_blob;
  const uint64_t * label_off;
  std::vector<uint64_t> kept;        // input indices of the reads within the length limits
  const char * seq(uint64_t k) const { return reads->seq + reads->off[kept[k]]; }
  const char * qual(uint64_t k) const { return reads->qual + reads->off[kept[k]]; }
  uint32_t len(uint64_t k) const { return reads->len[kept[k]]; }
  uint64_t abundance(uint64_t k) const { return reads->abundance ? reads->abundance[kept[k]] : 1; }
  const char * label(uint64_t k) const { return label_blob + label_off[kept[k]]; }
  uint64_t label_len(uint64_t k) const { return label_off[kept[k] + 1] - label_off[kept[k]]; }
};

// clusters ascending by representative; members are indices into Input::kept
struct Groups {
  std::vector<uint64_t> cstart;      // clusters + 1
  std::vector<uint64_t> member;      // kept: a cluster's members in input order (the representative is the first)
  std::vector<uint8_t> strand;       // kept: beside member
  std::vector<uint64_t> size;        // clusters
  std::vector<uint64_t> qoff;        // clusters + 1 (want_quality)
  std::vector<char> qual;
};

// ---- the host restatement ------------------------------------------------------------------------------------------------------
inline uint8_t complement4(uint8_t c)
{
  if (c == 0) return 15;                                      // a symbol outside the alphabet complements to 'N'
  return (uint8_t) (((c & 1) << 3) | ((c & 2) << 1) | ((c & 4) >> 1) | ((c & 8) >> 3));
}

void host_groups(const Input & in, Groups & G)
{
  const vsx_derep_opts & o = *in.o;
  const uint64_t K = in.kept.size();
  std::unordered_map<std::string, uint64_t> table;
  std::vector<uint64_t> cluster_of(K), count;
  std::vector<uint8_t> minus(K, 0);
  std::vector<uint64_t> rep;
  std::string plus, rc;
  auto with_label = [&](std::string & key, uint64_t k) {
    if (!o.by_label) return;
    key.push_back((char) 0xFF);
    key.append(in.label(k), in.label_len(k));
  };
  for (uint64_t k = 0; k < K; ++k)
    {
      const uint32_t L = in.len(k);
      const char * s = in.seq(k);
      plus.resize(L);
      for (uint32_t i = 0; i < L; ++i) plus[i] = (char) map4((unsigned char) s[i]);
      rc.clear();
      if (o.strand_both)
        {
          rc.resize(L);
          for (uint32_t i = 0; i < L; ++i) rc[i] = (char) complement4((uint8_t) plus[L - 1 - i]);
          with_label(rc, k);
        }
      with_label(plus, k);
      auto hit = table.find(plus);
      if (hit == table.end() && o.strand_both)
        {
          hit = table.find(rc);
          if (hit != table.end()) minus[k] = 1;
        }
      const uint64_t s2 = in.abundance(k);
      if (hit == table.end())
        {
          const uint64_t c = rep.size();
          table.emplace(plus, c);
          rep.push_back(k); count.push_back(1); G.size.push_back(s2);
          cluster_of[k] = c;
          if (o.want_quality)
            {
              G.qoff.push_back(G.qual.size());
              G.qual.insert(G.qual.end(), in.qual(k), in.qual(k) + L);
            }
          continue;
        }
      const uint64_t c = hit->second;
      cluster_of[k] = c;
      const uint64_t s1 = G.size[c], s3 = s1 + s2;
      if (o.want_quality)
        {
          char * q = G.qual.data() + G.qoff[c];
          const char * q2 = in.qual(k);                        // a minus-strand member's string is applied unreversed
          for (uint32_t i = 0; i < L; ++i)
            {
              const int v1 = (int) q[i] - (int) o.ascii, v2 = (int) q2[i] - (int) o.ascii;
              const double p1 = v1 < 2 ? 0.75 : std::pow(10.0, -v1 / 10.0);
              const double p2 = v2 < 2 ? 0.75 : std::pow(10.0, -v2 / 10.0);
              const double p3 = o.qout_max ? std::min(p1, p2) : ((p1 * (double) (int64_t) s1) + (p2 * (double) (int64_t) s2)) / (double) (int64_t) s3;
              q[i] = (char) quality_symbol(p3, o);
            }
        }
      G.size[c] = s3;
      ++count[c];
    }
  const uint64_t C = rep.size();
  if (o.want_quality) G.qoff.push_back(G.qual.size());
  G.cstart.assign(C + 1, 0);
  for (uint64_t c = 0; c < C; ++c) G.cstart[c + 1] = G.cstart[c] + count[c];
  G.member.resize(K); G.strand.resize(K);
  std::vector<uint64_t> at(G.cstart.begin(), G.cstart.end() - 1);
  for (uint64_t k = 0; k < K; ++k) { const uint64_t p = at[cluster_of[k]]++; G.member[p] = k; G.strand[p] = minus[k]; }
  g_stats.reads_host = K;
}

// ---- the device route ------------------------------------------------------------------------------------------------------------
struct Events {
  hipEvent_t a = nullptr, b = nullptr, c = nullptr;
  ~Events() { for (hipEvent_t e : { a, b, c }) if (e) (void) hipEventDestroy(e); }
};

// bytes the device route keeps resident for K reads of W code words (both strands counted in W), the quality blobs included
uint64_t device_bytes(uint64_t K, uint64_t W, uint64_t T, uint64_t qual_bytes)
{
  return W * 8 + K * 160 + T * 4 + 3 * qual_bytes + ((uint64_t) 64 << 20);
}

int device_groups(vsx_ctx * ctx, const Input & in, uint64_t W, Groups & G)
{
  const vsx_derep_opts & o = *in.o;
  const uint64_t K = in.kept.size();
  const bool both = o.strand_both != 0;
  VSX_HIP_AS(WHO, hipSetDevice(vsx_internal_device(ctx)));
  hipStream_t st = vsx_internal_stream(ctx);
  Events ev;
  for (hipEvent_t * e : { &ev.a, &ev.b, &ev.c }) VSX_HIP_AS(WHO, hipEventCreate(e));
  const uint64_t hash_mask = vsxe::hash_mask_from_env("VSX_DEREP_HASH_BITS");
  const uint64_t window = o.window > 0 ? (uint64_t) o.window : WINDOW_READS;

  // ---- stage and hash, window by window: the words and hashes of every strand stay on the device
  DevBuf<uint64_t> d_words, d_hash_p, d_hash_m;
  DevBuf<uint8_t> d_text;
  DevBuf<VsxExactItem> d_items;
  PinnedBuf<char> h_text;
  PinnedBuf<VsxExactItem> h_items;
  VSX_HIP_AS(WHO, d_words.alloc(W + 2));
  VSX_HIP_AS(WHO, d_hash_p.alloc(K));
  if (both) VSX_HIP_AS(WHO, d_hash_m.alloc(K));
  std::vector<uint64_t> woff_p(K), woff_m(both ? K : 0);
  std::vector<uint32_t> len(K);
  uint64_t wbase = 0;
  for (uint64_t w0 = 0; w0 < K; w0 += window)
    {
      const double t0 = now_s();
      const uint64_t wn = std::min(window, K - w0), ns = both ? 2 * wn : wn;
      VSX_HIP_AS(WHO, ensure_pinned(h_items, ns));
      const vsxe::Plan P = vsxe::plan_items(wn, [&](uint64_t k) { return in.len(w0 + k); }, both, false, h_items.p);
      VSX_HIP_AS(WHO, ensure_pinned(h_text, P.text_bytes));
      for (uint64_t k = 0; k < wn; ++k)
        {
          VsxExactItem & it = h_items.p[k];
          it.woff += wbase;
          woff_p[w0 + k] = it.woff; len[w0 + k] = it.len;
          if (both) { h_items.p[wn + k].woff += wbase; woff_m[w0 + k] = h_items.p[wn + k].woff; }
          if (it.len) std::memcpy(h_text.p + it.off, in.seq(w0 + k), it.len);
        }
      wbase += P.words;
      g_stats.seconds_stage += now_s() - t0;
      VSX_HIP_AS(WHO, d_text.ensure(P.text_bytes));
      VSX_HIP_AS(WHO, d_items.ensure(ns));
      VSX_HIP_AS(WHO, hipEventRecord(ev.a, st));
      VSX_HIP_AS(WHO, hipMemcpyAsync(d_text.p, h_text.p, P.text_bytes, hipMemcpyHostToDevice, st));
      VSX_HIP_AS(WHO, hipMemcpyAsync(d_items.p, h_items.p, ns * sizeof(VsxExactItem), hipMemcpyHostToDevice, st));
      VSX_HIP_AS(WHO, hipEventRecord(ev.b, st));
      VSX_HIP_AS(WHO, vsx_launch_exact_hash(d_items.p, (uint32_t) wn, d_text.p, hash_mask, d_words.p, d_hash_p.p + w0, st));
      if (both) VSX_HIP_AS(WHO, vsx_launch_exact_hash(d_items.p + wn, (uint32_t) wn, d_text.p, hash_mask, d_words.p, d_hash_m.p + w0, st));
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
  d_text.release(); d_items.release();

  // ---- the per-read arrays
  double t0 = now_s();
  std::vector<uint64_t> ab;
  if (in.reads->abundance) { ab.resize(K); for (uint64_t k = 0; k < K; ++k) ab[k] = in.abundance(k); }
  std::vector<uint32_t> label;
  if (o.by_label)
    {
      // labels interned to integer ids: the id is part of the key
      std::unordered_map<std::string, uint32_t> ids;
      label.resize(K);
      for (uint64_t k = 0; k < K; ++k)
        label[k] = ids.emplace(std::string(in.label(k), in.label_len(k)), (uint32_t) ids.size()).first->second;
    }
  g_stats.seconds_stage += now_s() - t0;
  t0 = now_s();
  DevBuf<uint32_t> d_len, d_label, d_table, d_root, d_rep, d_count;
  DevBuf<uint64_t> d_woff_p, d_woff_m, d_ab, d_khash, d_kwoff, d_size, d_keys_a, d_keys_b;
  DevBuf<uint8_t> d_flag, d_temp;
  DevBuf<VsxDerepCounters> d_counters;
  VSX_HIP_AS(WHO, upload(d_len, len.data(), K, st));
  VSX_HIP_AS(WHO, upload(d_woff_p, woff_p.data(), K, st));
  if (both) VSX_HIP_AS(WHO, upload(d_woff_m, woff_m.data(), K, st));
  if (!ab.empty()) VSX_HIP_AS(WHO, upload(d_ab, ab.data(), K, st));
  if (o.by_label) VSX_HIP_AS(WHO, upload(d_label, label.data(), K, st));
  const uint64_t table_size = vsxe::table_size_for(K);
  VSX_HIP_AS(WHO, d_table.alloc(table_size));
  VSX_HIP_AS(WHO, d_root.alloc(K)); VSX_HIP_AS(WHO, d_rep.alloc(K)); VSX_HIP_AS(WHO, d_count.alloc(K)); VSX_HIP_AS(WHO, d_size.alloc(K));
  VSX_HIP_AS(WHO, d_khash.alloc(K)); VSX_HIP_AS(WHO, d_kwoff.alloc(K)); VSX_HIP_AS(WHO, d_flag.alloc(K));
  VSX_HIP_AS(WHO, d_keys_a.alloc(K)); VSX_HIP_AS(WHO, d_keys_b.alloc(K));
  VSX_HIP_AS(WHO, d_counters.alloc(1));
  VSX_HIP_AS(WHO, hipMemsetAsync(d_table.p, 0xFF, table_size * sizeof(uint32_t), st));
  VSX_HIP_AS(WHO, hipMemsetAsync(d_rep.p, 0xFF, K * sizeof(uint32_t), st));
  VSX_HIP_AS(WHO, hipMemsetAsync(d_count.p, 0, K * sizeof(uint32_t), st));
  VSX_HIP_AS(WHO, hipMemsetAsync(d_size.p, 0, K * sizeof(uint64_t), st));
  VSX_HIP_AS(WHO, hipMemsetAsync(d_counters.p, 0, sizeof(VsxDerepCounters), st));
  VsxDerepReads R {};
  R.n = (uint32_t) K; R.len = d_len.p; R.hash_plus = d_hash_p.p; R.hash_minus = both ? d_hash_m.p : nullptr;
  R.woff_plus = d_woff_p.p; R.woff_minus = both ? d_woff_m.p : nullptr; R.label = o.by_label ? d_label.p : nullptr; R.words = d_words.p;
  const uint64_t * const d_abundance = ab.empty() ? nullptr : d_ab.p;

  // ---- key, group
  VSX_HIP_AS(WHO, vsx_launch_derep_key(R, hash_mask, d_khash.p, d_kwoff.p, d_flag.p, st));
  VSX_HIP_AS(WHO, vsx_launch_derep_group(R, d_khash.p, d_kwoff.p, d_table.p, table_size, d_root.p, d_counters.p, st));
  VsxDerepCounters counters {};
  VSX_HIP_AS(WHO, hipMemcpyAsync(&counters, d_counters.p, sizeof counters, hipMemcpyDeviceToHost, st));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  g_stats.slots_visited = counters.slots_visited;
  g_stats.candidates_compared = counters.candidates_compared;
  g_stats.seconds_group += now_s() - t0;

  // ---- account, member list
  t0 = now_s();
  size_t temp_bytes = 0;
  VSX_HIP_AS(WHO, vsx_launch_derep_members((uint32_t) K, d_root.p, d_rep.p, d_keys_a.p, d_keys_b.p, nullptr, &temp_bytes, st));
  VSX_HIP_AS(WHO, d_temp.alloc(temp_bytes));
  VSX_HIP_AS(WHO, vsx_launch_derep_account((uint32_t) K, d_root.p, d_abundance, d_rep.p, d_size.p, d_count.p, st));
  VSX_HIP_AS(WHO, vsx_launch_derep_members((uint32_t) K, d_root.p, d_rep.p, d_keys_a.p, d_keys_b.p, d_temp.p, &temp_bytes, st));
  std::vector<uint64_t> keys(K), csize(K);
  std::vector<uint32_t> root(K), ccount(K);
  std::vector<uint8_t> flag(K);
  VSX_HIP_AS(WHO, hipMemcpyAsync(keys.data(), d_keys_b.p, K * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  VSX_HIP_AS(WHO, hipMemcpyAsync(csize.data(), d_size.p, K * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  VSX_HIP_AS(WHO, hipMemcpyAsync(root.data(), d_root.p, K * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  VSX_HIP_AS(WHO, hipMemcpyAsync(ccount.data(), d_count.p, K * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  VSX_HIP_AS(WHO, hipMemcpyAsync(flag.data(), d_flag.p, K, hipMemcpyDeviceToHost, st));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  G.member.resize(K); G.strand.resize(K);
  G.cstart.clear();
  for (uint64_t p = 0; p < K; ++p)
    {
      const uint64_t rep = keys[p] >> 32, k = keys[p] & 0xFFFFFFFFull;
      if (rep >= K || k >= K || root[k] >= K) return fail(VSX_EHIP, "%s: the member list names a read that is not there", WHO);
      if (p == 0 || rep != keys[p - 1] >> 32)
        {
          if (k != rep) return fail(VSX_EHIP, "%s: a cluster does not begin with its representative", WHO);
          G.cstart.push_back(p);
          G.size.push_back(csize[root[rep]]);
        }
      G.member[p] = k;
      G.strand[p] = flag[k] ^ flag[rep];
    }
  G.cstart.push_back(K);
  const uint64_t C = G.cstart.size() - 1;
  for (uint64_t c = 0; c < C; ++c)
    if (ccount[root[G.member[G.cstart[c]]]] != G.cstart[c + 1] - G.cstart[c]) return fail(VSX_EHIP, "%s: a cluster's count differs from its member list", WHO);
  g_stats.seconds_account += now_s() - t0;
  if (!o.want_quality) return VSX_OK;

  // ---- quality: the clusters of two or more members on the device, a single member's string is its own
  t0 = now_s();
  d_table.release(); d_keys_a.release(); d_temp.release(); d_khash.release(); d_kwoff.release(); d_words.release();
  std::vector<VsxDerepQTask> tasks;
  std::vector<uint64_t> merged_off(C, 0);
  uint64_t merged_bytes = 0;
  G.qoff.assign(C + 1, 0);
  for (uint64_t c = 0; c < C; ++c)
    {
      const uint64_t members = G.cstart[c + 1] - G.cstart[c];
      const uint32_t L = len[G.member[G.cstart[c]]];
      G.qoff[c + 1] = G.qoff[c] + L;
      if (members < 2) continue;
      merged_off[c] = merged_bytes;
      for (uint32_t b = 0; (uint64_t) b * VSX_DEREP_QBLOCK < L; ++b)
        tasks.push_back(VsxDerepQTask { G.cstart[c], merged_bytes, (uint32_t) members, L, b, 0u });
      merged_bytes += L;
    }
  G.qual.resize(G.qoff[C]);
  std::vector<char> merged(merged_bytes);
  if (!tasks.empty())
    {
      double prob[128], thr[VSX_DEREP_THRESHOLDS];
      build_prob(o.ascii, prob);
      build_thresholds(thr);
      std::vector<uint64_t> qoff(K);
      for (uint64_t k = 0; k < K; ++k) qoff[k] = in.reads->off[in.kept[k]];
      DevBuf<double> d_prob, d_thr;
      DevBuf<uint8_t> d_qual, d_out;
      DevBuf<uint64_t> d_qoff;
      DevBuf<VsxDerepQTask> d_tasks;
      VSX_HIP_AS(WHO, upload(d_prob, prob, 128, st));
      VSX_HIP_AS(WHO, upload(d_thr, thr, VSX_DEREP_THRESHOLDS, st));
      VSX_HIP_AS(WHO, upload(d_qual, reinterpret_cast<const uint8_t *>(in.reads->qual), in.reads->bytes, st));
      VSX_HIP_AS(WHO, upload(d_qoff, qoff.data(), K, st));
      VSX_HIP_AS(WHO, upload(d_tasks, tasks.data(), tasks.size(), st));
      VSX_HIP_AS(WHO, d_out.alloc(merged_bytes));
      VsxDerepQParams QP {};
      QP.prob = d_prob.p; QP.threshold = reinterpret_cast<const uint64_t *>(d_thr.p);
      QP.qout_max = o.qout_max; QP.asciiout = (int32_t) o.asciiout; QP.qminout = (int32_t) o.qminout; QP.qmaxout = (int32_t) o.qmaxout;
      const uint64_t chunk = 1ull << 30;
      for (uint64_t t = 0; t < tasks.size(); t += chunk)
        VSX_HIP_AS(WHO, vsx_launch_derep_quality(d_tasks.p + t, (uint32_t) std::min<uint64_t>(chunk, tasks.size() - t), d_keys_b.p, d_qual.p,
                                                 d_qoff.p, d_abundance, QP, d_out.p, st));
      VSX_HIP_AS(WHO, hipMemcpyAsync(merged.data(), d_out.p, merged_bytes, hipMemcpyDeviceToHost, st));
      VSX_HIP_AS(WHO, hipStreamSynchronize(st));
    }
  for (uint64_t c = 0; c < C; ++c)
    {
      const uint64_t L = G.qoff[c + 1] - G.qoff[c];
      if (!L) continue;
      const char * src = G.cstart[c + 1] - G.cstart[c] < 2 ? in.qual(G.member[G.cstart[c]]) : merged.data() + merged_off[c];
      std::memcpy(G.qual.data() + G.qoff[c], src, L);
    }
  g_stats.seconds_quality += now_s() - t0;
  return VSX_OK;
}

// ---- the caller's output -----------------------------------------------------------------------------------------------------------
void release(vsx_derep_out * out)
{
  std::free(out->rep); std::free(out->size); std::free(out->count); std::free(out->member_start); std::free(out->member);
  std::free(out->strand); std::free(out->qual_off); std::free(out->qual_blob);
  std::memset(out, 0, sizeof *out);
}


int finish(const Input & in, const Groups & G, vsx_derep_out & out)
{
  const vsx_derep_opts & o = *in.o;
  const uint64_t K = in.kept.size(), C = G.size.size();
  // derep_compare_full: size descending, strcmp of the representatives' labels, representative index
  std::vector<uint64_t> order(C);
  std::iota(order.begin(), order.end(), (uint64_t) 0);
  auto rep_of = [&](uint64_t c) { return G.member[G.cstart[c]]; };
  std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
    if (G.size[a] != G.size[b]) return G.size[a] > G.size[b];
    const uint64_t ka = rep_of(a), kb = rep_of(b), la = in.label_len(ka), lb = in.label_len(kb);
    const int cmp = std::memcmp(in.label(ka), in.label(kb), std::min(la, lb));
    if (cmp != 0) return cmp < 0;
    if (la != lb) return la < lb;
    return ka < kb;
  });
  out.n_clusters = C;
  out.rep = array_of<uint64_t>(C); out.size = array_of<uint64_t>(C); out.count = array_of<uint64_t>(C);
  out.member_start = array_of<uint64_t>(C + 1); out.member = array_of<uint64_t>(K); out.strand = array_of<uint8_t>(K);
  if (o.want_quality) { out.qual_off = array_of<uint64_t>(C + 1); out.qual_blob = array_of<char>(G.qual.size()); out.qual_bytes = G.qual.size(); }
  if (!out.rep || !out.size || !out.count || !out.member_start || !out.member || !out.strand || (o.want_quality && (!out.qual_off || !out.qual_blob)))
    return fail(VSX_ENOMEM, "%s: out of memory", WHO);
  uint64_t at = 0, qat = 0, in_range = 0;
  for (uint64_t i = 0; i < C; ++i)
    {
      const uint64_t c = order[i], members = G.cstart[c + 1] - G.cstart[c];
      out.rep[i] = in.kept[rep_of(c)]; out.size[i] = G.size[c]; out.count[i] = members;
      out.member_start[i] = at;
      for (uint64_t m = 0; m < members; ++m) { out.member[at + m] = in.kept[G.member[G.cstart[c] + m]]; out.strand[at + m] = G.strand[G.cstart[c] + m]; }
      at += members;
      if (o.want_quality)
        {
          const uint64_t L = G.qoff[c + 1] - G.qoff[c];
          out.qual_off[i] = qat;
          if (L) std::memcpy(out.qual_blob + qat, G.qual.data() + G.qoff[c], L);
          qat += L;
        }
      out.maxsize = std::max(out.maxsize, G.size[c]);
      if ((int64_t) G.size[c] >= o.minuniquesize && (int64_t) G.size[c] <= o.maxuniquesize) ++in_range;
    }
  out.member_start[C] = at;
  if (o.want_quality) out.qual_off[C] = qat;
  // count_selected, find_median_size
  out.selected = std::min<uint64_t>(in_range, o.topn < 0 ? 0 : (uint64_t) o.topn);
  if (C == 0) out.median = 0.0;
  else if (C % 2) out.median = (double) out.size[C / 2];
  else out.median = (double) out.size[C / 2] + (double) (out.size[C / 2 - 1] - out.size[C / 2]) * 0.5;
  return VSX_OK;
}

int check_options(const vsx_derep_opts & o)
{
  const char * bad = nullptr;
  if (o.window < 0) bad = "window cannot be negative";
  // quality symbols are table indices, and the merged symbols are read back as such
  else if (o.ascii < 0 || o.ascii > 127 || o.qminout > o.qmaxout || o.asciiout + o.qminout < 0 || o.asciiout + o.qmaxout > 127)
    bad = "the quality offset must lie within 0..127, and so must the output offset plus qminout / qmaxout";
  return bad ? fail(VSX_EINVAL, "%s: %s", WHO, bad) : VSX_OK;
}

}  // namespace

extern "C" {

void vsx_derep_opts_default(vsx_derep_opts * o)
{
  std::memset(o, 0, sizeof *o);
  o->minseqlength = 32; o->maxseqlength = 50000;
  o->minuniquesize = 1; o->maxuniquesize = INT64_MAX; o->topn = INT64_MAX;
  o->ascii = 33; o->asciiout = 33; o->qminout = 0; o->qmaxout = 41;
}

void vsx_derep_last_stats(vsx_derep_stats * out) { if (out) *out = g_stats; }

void vsx_derep_out_free(vsx_derep_out * out) { if (out) release(out); }

void vsx_internal_derep_thresholds(double * out129) { build_thresholds(out129); }

int vsx_derep(vsx_ctx * ctx, const vsx_derep_opts * opts, uint64_t n, const vsx_fastx_reads * reads, const char * label_blob,
              const uint64_t * label_off, vsx_derep_out * out)
{
  g_stats = vsx_derep_stats {};
  const double t_begin = now_s();
  if (!opts || !out || !reads || (n && (!reads->seq || !reads->off || !reads->len || !label_blob || !label_off)))
    return fail(VSX_EINVAL, "%s: null argument", WHO);
  std::memset(out, 0, sizeof *out);
  const vsx_derep_opts & o = *opts;
  const int rc_opts = check_options(o);
  if (rc_opts != VSX_OK) return rc_opts;
  if (o.want_quality && n && !reads->qual) return fail(VSX_EINVAL, "%s: want_quality needs the reads' quality strings", WHO);

  // ---- the discards, the counts of the first log line, the refusals
  Input in { opts, reads, label_blob, label_off, {} };
  out->n = n;
  uint64_t shortest = UINT64_MAX, W = 0;
  for (uint64_t k = 0; k < n; ++k)
    {
      if (reads->off[k] > reads->bytes || reads->len[k] > reads->bytes - reads->off[k]) return fail(VSX_EINVAL, "%s: a read exceeds its blob", WHO);
      if (label_off[k + 1] < label_off[k]) return fail(VSX_EINVAL, "%s: the label offsets decrease", WHO);
      const int64_t L = reads->len[k];
      if (L < o.minseqlength) { ++out->discarded_short; continue; }
      if (L > o.maxseqlength) { ++out->discarded_long; continue; }
      const uint64_t ab = reads->abundance ? reads->abundance[k] : 1;
      if (ab == 0) return fail(VSX_EINVAL, "%s: read %llu has abundance 0", WHO, (unsigned long long) k);
      if (ab >= SIZE_LIMIT || (out->sumsize += ab) >= SIZE_LIMIT)
        return fail(VSX_EINVAL, "%s: the abundances sum to 2^32 or more (the reference's 32-bit cluster size would wrap)", WHO);
      if (o.want_quality)
        {
          const unsigned char * q = reinterpret_cast<const unsigned char *>(reads->qual) + reads->off[k];
          for (int64_t i = 0; i < L; ++i)
            if (q[i] < 33 || q[i] > 126) return fail(VSX_EINVAL, "%s: read %llu has a quality symbol outside 33..126", WHO, (unsigned long long) k);
        }
      in.kept.push_back(k);
      out->nucleotides += (uint64_t) L;
      shortest = std::min<uint64_t>(shortest, (uint64_t) L);
      out->longest = std::max<uint64_t>(out->longest, (uint64_t) L);
      W += vsxe::words_of((uint32_t) L);
    }
  const uint64_t K = in.kept.size();
  out->kept = K;
  out->shortest = K ? shortest : 0;
  if (o.strand_both) W *= 2;

  // ---- the route
  bool host_all = vsxp::env_is_host("VSX_DEREP") || !ctx || K > (uint64_t) UINT32_MAX - 1;
  Groups G;
  int rc = VSX_OK;
  if (!host_all && K)
    {
      bool fits = false;
      rc = vsxp::device_fits(ctx, WHO, device_bytes(K, W, vsxe::table_size_for(K), o.want_quality ? reads->bytes : 0), nullptr, &fits);
      if (rc != VSX_OK) return rc;
      if (!fits) host_all = true;       // buffers that do not fit: the host, as a whole
    }
  if (host_all || K == 0) host_groups(in, G);
  else rc = device_groups(ctx, in, W, G);
  if (rc == VSX_OK)
    {
      const double t0 = now_s();
      rc = finish(in, G, *out);
      g_stats.seconds_output += now_s() - t0;
    }
  if (rc != VSX_OK) { release(out); return rc; }
  g_stats.seconds_total = now_s() - t_begin;
  return VSX_OK;
}

}  // extern "C"
