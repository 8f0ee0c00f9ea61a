// vsx_lca.cpp -- host side of vsx_lca (include/vsx_lca.h): the checks, the routes, the index build and the windows around the
// kernels of vsx_lca.hip, the cutoff test and the host restatement.
//
//   index     device: the labels go up once; split, sort, heads, verify (vsx_lca_internal.h); start / len and the numbers come
//             down, the numbers also stay on the device.  A verified collision: the host numbers the prefixes itself from the
//             split it was given (host_collision) and uploads them.  host: vsx_tax_split.h per label on the threads, then the same
//             host numbering.
//   call      device: `first` goes up once; per window of queries the hits' targets (and ids under top_hits_only) are gathered
//             from the hit records, go up, the vote kernel runs, nine (matches, first hit) pairs and n_top per query come down.
//             host: the reference's loop per query on the threads, comparing prefix numbers where the reference compares bytes.
//   verdict   1.0 * matches / n_top < lca_cutoff in the reference's double arithmetic, on the host for both routes; everything
//             from the first failing level on is blanked.
//   vsx_internal_lca_host   the same loop over the labels' bytes, as the reference has it; no numbers.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/vsx_lca.h"
#include "vsx_private.h"
#include "vsx_lca_internal.h"
#include "vsx_tax_split.h"

using vsxp::DevBuf;
using vsxp::env_u64;
using vsxp::fail;
using vsxp::now_s;
using vsxp::Scratch;

struct vsx_lca_index {
  vsx_ctx * ctx = nullptr;
  uint64_t n = 0;
  bool device = false;                       // the numbers are on the device too: calls may vote there
  std::vector<int32_t> start, len;           // 9 n
  std::vector<uint32_t> id;                  // 9 n; without them (vsx_internal_lca_host) the bytes are compared
  const vsx_labels * labels = nullptr;       // only during vsx_internal_lca_host
  DevBuf<uint32_t> d_id;
  vsx_lca_stats made {};                     // the figures of its creation
};

namespace {

constexpr const char * WHO = "vsx_lca";
constexpr const char * WHO_INDEX = "vsx_lca_index_create";
constexpr uint64_t COUNT_LIMIT = (uint64_t) UINT32_MAX - 1;
constexpr int HOST_THREADS = 16;
constexpr int LEVELS = LCA_LEVELS;
constexpr uint64_t DEFAULT_WINDOW = (uint64_t) 1 << 20;

thread_local vsx_lca_stats g_stats {};

int threads_of(int32_t asked) { return std::max(1, std::min(asked > 0 ? asked : vsxp::usable_cpus(), HOST_THREADS)); }

// a rocPRIM call: the first call sizes the temporary storage, the second runs
template <typename F>
int with_temp(const char * who, vsx_ctx * ctx, std::vector<std::unique_ptr<Scratch<uint8_t>>> & temps, F && call)
{
  size_t bytes = 0;
  VSX_HIP_AS(who, call(nullptr, &bytes));
  temps.emplace_back(new Scratch<uint8_t>());
  VSX_HIP_AS(who, temps.back()->alloc(ctx, bytes));
  VSX_HIP_AS(who, call(temps.back()->p, &bytes));
  return VSX_OK;
}

// ---- the labels --------------------------------------------------------------------------------------------------------------
int check_labels(const char * who, const vsx_labels * T)
{
  if (!T) return fail(VSX_EINVAL, "%s: null argument", who);
  if (T->n && (!T->offsets || !T->lengths || (!T->blob && T->bytes))) return fail(VSX_EINVAL, "%s: null argument", who);
  if (const int rc = vsxp::check_spans(who, "a label", T->n, T->offsets, T->lengths, T->bytes)) return rc;
  for (uint64_t i = 0; i < T->n; ++i)
    {
      if (T->lengths[i] > (uint32_t) INT32_MAX) return fail(VSX_EINVAL, "%s: label %llu is longer than %d bytes", who, (unsigned long long) i, INT32_MAX);
      if (T->lengths[i] && std::memchr(T->blob + T->offsets[i], 0, T->lengths[i]))
        return fail(VSX_EINVAL, "%s: label %llu holds a NUL byte", who, (unsigned long long) i);
    }
  return VSX_OK;
}

void split_on_host(const vsx_labels * T, int nth, std::vector<int32_t> & start, std::vector<int32_t> & len)
{
  start.assign(T->n * LEVELS, 0); len.assign(T->n * LEVELS, 0);
  const uint64_t n = T->n;
  vsxp::run_pool(nth, [&](int t) {
    for (uint64_t i = n * (uint64_t) t / (uint64_t) nth; i < n * (uint64_t) (t + 1) / (uint64_t) nth; ++i)
      {
        int st[LEVELS], ln[LEVELS];
        vsxtax::tax_split(T->lengths[i] ? T->blob + T->offsets[i] : "", (int) T->lengths[i], st, ln);
        for (int k = 0; k < LEVELS; ++k) { start[i * LEVELS + (uint64_t) k] = st[k]; len[i * LEVELS + (uint64_t) k] = ln[k]; }
      }
  });
}

// id[9 i + k]: equal at level k iff the names of levels 0 .. k are equal -- the number of (the number at level k - 1, name k)
void number_on_host(const vsx_labels * T, const std::vector<int32_t> & start, const std::vector<int32_t> & len, std::vector<uint32_t> & id)
{
  id.assign(T->n * LEVELS, 0);
  std::unordered_map<std::string, uint32_t> seen[LEVELS];
  std::string key;
  for (uint64_t i = 0; i < T->n; ++i)
    {
      uint32_t prev = 0;
      for (int k = 0; k < LEVELS; ++k)
        {
          const uint64_t e = i * LEVELS + (uint64_t) k;
          key.assign(reinterpret_cast<const char *>(&prev), sizeof prev);
          if (len[e]) key.append(T->blob + T->offsets[i] + start[e], (size_t) len[e]);
          prev = seen[k].emplace(key, (uint32_t) seen[k].size()).first->second;
          id[e] = prev;
        }
    }
}

int index_on_device(vsx_ctx * ctx, hipStream_t st, const vsx_labels * T, uint64_t first, uint64_t span, uint64_t hash_mask, uint32_t hash_bits,
                    vsx_lca_index & X, vsx_lca_stats & S)
{
  const uint32_t n = (uint32_t) T->n, count = n * (uint32_t) LEVELS;
  int rc;
  double t0 = now_s();
  Scratch<uint8_t> blob;
  Scratch<uint64_t> off, key, key_sorted;
  Scratch<uint32_t> len, idx, idx_sorted, mark, head, differ;
  Scratch<int32_t> start, name_len;
  std::vector<std::unique_ptr<Scratch<uint8_t>>> temps;
  std::vector<uint64_t> rebased((size_t) n);
  for (uint32_t i = 0; i < n; ++i) rebased[i] = T->lengths[i] ? T->offsets[i] - first : 0;      // (an empty label may point anywhere)
  VSX_HIP_AS(WHO_INDEX, blob.upload(ctx, reinterpret_cast<const uint8_t *>(T->blob) + first, span, st));
  VSX_HIP_AS(WHO_INDEX, off.upload(ctx, rebased.data(), n, st));
  VSX_HIP_AS(WHO_INDEX, len.upload(ctx, T->lengths, n, st));
  for (Scratch<uint64_t> * a : { &key, &key_sorted }) VSX_HIP_AS(WHO_INDEX, a->alloc(ctx, count));
  for (Scratch<uint32_t> * a : { &idx, &idx_sorted, &mark, &head }) VSX_HIP_AS(WHO_INDEX, a->alloc(ctx, count));
  for (Scratch<int32_t> * a : { &start, &name_len }) VSX_HIP_AS(WHO_INDEX, a->alloc(ctx, count));
  VSX_HIP_AS(WHO_INDEX, differ.alloc(ctx, 1));
  VSX_HIP_AS(WHO_INDEX, X.d_id.alloc(count));
  VSX_HIP_AS(WHO_INDEX, hipMemsetAsync(differ.p, 0, sizeof(uint32_t), st));
  VSX_HIP_AS(WHO_INDEX, hipStreamSynchronize(st));
  S.seconds_index_stage += now_s() - t0;

  t0 = now_s();
  VSX_HIP_AS(WHO_INDEX, vsx_launch_lca_split(n, blob.p, off.p, len.p, hash_mask, start.p, name_len.p, key.p, idx.p, st));
  VSX_HIP_AS(WHO_INDEX, vsxp::download(X.start, start.p, count, st));
  VSX_HIP_AS(WHO_INDEX, vsxp::download(X.len, name_len.p, count, st));
  VSX_HIP_AS(WHO_INDEX, hipStreamSynchronize(st));
  // what the kernels hand back is checked before anything -- the verify kernel first -- indexes with it
  for (uint32_t i = 0; i < n; ++i)
    for (int k = 0; k < LEVELS; ++k)
      {
        const uint64_t e = (uint64_t) i * LEVELS + (uint64_t) k;
        if (X.start[e] < 0 || X.len[e] < 0 || (uint64_t) X.start[e] + (uint64_t) X.len[e] > T->lengths[i])
          return fail(VSX_EHIP, "%s: the split of label %u leaves it", WHO_INDEX, i);
      }
  S.seconds_index_split += now_s() - t0;

  t0 = now_s();
  if ((rc = with_temp(WHO_INDEX, ctx, temps, [&](void * t, size_t * b) { return vsx_launch_lca_sort(t, b, key.p, key_sorted.p, idx.p, idx_sorted.p, count, hash_bits, st); })) != VSX_OK) return rc;
  VSX_HIP_AS(WHO_INDEX, vsx_launch_lca_heads(count, key_sorted.p, mark.p, st));
  if ((rc = with_temp(WHO_INDEX, ctx, temps, [&](void * t, size_t * b) { return vsx_launch_lca_scan_max(t, b, mark.p, head.p, count, st); })) != VSX_OK) return rc;
  VSX_HIP_AS(WHO_INDEX, vsx_launch_lca_verify(count, idx_sorted.p, head.p, blob.p, off.p, start.p, name_len.p, X.d_id.p, differ.p, st));
  uint32_t differs = 0;
  VSX_HIP_AS(WHO_INDEX, hipMemcpyAsync(&differs, differ.p, sizeof differs, hipMemcpyDeviceToHost, st));
  VSX_HIP_AS(WHO_INDEX, vsxp::download(X.id, X.d_id.p, count, st));
  VSX_HIP_AS(WHO_INDEX, hipStreamSynchronize(st));
  temps.clear();
  if (differs)
    {
      number_on_host(T, X.start, X.len, X.id);
      VSX_HIP_AS(WHO_INDEX, hipMemcpyAsync(X.d_id.p, X.id.data(), (size_t) count * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      VSX_HIP_AS(WHO_INDEX, hipStreamSynchronize(st));
      S.host_collision = 1;
    }
  S.seconds_index_number += now_s() - t0;
  S.labels_device = n;
  X.device = true;
  return VSX_OK;
}

// ---- the vote on the host: the reference's loop (core/results.cpp:573-658) ----------------------------------------------------
// match(k, a, b): the names of levels 0 .. k of labels a and b agree
template <typename Match>
void vote_query(const vsx_hit * hit, uint64_t nh, const vsx_lca_opts & o, Match && match, VsxLcaVote & v)
{
  const uint64_t toreport = (o.maxhits && (uint64_t) o.maxhits < nh) ? (uint64_t) o.maxhits : nh;
  int64_t votes[LEVELS] = {};
  uint32_t cand[LEVELS] = {};
  uint64_t tophitcount = 0;
  for (int k = 0; k < LEVELS; ++k) { v.matches[k] = 0; v.first[k] = VSX_LCA_NONE; }
  v.n_top = 0;
  if (toreport == 0) return;
  const double top_hit_id = hit[0].id;
  for (uint64_t t = 0; t < toreport; ++t)
    {
      if (o.top_hits_only && hit[t].id < top_hit_id) break;
      ++tophitcount;
      const uint32_t seqno = hit[t].target;
      for (int k = 0; k < LEVELS; ++k)
        {
          if (votes[k] == 0) { cand[k] = seqno; votes[k] = 1; }
          else if (match(k, cand[k], seqno)) ++votes[k];
          else --votes[k];
        }
    }
  // count actual matches to the candidate at each level (and keep the first: the representative)
  for (uint64_t t = 0; t < tophitcount; ++t)
    for (int k = 0; k < LEVELS; ++k)
      if (match(k, cand[k], hit[t].target))
        {
          ++v.matches[k];
          if (v.first[k] == VSX_LCA_NONE) v.first[k] = (uint32_t) t;
        }
  v.n_top = (uint32_t) tophitcount;
}

void vote_on_host(const vsx_lca_index & X, const vsx_lca_opts & o, const vsx_hits * H, int nth, std::vector<VsxLcaVote> & votes)
{
  const uint64_t nq = H->n_queries;
  votes.resize(nq);
  const vsx_labels * T = X.labels;
  auto by_id = [&X](int k, uint32_t a, uint32_t b) { return X.id[(uint64_t) a * LEVELS + (uint64_t) k] == X.id[(uint64_t) b * LEVELS + (uint64_t) k]; };
  auto by_bytes = [&X, T](int k, uint32_t a, uint32_t b) {
    for (int j = 0; j <= k; ++j)
      {
        const uint64_t ea = (uint64_t) a * LEVELS + (uint64_t) j, eb = (uint64_t) b * LEVELS + (uint64_t) j;
        if (X.len[eb] != X.len[ea]) return false;
        if (X.len[ea] && std::memcmp(T->blob + T->offsets[a] + X.start[ea], T->blob + T->offsets[b] + X.start[eb], (size_t) X.len[ea]) != 0) return false;
      }
    return true;
  };
  vsxp::run_pool(nth, [&](int t) {
    for (uint64_t q = nq * (uint64_t) t / (uint64_t) nth; q < nq * (uint64_t) (t + 1) / (uint64_t) nth; ++q)
      {
        const vsx_hit * hit = H->hit + H->first[q];
        const uint64_t nh = H->first[q + 1] - H->first[q];
        if (T) vote_query(hit, nh, o, by_bytes, votes[q]);
        else vote_query(hit, nh, o, by_id, votes[q]);
      }
  });
}

// ---- the vote on the device ----------------------------------------------------------------------------------------------------
uint64_t window_of(const vsx_lca_opts & o) { return o.window ? o.window : DEFAULT_WINDOW; }

// the most hits a window of the call holds
uint64_t window_hits(const vsx_hits * H, uint64_t window)
{
  uint64_t most = 0;
  for (uint64_t q0 = 0; q0 < H->n_queries; q0 += window)
    most = std::max(most, H->first[std::min(H->n_queries, q0 + window)] - H->first[q0]);
  return most;
}

uint64_t call_bytes(const vsx_hits * H, uint64_t window, uint64_t most_hits)
{
  return 8 * (H->n_queries + 1) + most_hits * 12 + std::min(window, H->n_queries) * sizeof(VsxLcaVote) + ((uint64_t) 16 << 20);
}

int vote_on_device(vsx_lca_index & X, const vsx_lca_opts & o, const vsx_hits * H, int nth, std::vector<VsxLcaVote> & votes)
{
  vsx_ctx * ctx = X.ctx;
  hipStream_t st = vsx_internal_stream(ctx);
  const uint64_t nq = H->n_queries, window = window_of(o);
  votes.resize(nq);
  Scratch<uint64_t> first;
  Scratch<uint32_t> target;
  Scratch<double> hit_id;
  Scratch<VsxLcaVote> vote;
  std::vector<uint32_t> h_target;
  std::vector<double> h_id;
  double t0 = now_s();
  VSX_HIP_AS(WHO, first.upload(ctx, H->first, nq + 1, st));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  g_stats.seconds_h2d += now_s() - t0;
  for (uint64_t q0 = 0; q0 < nq; q0 += window)
    {
      const uint64_t wn = std::min(window, nq - q0), hit0 = H->first[q0], wh = H->first[q0 + wn] - hit0;
      t0 = now_s();
      h_target.resize(wh);
      if (o.top_hits_only) h_id.resize(wh);
      const int gth = (int) std::max<uint64_t>(1, std::min<uint64_t>((uint64_t) nth, wh >> 16));
      vsxp::run_pool(gth, [&](int t) {
        for (uint64_t x = wh * (uint64_t) t / (uint64_t) gth; x < wh * (uint64_t) (t + 1) / (uint64_t) gth; ++x)
          {
            h_target[x] = H->hit[hit0 + x].target;
            if (o.top_hits_only) h_id[x] = H->hit[hit0 + x].id;
          }
      });
      g_stats.seconds_stage += now_s() - t0;
      t0 = now_s();
      VSX_HIP_AS(WHO, target.upload(ctx, h_target.data(), wh, st));
      if (o.top_hits_only) VSX_HIP_AS(WHO, hit_id.upload(ctx, h_id.data(), wh, st));
      VSX_HIP_AS(WHO, vote.alloc(ctx, wn));
      VSX_HIP_AS(WHO, hipStreamSynchronize(st));
      g_stats.seconds_h2d += now_s() - t0;
      t0 = now_s();
      VSX_HIP_AS(WHO, vsx_launch_lca_vote((uint32_t) wn, first.p + q0, hit0, target.p, o.top_hits_only ? hit_id.p : nullptr, X.d_id.p, (uint64_t) o.maxhits,
                                          vote.p, st));
      VSX_HIP_AS(WHO, hipStreamSynchronize(st));
      g_stats.seconds_vote += now_s() - t0;
      t0 = now_s();
      VSX_HIP_AS(WHO, hipMemcpyAsync(votes.data() + q0, vote.p, wn * sizeof(VsxLcaVote), hipMemcpyDeviceToHost, st));
      VSX_HIP_AS(WHO, hipStreamSynchronize(st));
      g_stats.seconds_d2h += now_s() - t0;
      ++g_stats.windows;
    }
  return VSX_OK;
}

// ---- the verdict and the result --------------------------------------------------------------------------------------------------
void release(vsx_lca_result * out)
{
  std::free(out->n_top); std::free(out->depth); std::free(out->matches); std::free(out->target); std::free(out->start); std::free(out->len);
  std::memset(out, 0, sizeof *out);
}

int finish(const char * who, const vsx_lca_index & X, const vsx_lca_opts & o, const vsx_hits * H, const std::vector<VsxLcaVote> & votes, int nth,
           vsx_lca_result * out)
{
  const uint64_t nq = H->n_queries;
  out->n_queries = nq;
  out->n_top = vsxp::host_array<uint32_t>(nq); out->depth = vsxp::host_array<uint32_t>(nq);
  out->matches = vsxp::host_array<uint32_t>(nq * LEVELS); out->target = vsxp::host_array<uint32_t>(nq * LEVELS);
  out->start = vsxp::host_array<uint32_t>(nq * LEVELS); out->len = vsxp::host_array<uint32_t>(nq * LEVELS);
  if (!out->n_top || !out->depth || !out->matches || !out->target || !out->start || !out->len) return fail(VSX_ENOMEM, "%s: out of memory", who);
  std::vector<int> bad((size_t) nth, 0);
  vsxp::run_pool(nth, [&](int t) {
    for (uint64_t q = nq * (uint64_t) t / (uint64_t) nth; q < nq * (uint64_t) (t + 1) / (uint64_t) nth; ++q)
      {
        const VsxLcaVote & v = votes[q];
        const uint64_t nh = H->first[q + 1] - H->first[q];
        uint32_t depth = 0;
        if (v.n_top > nh) { bad[(size_t) t] = 1; continue; }
        if (v.n_top)
          for (; depth < (uint32_t) LEVELS; ++depth)
            if (1.0 * v.matches[depth] / v.n_top < o.lca_cutoff) break;
        out->n_top[q] = v.n_top; out->depth[q] = depth;
        for (uint32_t j = 0; j < (uint32_t) LEVELS; ++j)
          {
            const uint64_t e = q * LEVELS + j;
            out->matches[e] = 0; out->target[e] = VSX_LCA_NONE; out->start[e] = 0; out->len[e] = 0;
            if (j >= depth) continue;
            if (v.first[j] >= v.n_top || v.matches[j] > v.n_top) { bad[(size_t) t] = 1; continue; }
            const uint32_t tg = H->hit[H->first[q] + v.first[j]].target;
            out->matches[e] = v.matches[j]; out->target[e] = tg;
            out->start[e] = (uint32_t) X.start[(uint64_t) tg * LEVELS + j]; out->len[e] = (uint32_t) X.len[(uint64_t) tg * LEVELS + j];
          }
      }
  });
  for (int b : bad) if (b) return fail(VSX_EHIP, "%s: a vote is out of range", who);
  return VSX_OK;
}

int check_call(const char * who, const vsx_lca_opts * o, uint64_t n_labels, const vsx_hits * H, vsx_lca_result * out)
{
  if (!o || !H || !out) return fail(VSX_EINVAL, "%s: null argument", who);
  std::memset(out, 0, sizeof *out);
  if (!H->first || (H->n_hits && !H->hit)) return fail(VSX_EINVAL, "%s: null argument", who);
  if (!(o->lca_cutoff > 0.5 && o->lca_cutoff <= 1.0))
    return fail(VSX_EINVAL, "%s: The argument to lca_cutoff must be larger than 0.5, but not larger than 1.0", who);
  if (o->maxhits < 0 || o->threads < 0) return fail(VSX_EINVAL, "%s: maxhits and threads cannot be negative", who);
  if (H->first[0] != 0 || H->first[H->n_queries] != H->n_hits) return fail(VSX_EINVAL, "%s: first does not run from 0 to n_hits", who);
  for (uint64_t q = 0; q < H->n_queries; ++q)
    if (H->first[q + 1] < H->first[q] || H->first[q + 1] > H->n_hits) return fail(VSX_EINVAL, "%s: first does not ascend at query %llu", who, (unsigned long long) q);
  // (the hit records are 150 bytes apart: the walk over millions of them is shared by the threads)
  const uint64_t nh = H->n_hits;
  const int nth = (int) std::max<uint64_t>(1, std::min<uint64_t>((uint64_t) threads_of(o->threads), nh >> 16));
  std::vector<uint64_t> bad((size_t) nth, UINT64_MAX);
  vsxp::run_pool(nth, [&](int t) {
    for (uint64_t x = nh * (uint64_t) t / (uint64_t) nth; x < nh * (uint64_t) (t + 1) / (uint64_t) nth; ++x)
      if (H->hit[x].target >= n_labels) { bad[(size_t) t] = x; break; }
  });
  for (uint64_t x : bad)
    if (x != UINT64_MAX)
      return fail(VSX_EINVAL, "%s: hit %llu names target %u of %llu labels", who, (unsigned long long) x, H->hit[x].target, (unsigned long long) n_labels);
  return VSX_OK;
}

int index_create(vsx_ctx * ctx, const vsx_labels * T, vsx_lca_index ** out)
{
  g_stats = vsx_lca_stats {};
  const double t_begin = now_s();
  if (!out) return fail(VSX_EINVAL, "%s: null argument", WHO_INDEX);
  *out = nullptr;
  if (const int rc = check_labels(WHO_INDEX, T)) return rc;
  const uint64_t bits = env_u64("VSX_LCA_HASH_BITS", 64);
  if (bits < 1 || bits > 64) return fail(VSX_EINVAL, "%s: VSX_LCA_HASH_BITS must be 1 .. 64", WHO_INDEX);
  std::unique_ptr<vsx_lca_index> X(new vsx_lca_index());
  X->ctx = ctx; X->n = T->n;
  vsx_lca_stats & S = X->made;
  S.labels = T->n;
  uint64_t first = T->bytes, last = 0;
  for (uint64_t i = 0; i < T->n; ++i)
    if (T->lengths[i]) { first = std::min(first, T->offsets[i]); last = std::max(last, T->offsets[i] + T->lengths[i]); }
  const uint64_t span = last > first ? last - first : 0;
  if (span == 0) first = 0;
  S.seconds_index_stage += now_s() - t_begin;

  bool host = true;
  const uint64_t count_limit = std::min<uint64_t>(COUNT_LIMIT, env_u64("VSX_LCA_DEVICE_COUNT", COUNT_LIMIT));
  if (!ctx) S.host_no_context = 1;
  else if (vsxp::env_is_host("VSX_LCA")) S.host_environment = 1;
  else if (T->n > count_limit / LEVELS) S.host_count = 1;
  else host = false;
  if (!host && T->n)
    {
      const uint64_t need = env_u64("VSX_LCA_PRETEND_BYTES", span + 12 * T->n + 52 * LEVELS * T->n + ((uint64_t) 64 << 20));
      bool fit = false;
      if (const int rc = vsxp::device_fits(ctx, WHO_INDEX, need, nullptr, &fit)) return rc;
      if (!fit) { host = true; S.host_memory = 1; }
    }
  if (!host && T->n)
    {
      hipStream_t st = vsx_internal_stream(ctx);
      const int rc = index_on_device(ctx, st, T, first, span, bits == 64 ? ~0ull : ((1ull << bits) - 1), (uint32_t) bits, *X, S);
      (void) hipStreamSynchronize(st);                           // nothing of this call runs on once its blocks go back to the pool
      if (rc != VSX_OK) return rc;
    }
  else
    {
      const int nth = threads_of(0);
      double t0 = now_s();
      split_on_host(T, nth, X->start, X->len);
      S.seconds_index_split += now_s() - t0;
      t0 = now_s();
      number_on_host(T, X->start, X->len, X->id);
      S.seconds_index_number += now_s() - t0;
      S.labels_host = T->n;
      X->device = !host;                                        // (no labels at all: nothing to vote over, the device route stays open)
    }
  S.seconds_index_total = now_s() - t_begin;
  g_stats = S;
  *out = X.release();
  return VSX_OK;
}

int run(vsx_lca_index * X, const vsx_lca_opts * o, const vsx_hits * H, vsx_lca_result * out)
{
  g_stats = vsx_lca_stats {};
  const double t_begin = now_s();
  if (!X) return fail(VSX_EINVAL, "%s: null argument", WHO);
  g_stats = X->made;
  if (const int rc = check_call(WHO, o, X->n, H, out)) return rc;
  const int nth = threads_of(o->threads);
  g_stats.seconds_stage += now_s() - t_begin;

  bool host = true;
  const uint64_t count_limit = std::min<uint64_t>(COUNT_LIMIT, env_u64("VSX_LCA_DEVICE_COUNT", COUNT_LIMIT));
  if (!X->device) host = true;                                  // the index's own reason is already counted
  else if (vsxp::env_is_host("VSX_LCA")) g_stats.host_environment = 1;
  else if (H->n_hits > count_limit || H->n_queries > count_limit) g_stats.host_count = 1;
  else host = false;
  if (!host && H->n_queries && X->n)
    {
      const uint64_t window = window_of(*o);
      const uint64_t need = env_u64("VSX_LCA_PRETEND_BYTES", call_bytes(H, window, window_hits(H, window)));
      bool fit = false;
      if (const int rc = vsxp::device_fits(X->ctx, WHO, need, nullptr, &fit)) return rc;
      if (!fit) { host = true; g_stats.host_memory = 1; }
    }
  std::vector<VsxLcaVote> votes;
  int rc = VSX_OK;
  if (!host && H->n_queries && X->n)
    {
      rc = vote_on_device(*X, *o, H, nth, votes);
      (void) hipStreamSynchronize(vsx_internal_stream(X->ctx));
      g_stats.queries_device = H->n_queries; g_stats.hits_device = H->n_hits;
    }
  else
    {
      const vsxp::Stopwatch watch(g_stats.seconds_output);
      vote_on_host(*X, *o, H, nth, votes);
      g_stats.queries_host = H->n_queries; g_stats.hits_host = H->n_hits;
    }
  if (rc == VSX_OK)
    {
      const vsxp::Stopwatch watch(g_stats.seconds_output);
      rc = finish(WHO, *X, *o, H, votes, nth, out);
    }
  if (rc != VSX_OK) { release(out); return rc; }
  g_stats.seconds_total = now_s() - t_begin;
  return VSX_OK;
}

}  // namespace

extern "C" {

void vsx_lca_opts_default(vsx_lca_opts * o)
{
  std::memset(o, 0, sizeof *o);
  o->lca_cutoff = 1.0;
}

void vsx_lca_last_stats(vsx_lca_stats * out) { if (out) *out = g_stats; }

void vsx_lca_result_free(vsx_lca_result * out) { if (out) release(out); }

int vsx_lca_index_create(vsx_ctx * ctx, const vsx_labels * targets, vsx_lca_index ** out) { return index_create(ctx, targets, out); }

void vsx_lca_index_destroy(vsx_lca_index * index) { delete index; }

int vsx_lca(vsx_lca_index * index, const vsx_lca_opts * opts, const vsx_hits * hits, vsx_lca_result * out) { return run(index, opts, hits, out); }

int vsx_internal_lca_host(const vsx_lca_opts * opts, const vsx_labels * targets, const vsx_hits * hits, vsx_lca_result * out)
{
  static constexpr const char * who = "vsx_internal_lca_host";
  g_stats = vsx_lca_stats {};
  const double t_begin = now_s();
  if (!opts || !out) return fail(VSX_EINVAL, "%s: null argument", who);
  if (const int rc = check_labels(who, targets)) return rc;
  if (const int rc = check_call(who, opts, targets->n, hits, out)) return rc;
  const int nth = threads_of(opts->threads);
  vsx_lca_index X;
  X.n = targets->n; X.labels = targets;
  g_stats.labels = g_stats.labels_host = targets->n;
  double t0 = now_s();
  split_on_host(targets, nth, X.start, X.len);
  g_stats.seconds_index_split = now_s() - t0;
  std::vector<VsxLcaVote> votes;
  int rc;
  {
    const vsxp::Stopwatch watch(g_stats.seconds_output);
    vote_on_host(X, *opts, hits, nth, votes);
    rc = finish(who, X, *opts, hits, votes, nth, out);
  }
  if (rc != VSX_OK) { release(out); return rc; }
  g_stats.queries_host = hits->n_queries; g_stats.hits_host = hits->n_hits;
  g_stats.seconds_total = now_s() - t_begin;
  return VSX_OK;
}

int vsx_internal_lca_index_split(const vsx_lca_index * index, uint64_t n, int32_t * start, int32_t * len)
{
  if (!index || !start || !len || n != index->n) return fail(VSX_EINVAL, "vsx_internal_lca_index_split: null argument or another label count");
  std::copy(index->start.begin(), index->start.end(), start);
  std::copy(index->len.begin(), index->len.end(), len);
  return VSX_OK;
}

}  // extern "C"
