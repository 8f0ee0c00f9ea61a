// vsx_getseqs.cpp -- sequence extraction by label (include/vsx_getseqs.h: vsx_getseqs), the host side of vsx_getseqs.hip and the
// host restatement.
//
// Restated from the reference (src/, v2.31.0): core/getseq.cpp: test_label_match() and the subsequence arithmetic of getseq(),
// utils/compare_strings_nocase.cpp for the folded comparisons.  The reference walks every label for every header; both routes here
// enter the needles (field '=' label in the field modes) into one table keyed by (length, polynomial hash) and look every
// (position, distinct length) of a header up in it (vsx_getseqs_internal.h has the hash).
//
//   device   uploads -> table zeroed and filled by the insert kernel -> match launches of `window` headers -> inclusive sum of the
//            verdicts -> record kernel -> one download.  All device memory comes from the context's scratch pool; every buffer a
//            kernel reads was written by this call.
//   host     the same table built serially, the headers over opts->threads threads, the ordinals by a serial count.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "../../include/vsx_getseqs.h"
#include "vsx_getseqs_internal.h"
#include "vsx_private.h"

using vsxp::fail;
using vsxp::now_s;
using vsxp::Scratch;

namespace {

constexpr const char * WHO = "vsx_getseqs";
constexpr uint64_t COUNT_LIMIT = (uint64_t) UINT32_MAX - 1;
constexpr uint64_t NEEDLE_LIMIT = (uint64_t) 1 << 30;     // needle numbers and the table's slot count stay in 32 bits
constexpr int HOST_THREADS = 16;
constexpr uint64_t WINDOW_DEFAULT = (uint64_t) 1 << 22;

thread_local vsx_getseqs_stats g_stats {};

// what both routes work on: the needles as they are looked for, their distinct lengths, the mode's switches
struct Plan {
  const vsx_labels * H;
  const uint32_t * seqlen;
  const char * nblob;
  uint64_t nbytes;
  const uint64_t * noff;
  const uint32_t * nlen;
  uint32_t nn;
  std::vector<char> composed;                  // field modes: field '=' label, one after the other
  std::vector<uint64_t> coff;
  std::vector<uint32_t> clen;
  std::vector<uint32_t> lengths;               // distinct, ascending
  uint32_t fold, bound, exact, empty_needle;
  uint32_t max_needle, max_header;
  uint64_t hash_mask;
  uint32_t slots;
  int64_t sub_start, sub_end;
  uint64_t window;
  int nth;
};

inline uint64_t inverse_of_base()
{
  uint64_t x = VSX_GS_BASE;                                      // correct to 3 bits; every round doubles them
  for (int r = 0; r < 6; ++r) x *= 2 - VSX_GS_BASE * x;
  return x;
}

inline uint64_t poly_of(const unsigned char * s, uint32_t L, uint32_t fold)
{
  uint64_t acc = 0, pw = 1;
  for (uint32_t j = 0; j < L; ++j, pw *= VSX_GS_BASE) acc += (uint64_t) (vsx_gs_fold(s[j], fold) + 1u) * pw;
  return acc;
}

inline bool equal_folded(const unsigned char * a, const unsigned char * b, uint32_t l, uint32_t fold)
{
  if (!fold) return std::memcmp(a, b, l) == 0;
  for (uint32_t j = 0; j < l; ++j) if (vsx_gs_fold(a[j], 1) != vsx_gs_fold(b[j], 1)) return false;
  return true;
}

// ---- the host route --------------------------------------------------------------------------------------------------------------
struct HostTable {
  std::vector<VsxGetseqsSlot> slots;
  uint32_t mask;
};

void host_table(const Plan & P, HostTable & T)
{
  T.slots.assign(P.slots, VsxGetseqsSlot { 0, 0, 0 });
  T.mask = P.slots - 1;
  if (P.empty_needle) return;
  for (uint32_t i = 0; i < P.nn; ++i)
    {
      const uint32_t l = P.nlen[i];
      const uint64_t key = vsx_gs_key(poly_of(reinterpret_cast<const unsigned char *>(P.nblob) + P.noff[i], l, P.fold), l, P.hash_mask);
      uint32_t at = (uint32_t) key & T.mask;
      while (T.slots[at].id1) at = (at + 1) & T.mask;
      T.slots[at] = VsxGetseqsSlot { key, i + 1, l };
    }
}

bool host_match(const Plan & P, const HostTable & T, uint64_t k, std::vector<uint64_t> & F, uint64_t inv, uint64_t & probes, uint64_t & checks)
{
  const unsigned char * const s = reinterpret_cast<const unsigned char *>(P.H->blob) + P.H->offsets[k];
  const unsigned char * const nb = reinterpret_cast<const unsigned char *>(P.nblob);
  const uint32_t L = P.H->lengths[k];
  if (P.empty_needle) return L != 0;
  if (P.exact)
    {
      const uint64_t key = vsx_gs_key(poly_of(s, L, P.fold), L, P.hash_mask);
      ++probes;
      for (uint32_t at = (uint32_t) key & T.mask; T.slots[at].id1; at = (at + 1) & T.mask)
        {
          const VsxGetseqsSlot & sl = T.slots[at];
          if (sl.key != key || sl.len != L) continue;
          ++checks;
          if (equal_folded(s, nb + P.noff[sl.id1 - 1], L, P.fold)) return true;
        }
      return false;
    }
  if (P.lengths.empty() || L == 0 || P.lengths[0] > L) return false;
  F.resize((size_t) L + 1);
  F[0] = 0;
  uint64_t pw = 1;
  for (uint32_t j = 0; j < L; ++j, pw *= VSX_GS_BASE) F[j + 1] = F[j] + (uint64_t) (vsx_gs_fold(s[j], P.fold) + 1u) * pw;
  uint64_t ipw = 1;
  for (uint32_t p = 0; p < L; ++p, ipw *= inv)
    for (const uint32_t l : P.lengths)
      {
        if (l > L - p) break;
        const uint64_t key = vsx_gs_key((F[p + l] - F[p]) * ipw, l, P.hash_mask);
        ++probes;
        for (uint32_t at = (uint32_t) key & T.mask; T.slots[at].id1; at = (at + 1) & T.mask)
          {
            const VsxGetseqsSlot & sl = T.slots[at];
            if (sl.key != key || sl.len != l) continue;
            ++checks;
            if (!equal_folded(s + p, nb + P.noff[sl.id1 - 1], l, P.fold)) continue;
            bool ok = true;
            if (P.bound == VSX_GS_BOUND_ALNUM) ok = (p == 0 || !vsx_gs_alnum(s[p - 1])) && (p + l == L || !vsx_gs_alnum(s[p + l]));
            else if (P.bound == VSX_GS_BOUND_SEMI) ok = (p == 0 || s[p - 1] == ';') && (p + l == L || s[p + l] == ';');
            if (ok) return true;
            break;                                                // the same bytes at the same place: no other slot decides otherwise
          }
      }
  return false;
}

inline void piece_of(const Plan & P, uint32_t matched, uint32_t len, uint32_t & start, uint32_t & length)
{
  start = 0; length = len;
  if (!matched || P.sub_start <= 0) return;
  const int64_t a = std::max<int64_t>(P.sub_start, 1), e = std::min<int64_t>(P.sub_end, (int64_t) len);
  if (e < a) { start = 0; length = 0; }
  else { start = (uint32_t) (a - 1); length = (uint32_t) (e - a + 1); }
}

int host_route(const Plan & P, vsx_getseqs_out & out)
{
  const uint64_t n = P.H->n;
  double t0 = now_s();
  HostTable T;
  host_table(P, T);
  g_stats.seconds_table += now_s() - t0;
  t0 = now_s();
  const uint64_t inv = inverse_of_base();
  std::vector<uint8_t> verdict(n);
  const int nth = (int) std::max<uint64_t>(1, std::min<uint64_t>((uint64_t) P.nth, n / 1024 + 1));
  std::vector<uint64_t> probes((size_t) nth, 0), checks((size_t) nth, 0);
  vsxp::run_pool(nth, [&](int t) {
    std::vector<uint64_t> F;
    uint64_t pr = 0, ck = 0;
    for (uint64_t k = n * (uint64_t) t / (uint64_t) nth, e = n * (uint64_t) (t + 1) / (uint64_t) nth; k < e; ++k)
      verdict[k] = host_match(P, T, k, F, inv, pr, ck) ? 1 : 0;
    probes[(size_t) t] = pr; checks[(size_t) t] = ck;
  });
  for (int t = 0; t < nth; ++t) { g_stats.probes += probes[(size_t) t]; g_stats.verifications += checks[(size_t) t]; }
  g_stats.seconds_match += now_s() - t0;
  t0 = now_s();
  uint64_t kept = 0, discarded = 0;
  for (uint64_t k = 0; k < n; ++k)
    {
      vsx_getseqs_record & r = out.rec[k];
      r.matched = verdict[k];
      const uint64_t ordinal = verdict[k] ? ++kept : ++discarded;
      if (ordinal > UINT32_MAX) return fail(VSX_EINVAL, "%s: more than 2^32 - 1 sequences of one verdict", WHO);
      r.ordinal = (uint32_t) ordinal;
      piece_of(P, r.matched, P.seqlen[k], r.start, r.length);
    }
  out.kept = kept; out.discarded = discarded;
  g_stats.seconds_ordinals += now_s() - t0;
  g_stats.headers_host = n;
  return VSX_OK;
}

// ---- the device route ------------------------------------------------------------------------------------------------------------
struct DeviceBufs {
  Scratch<uint8_t> hblob, nblob, temp;
  Scratch<uint64_t> hoff, noff;
  Scratch<uint32_t> hlen, nlen, seqlen, lengths, verdict, incl, rec;
  Scratch<VsxGetseqsSlot> slots;
  Scratch<unsigned long long> counters;
};

uint64_t device_bytes(const Plan & P)
{
  return P.H->bytes + P.nbytes + 48 * P.H->n + 16 * (uint64_t) P.nn + sizeof(VsxGetseqsSlot) * (uint64_t) P.slots + ((uint64_t) 64 << 20);
}

int device_run(vsx_ctx * ctx, hipStream_t st, const Plan & P, DeviceBufs & B, vsx_getseqs_out & out)
{
  const vsx_labels & H = *P.H;
  const uint32_t n = (uint32_t) H.n;
  double t0 = now_s();
  VSX_HIP_AS(WHO, B.hblob.upload(ctx, reinterpret_cast<const uint8_t *>(H.blob), H.bytes, st));
  VSX_HIP_AS(WHO, B.hoff.upload(ctx, H.offsets, n, st));
  VSX_HIP_AS(WHO, B.hlen.upload(ctx, H.lengths, n, st));
  VSX_HIP_AS(WHO, B.seqlen.upload(ctx, P.seqlen, n, st));
  VSX_HIP_AS(WHO, B.nblob.upload(ctx, reinterpret_cast<const uint8_t *>(P.nblob), P.nbytes, st));
  VSX_HIP_AS(WHO, B.noff.upload(ctx, P.noff, P.nn, st));
  VSX_HIP_AS(WHO, B.nlen.upload(ctx, P.nlen, P.nn, st));
  VSX_HIP_AS(WHO, B.lengths.upload(ctx, P.lengths.data(), P.lengths.size(), st));
  VSX_HIP_AS(WHO, B.slots.alloc(ctx, P.slots));
  VSX_HIP_AS(WHO, B.counters.alloc(ctx, 2));
  VSX_HIP_AS(WHO, B.verdict.alloc(ctx, n));
  VSX_HIP_AS(WHO, B.incl.alloc(ctx, n));
  VSX_HIP_AS(WHO, B.rec.alloc(ctx, (size_t) n * 4));
  size_t temp_bytes = 0;
  if (n) VSX_HIP_AS(WHO, vsx_launch_getseqs_scan(nullptr, &temp_bytes, nullptr, nullptr, n, st));
  VSX_HIP_AS(WHO, B.temp.alloc(ctx, temp_bytes));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  g_stats.seconds_stage += now_s() - t0;

  // ---- the table
  t0 = now_s();
  VsxGetseqsTable T {};
  T.n = P.empty_needle ? 0 : P.nn; T.blob = B.nblob.p; T.off = B.noff.p; T.len = B.nlen.p; T.slots = B.slots.p; T.slot_mask = P.slots - 1;
  T.fold = P.fold; T.hash_mask = P.hash_mask;
  VSX_HIP_AS(WHO, hipMemsetAsync(B.slots.p, 0, (size_t) P.slots * sizeof(VsxGetseqsSlot), st));
  VSX_HIP_AS(WHO, hipMemsetAsync(B.counters.p, 0, 2 * sizeof(unsigned long long), st));
  VSX_HIP_AS(WHO, vsx_launch_getseqs_insert(T, st));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  g_stats.seconds_table += now_s() - t0;

  // ---- match
  t0 = now_s();
  VsxGetseqsMatch M {};
  M.blob = B.hblob.p; M.off = B.hoff.p; M.len = B.hlen.p; M.T = T;
  M.lengths = B.lengths.p; M.n_lengths = (uint32_t) P.lengths.size(); M.bound = P.bound; M.exact = P.exact; M.empty_needle = P.empty_needle;
  M.lds_entries = P.exact ? 0 : P.max_header + 1; M.base_inv = inverse_of_base(); M.verdict = B.verdict.p; M.counters = B.counters.p;
  for (uint64_t first = 0; first < n; first += P.window)
    {
      M.first = (uint32_t) first; M.count = (uint32_t) std::min<uint64_t>(P.window, n - first);
      VSX_HIP_AS(WHO, vsx_launch_getseqs_match(M, st));
    }
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  g_stats.seconds_match += now_s() - t0;

  // ---- ordinals and records
  t0 = now_s();
  uint32_t kept = 0;
  if (n)
    {
      VSX_HIP_AS(WHO, vsx_launch_getseqs_scan(B.temp.p, &temp_bytes, B.verdict.p, B.incl.p, n, st));
      VSX_HIP_AS(WHO, vsx_launch_getseqs_records(n, B.verdict.p, B.incl.p, B.seqlen.p, P.sub_start, P.sub_end, B.rec.p, st));
      VSX_HIP_AS(WHO, hipMemcpyAsync(&kept, B.incl.p + (n - 1), sizeof kept, hipMemcpyDeviceToHost, st));
    }
  unsigned long long counters[2] = { 0, 0 };
  VSX_HIP_AS(WHO, hipMemcpyAsync(counters, B.counters.p, sizeof counters, hipMemcpyDeviceToHost, st));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  g_stats.seconds_ordinals += now_s() - t0;
  if (kept > n) return fail(VSX_EHIP, "%s: the scan counts %u matches among %u headers", WHO, kept, n);

  t0 = now_s();
  if (n) VSX_HIP_AS(WHO, hipMemcpyAsync(out.rec, B.rec.p, (size_t) n * sizeof(vsx_getseqs_record), hipMemcpyDeviceToHost, st));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  out.kept = kept; out.discarded = n - kept;
  g_stats.probes = counters[0]; g_stats.verifications = counters[1];
  g_stats.headers_device = n;
  g_stats.seconds_output += now_s() - t0;
  return VSX_OK;
}

int device_route(vsx_ctx * ctx, const Plan & P, vsx_getseqs_out & out)
{
  VSX_HIP_AS(WHO, hipSetDevice(vsx_internal_device(ctx)));
  hipStream_t st = vsx_internal_stream(ctx);
  DeviceBufs B;
  const int rc = device_run(ctx, st, P, B, out);
  (void) hipStreamSynchronize(st);                             // nothing of this call runs on once its blocks go back to the pool
  return rc;
}

// ---- the refusals of both routes, and the plan -------------------------------------------------------------------------------------
int check(const vsx_getseqs_opts * o, const vsx_labels * H, const uint32_t * seqlen, const vsx_labels * N, vsx_getseqs_out * out)
{
  if (!o || !H || !N || !out) return fail(VSX_EINVAL, "%s: null argument", WHO);
  if ((H->n && (!H->offsets || !H->lengths || !seqlen)) || (N->n && (!N->offsets || !N->lengths)) || (H->bytes && !H->blob) || (N->bytes && !N->blob))
    return fail(VSX_EINVAL, "%s: null argument", WHO);
  if (o->mode < VSX_GETSEQS_LABEL || o->mode > VSX_GETSEQS_WORDS) return fail(VSX_EINVAL, "%s: unknown mode %d", WHO, o->mode);
  if (o->substr != 0 && o->substr != 1) return fail(VSX_EINVAL, "%s: substr must be 0 or 1", WHO);
  if (o->threads < 0 || o->window < 0) return fail(VSX_EINVAL, "%s: threads and window cannot be negative", WHO);
  if (o->field_len && !o->field) return fail(VSX_EINVAL, "%s: field_len without field", WHO);
  if (o->field_len > (uint64_t) 1 << 30) return fail(VSX_EINVAL, "%s: field of %llu bytes", WHO, (unsigned long long) o->field_len);
  if (o->field && o->field_len && std::memchr(o->field, 0, o->field_len)) return fail(VSX_EINVAL, "%s: a NUL byte in field", WHO);
  if (o->subseq_start != 0 || o->subseq_end != 0)
    {
      if (o->subseq_start < 1 || o->subseq_end < 1)
        return fail(VSX_EINVAL, "%s: The argument to options subseq_start and subseq_end must be at least 1", WHO);
      if (o->subseq_start > o->subseq_end)
        return fail(VSX_EINVAL, "%s: The argument to option subseq_start must be equal or less than to subseq_end", WHO);
    }
  const bool single = o->mode == VSX_GETSEQS_LABEL || o->mode == VSX_GETSEQS_WORD;
  const bool word = o->mode == VSX_GETSEQS_WORD || o->mode == VSX_GETSEQS_WORDS;
  if (N->n > NEEDLE_LIMIT) return fail(VSX_EINVAL, "%s: more than 2^30 needles", WHO);
  if (single && N->n != 1) return fail(VSX_EINVAL, "%s: a single-needle mode takes one needle, not %llu", WHO, (unsigned long long) N->n);
  for (const vsx_labels * S : { H, N })
    for (uint64_t k = 0; k < S->n; ++k)
      if (S->offsets[k] > S->bytes || S->lengths[k] > S->bytes - S->offsets[k])
        return fail(VSX_EINVAL, "%s: %s %llu lies outside its blob", WHO, S == H ? "header" : "needle", (unsigned long long) k);
  for (uint64_t k = 0; k < N->n; ++k)
    {
      if (N->lengths[k] == 0 && word) return fail(VSX_EINVAL, "%s: an empty needle in a word mode", WHO);
      if (N->lengths[k] == 0 && !single) return fail(VSX_EINVAL, "%s: label %llu of the list is empty", WHO, (unsigned long long) k);
      if (N->lengths[k] && std::memchr(N->blob + N->offsets[k], 0, N->lengths[k]))
        return fail(VSX_EINVAL, "%s: a NUL byte in needle %llu", WHO, (unsigned long long) k);
    }
  return VSX_OK;
}

int make_plan(const vsx_getseqs_opts * o, const vsx_labels * H, const uint32_t * seqlen, const vsx_labels * N, Plan & P)
{
  const bool word = o->mode == VSX_GETSEQS_WORD || o->mode == VSX_GETSEQS_WORDS;
  P.H = H; P.seqlen = seqlen;
  P.fold = word ? 0 : 1;
  P.bound = !word ? VSX_GS_BOUND_NONE : (o->field ? VSX_GS_BOUND_SEMI : VSX_GS_BOUND_ALNUM);
  P.exact = (!word && !o->substr) ? 1 : 0;
  P.sub_start = o->subseq_start; P.sub_end = o->subseq_end;
  P.window = o->window > 0 ? (uint64_t) o->window : WINDOW_DEFAULT;
  P.nth = o->threads > 0 ? o->threads : std::max(1, std::min(vsxp::usable_cpus(), HOST_THREADS));
  P.nblob = N->blob; P.nbytes = N->bytes; P.noff = N->offsets; P.nlen = N->lengths;
  P.nn = (uint32_t) N->n;
  if (word && o->field)
    {
      // the reference prints field '=' in front of every label and looks for the whole
      uint64_t total = 0;
      for (uint64_t k = 0; k < N->n; ++k) total += o->field_len + 1 + N->lengths[k];
      P.composed.resize(total); P.coff.resize(N->n); P.clen.resize(N->n);
      uint64_t at = 0;
      for (uint64_t k = 0; k < N->n; ++k)
        {
          const uint64_t l = o->field_len + 1 + N->lengths[k];
          if (l > UINT32_MAX) return fail(VSX_EINVAL, "%s: needle %llu with its field is longer than 2^32 - 1 bytes", WHO, (unsigned long long) k);
          P.coff[k] = at; P.clen[k] = (uint32_t) l;
          if (o->field_len) std::memcpy(&P.composed[at], o->field, o->field_len);
          P.composed[at + o->field_len] = '=';
          if (N->lengths[k]) std::memcpy(&P.composed[at + o->field_len + 1], N->blob + N->offsets[k], N->lengths[k]);
          at += l;
        }
      P.nblob = P.composed.data(); P.nbytes = total; P.noff = P.coff.data(); P.nlen = P.clen.data();
    }
  P.empty_needle = (o->mode == VSX_GETSEQS_LABEL && o->substr && N->n == 1 && P.nlen[0] == 0) ? 1 : 0;
  P.max_needle = 0; P.max_header = 0;
  for (uint32_t k = 0; k < P.nn; ++k) P.max_needle = std::max(P.max_needle, P.nlen[k]);
  for (uint64_t k = 0; k < H->n; ++k) P.max_header = std::max(P.max_header, H->lengths[k]);
  if (!P.empty_needle)
    {
      P.lengths.assign(P.nlen, P.nlen + P.nn);
      std::sort(P.lengths.begin(), P.lengths.end());
      P.lengths.erase(std::unique(P.lengths.begin(), P.lengths.end()), P.lengths.end());
    }
  uint64_t slots = 64;
  while (slots < 2 * (uint64_t) P.nn) slots <<= 1;
  P.slots = (uint32_t) slots;
  P.hash_mask = ~0ull;
  if (const char * env = std::getenv("VSX_GETSEQS_HASH_BITS"))      // (not vsxp::env_u64: a signed value, used only within 1 .. 63)
    {
      const long b = std::strtol(env, nullptr, 10);
      if (b >= 1 && b < 64) P.hash_mask = (1ull << b) - 1;
    }
  g_stats.labels_in_table = P.empty_needle ? 0 : P.nn;
  g_stats.distinct_lengths = P.lengths.size();
  g_stats.table_slots = P.slots;
  return VSX_OK;
}

void release(vsx_getseqs_out * out)
{
  std::free(out->rec);
  std::memset(out, 0, sizeof *out);
}

int run(vsx_ctx * ctx, const vsx_getseqs_opts * opts, const vsx_labels * H, const uint32_t * seqlen, const vsx_labels * N, vsx_getseqs_out * out)
{
  g_stats = vsx_getseqs_stats {};
  const double t_begin = now_s();
  int rc = check(opts, H, seqlen, N, out);
  if (rc != VSX_OK) return rc;
  std::memset(out, 0, sizeof *out);
  Plan P {};
  if ((rc = make_plan(opts, H, seqlen, N, P)) != VSX_OK) return rc;
  out->n = H->n;
  out->rec = static_cast<vsx_getseqs_record *>(std::calloc(std::max<uint64_t>(H->n, 1), sizeof(vsx_getseqs_record)));
  if (!out->rec) return fail(VSX_ENOMEM, "%s: out of memory", WHO);
  g_stats.seconds_stage += now_s() - t_begin;

  bool host_all = true;
  const uint64_t device_headers = std::min<uint64_t>(COUNT_LIMIT, vsxp::env_u64("VSX_GETSEQS_DEVICE_HEADERS", COUNT_LIMIT, true));
  const uint64_t max_lengths = vsxp::env_u64("VSX_GETSEQS_MAX_LENGTHS", UINT64_MAX, true);
  if (!ctx) g_stats.host_no_context = 1;
  else if (vsxp::env_is_host("VSX_GETSEQS")) g_stats.host_environment = 1;
  else if (H->n > device_headers) g_stats.host_count = 1;
  else if (P.max_needle > VSX_GETSEQS_DEVICE_MAX_BYTES) g_stats.host_needle_length = 1;
  else if (!P.exact && P.max_header > VSX_GETSEQS_DEVICE_MAX_BYTES) g_stats.host_header_length = 1;
  else if (!P.exact && P.lengths.size() > max_lengths) g_stats.host_lengths = 1;
  else host_all = false;
  if (!host_all)
    {
      bool fits = false;
      if ((rc = vsxp::device_fits(ctx, WHO, device_bytes(P), "VSX_GETSEQS_PRETEND_BYTES", &fits)) != VSX_OK) { release(out); return rc; }
      if (!fits) { host_all = true; g_stats.host_memory = 1; }
    }
  rc = host_all ? host_route(P, *out) : device_route(ctx, P, *out);
  if (rc != VSX_OK) { release(out); return rc; }
  g_stats.seconds_total = now_s() - t_begin;
  return VSX_OK;
}

}  // namespace

extern "C" {

void vsx_getseqs_opts_default(vsx_getseqs_opts * o) { std::memset(o, 0, sizeof *o); o->mode = VSX_GETSEQS_LABELS; }

void vsx_getseqs_last_stats(vsx_getseqs_stats * out) { if (out) *out = g_stats; }

void vsx_getseqs_out_free(vsx_getseqs_out * out) { if (out) release(out); }

int vsx_getseqs(vsx_ctx * ctx, const vsx_getseqs_opts * opts, const vsx_labels * headers, const uint32_t * seq_lengths, const vsx_labels * needles,
                vsx_getseqs_out * out)
{
  return run(ctx, opts, headers, seq_lengths, needles, out);
}

}  // extern "C"
