// vsx_cut.cpp -- host side of vsx_cut (include/vsx_cut.h): the pattern checks, the routes, the stages around the kernels of vsx_cut.hip
// and the host restatement.
//
//   device    the text goes up packed (sequence k at the sum of the lengths before it; one copy from the caller's memory where the
//             spans are contiguous already) with the block table (bstart[k] = 64-position blocks before sequence k) and the work
//             items (sequence, first block of a tile).  Four points wait for the host, each for one number that sizes the next
//             buffers: the matches, the three list lengths, the bytes of text.
//   host      the literal rule (one comparison loop per position, the reference's running frag_start / rc_start) per sequence on the
//             library's threads, each thread over a contiguous run of sequences balanced by symbols, then a serial pass that joins
//             the runs in order: the ordinals.  Routes: no context, VSX_CUT=host, a count the 32-bit device arrays cannot hold, text
//             and tables that do not fit the device, a pattern longer than VSX_CUT_DEVICE_MAX_PATTERN; each with its counter.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/vsx_cut.h"
#include "vsx_cut_internal.h"
#include "vsx_private.h"

using vsxp::env_u64;
using vsxp::fail;
using vsxp::host_array;
using vsxp::now_s;
using vsxp::Scratch;

static_assert(sizeof(VsxCutRec) == sizeof(vsx_cut_fragment) && sizeof(vsx_cut_fragment) == 16, "the device writes vsx_cut_fragment records");
static_assert(VSX_CUT_MAX_P == VSX_CUT_DEVICE_MAX_PATTERN, "one pattern limit");

namespace {

constexpr const char * WHO = "vsx_cut";
constexpr uint64_t COUNT_LIMIT = (uint64_t) UINT32_MAX - 1;
constexpr uint64_t WINDOW_DEFAULT = (uint64_t) 1 << 20;          // sequences per launch of the match kernel
constexpr uint64_t TILE_DEFAULT = 4096;                          // positions per work item
constexpr int HOST_THREADS = 16;
constexpr uint32_t ALL_WANTS = VSX_CUT_WANT_FWD | VSX_CUT_WANT_REV | VSX_CUT_WANT_REV_TEXT | VSX_CUT_WANT_DISCARDED_REV_TEXT;

thread_local vsx_cut_stats g_stats {};

const char * const PATTERN_MESSAGE[6] = { "", "No forward sequence cut site (^) found in pattern", "No reverse sequence cut site (_) found in pattern",
                                          "Multiple cut sites not supported", "Empty cut pattern string", "Illegal character in cut pattern" };

struct Plan {
  uint64_t n = 0;
  const char * blob = nullptr;
  const uint64_t * off = nullptr;
  const uint32_t * len = nullptr;
  std::vector<uint64_t> poff;            // n + 1 packed offsets
  std::vector<uint8_t> code;             // the pattern's 4-bit codes, P of them
  uint32_t cut_fwd = 0, cut_rev = 0;
  uint32_t want = 0;
  uint64_t window = 0, tile_blocks = 0;
  int nth = 1;
  bool fwd() const { return want & VSX_CUT_WANT_FWD; }
  bool rev() const { return want & (VSX_CUT_WANT_REV | VSX_CUT_WANT_REV_TEXT); }
  bool rev_text() const { return want & VSX_CUT_WANT_REV_TEXT; }
  bool disc_text() const { return want & VSX_CUT_WANT_DISCARDED_REV_TEXT; }
};

void release(vsx_cut_out * out)
{
  std::free(out->matches); std::free(out->fwd); std::free(out->rev); std::free(out->uncut);
  std::free(out->text); std::free(out->rev_off); std::free(out->discarded_off);
  std::memset(out, 0, sizeof *out);
}

// the arrays of the result, once the list lengths are known
int allocate(const Plan & P, vsx_cut_out & out, uint64_t n_fwd, uint64_t n_rev, uint64_t n_uncut)
{
  out.n_fwd = n_fwd; out.n_rev = n_rev; out.n_uncut = n_uncut;
  out.uncut = host_array<uint64_t>(n_uncut);
  if (P.fwd()) out.fwd = host_array<vsx_cut_fragment>(n_fwd);
  if (P.rev()) out.rev = host_array<vsx_cut_fragment>(n_rev);
  if (P.rev_text()) out.rev_off = host_array<uint64_t>(n_rev + 1);
  if (P.disc_text()) out.discarded_off = host_array<uint64_t>(n_uncut + 1);
  if (!out.uncut || (P.fwd() && !out.fwd) || (P.rev() && !out.rev) || (P.rev_text() && !out.rev_off) || (P.disc_text() && !out.discarded_off))
    return fail(VSX_ENOMEM, "%s: out of memory", WHO);
  return VSX_OK;
}

// ---- the host restatement ---------------------------------------------------------------------------------------------------------
struct HostRun {
  std::vector<vsx_cut_fragment> fwd, rev;
  std::vector<uint64_t> uncut;
  uint64_t matches = 0;
};

// cut_a_sequence (commands/cut.cpp:114-288) without the printing; both lists always (their lengths are part of every result)
void host_one(const Plan & P, uint64_t k, HostRun & R, uint32_t * matches)
{
  const unsigned char * seq = reinterpret_cast<const unsigned char *>(P.blob) + P.off[k];
  const int64_t L = (int64_t) P.len[k], plen = (int64_t) P.code.size();
  uint32_t local = 0;
  int64_t frag_start = 0, frag_length = L, rc_start = L, rc_length = 0;
  for (int64_t i = 0; i < L - plen + 1; ++i)
    {
      bool match = true;
      for (int64_t j = 0; j < plen && match; ++j) match = (P.code[(size_t) j] & vsxp::map4(seq[i + j])) != 0;
      if (!match) continue;
      ++local;
      frag_length = i + P.cut_fwd - frag_start;
      rc_length = rc_start - (L - (i + P.cut_rev));
      rc_start -= rc_length;
      if (frag_length > 0) R.fwd.push_back({ k, (uint32_t) frag_start, (uint32_t) frag_length });
      // the reference prints rc_buffer[rc_start, rc_start + rc_length): the reverse complement of forward [L - rc_start - rc_length, L - rc_start)
      if (rc_length > 0) R.rev.push_back({ k, (uint32_t) (L - rc_start - rc_length), (uint32_t) rc_length });
      frag_start += frag_length;
    }
  if (local > 0)
    {
      frag_length = L - frag_start;
      rc_length = rc_start;
      rc_start = 0;
      if (frag_length > 0) R.fwd.push_back({ k, (uint32_t) frag_start, (uint32_t) frag_length });
      if (rc_length > 0) R.rev.push_back({ k, (uint32_t) (L - rc_start - rc_length), (uint32_t) rc_length });
    }
  else R.uncut.push_back(k);
  matches[k] = local;
  R.matches += local;
}

int host_route(const Plan & P, vsx_cut_out & out)
{
  const double t0 = now_s();
  const uint64_t n = P.n, symbols = P.poff[n];
  const int nth = (int) std::max<uint64_t>(1, std::min<uint64_t>((uint64_t) P.nth, (symbols + n) / 65536 + 1));
  // thread t takes the sequences [cutoff[t], cutoff[t + 1]): equal shares of symbols + sequences
  std::vector<uint64_t> cutoff((size_t) nth + 1, n);
  cutoff[0] = 0;
  for (int t = 1; t < nth; ++t)
    {
      const uint64_t goal = (symbols + n) / (uint64_t) nth * (uint64_t) t;
      uint64_t lo = cutoff[(size_t) t - 1], hi = n;
      while (lo < hi) { const uint64_t mid = (lo + hi) / 2; if (P.poff[mid] + mid < goal) lo = mid + 1; else hi = mid; }
      cutoff[(size_t) t] = lo;
    }
  std::vector<HostRun> runs((size_t) nth);
  vsxp::run_pool(nth, [&](int t) {
    for (uint64_t k = cutoff[(size_t) t]; k < cutoff[(size_t) t + 1]; ++k) host_one(P, k, runs[(size_t) t], out.matches);
  });
  // the serial pass: the runs in order are the lists in output order, a record's ordinal its index + 1
  uint64_t n_fwd = 0, n_rev = 0, n_uncut = 0;
  for (const HostRun & R : runs) { n_fwd += R.fwd.size(); n_rev += R.rev.size(); n_uncut += R.uncut.size(); out.total_matches += R.matches; }
  const int rc = allocate(P, out, n_fwd, n_rev, n_uncut);
  if (rc != VSX_OK) return rc;
  uint64_t af = 0, ar = 0, au = 0;
  for (const HostRun & R : runs)
    {
      if (P.fwd() && !R.fwd.empty()) std::memcpy(out.fwd + af, R.fwd.data(), R.fwd.size() * sizeof(vsx_cut_fragment));
      if (P.rev() && !R.rev.empty()) std::memcpy(out.rev + ar, R.rev.data(), R.rev.size() * sizeof(vsx_cut_fragment));
      if (!R.uncut.empty()) std::memcpy(out.uncut + au, R.uncut.data(), R.uncut.size() * sizeof(uint64_t));
      af += R.fwd.size(); ar += R.rev.size(); au += R.uncut.size();
    }
  out.uncut_total = n_uncut; out.cut = n - n_uncut;
  // the text: offsets serially, the pieces on the threads
  if (P.rev_text() || P.disc_text())
    {
      uint64_t at = 0;
      if (P.rev_text()) { for (uint64_t x = 0; x < n_rev; ++x) { out.rev_off[x] = at; at += out.rev[x].length; } out.rev_off[n_rev] = at; }
      if (P.disc_text()) { for (uint64_t x = 0; x < n_uncut; ++x) { out.discarded_off[x] = at; at += P.len[out.uncut[x]]; } out.discarded_off[n_uncut] = at; }
      out.text_bytes = at;
      out.text = host_array<char>(at);
      if (!out.text) return fail(VSX_ENOMEM, "%s: out of memory", WHO);
      const uint64_t pieces = (P.rev_text() ? n_rev : 0) + (P.disc_text() ? n_uncut : 0), first_disc = P.rev_text() ? n_rev : 0;
      const int nt = (int) std::max<uint64_t>(1, std::min<uint64_t>((uint64_t) P.nth, at / 65536 + 1));
      vsxp::run_pool(nt, [&](int t) {
        for (uint64_t x = pieces * (uint64_t) t / (uint64_t) nt, e = pieces * (uint64_t) (t + 1) / (uint64_t) nt; x < e; ++x)
          {
            uint64_t k, start, length, to;
            if (x < first_disc) { k = out.rev[x].seq; start = out.rev[x].start; length = out.rev[x].length; to = out.rev_off[x]; }
            else { k = out.uncut[x - first_disc]; start = 0; length = P.len[k]; to = out.discarded_off[x - first_disc]; }
            const unsigned char * src = reinterpret_cast<const unsigned char *>(P.blob) + P.off[k] + start;
            for (uint64_t b = 0; b < length; ++b) out.text[to + b] = (char) vsxsym::complement(src[length - 1 - b]);
          }
      });
    }
  g_stats.seconds_output += now_s() - t0;
  return VSX_OK;
}

// ---- the device route -----------------------------------------------------------------------------------------------------------
struct DeviceBufs {
  Scratch<uint8_t> text, otext;
  Scratch<uint64_t> off;
  Scratch<uint32_t> len, bstart, count, rank, matches, nfwd, nrev, uncut, basef, baser, baseu, ulist;
  Scratch<VsxCutItem> items;
  Scratch<unsigned long long> bits, pos, plen, poffs;
  Scratch<VsxCutRec> fwd, prec;
  std::vector<std::unique_ptr<Scratch<uint8_t>>> temps;       // rocPRIM's temporary storage, kept until the call's last kernel is through
};

// an exclusive scan by vsx_launch_cut_scan32 or vsx_launch_cut_scan64: the first call sizes the temporary storage, the second runs
template <typename T>
int scan(hipError_t (*launch)(void *, size_t *, const T *, T *, uint64_t, hipStream_t), vsx_ctx * ctx, DeviceBufs & B, const T * in, T * out,
         uint64_t count, hipStream_t st)
{
  size_t bytes = 0;
  VSX_HIP_AS(WHO, launch(nullptr, &bytes, in, out, count, st));
  B.temps.emplace_back(new Scratch<uint8_t>());
  VSX_HIP_AS(WHO, B.temps.back()->alloc(ctx, bytes));
  VSX_HIP_AS(WHO, launch(B.temps.back()->p, &bytes, in, out, count, st));
  return VSX_OK;
}

// the block table, and what the first stages need of the device (text, tables, bitmap, counts and ranks, per-sequence arrays)
uint64_t count_blocks(const Plan & P)
{
  uint64_t blocks = 0;
  for (uint64_t k = 0; k < P.n; ++k) blocks += ((uint64_t) P.len[k] + 63) / 64;
  return blocks;
}

uint64_t device_bytes(const Plan & P, uint64_t blocks)
{
  const uint64_t items = blocks / P.tile_blocks + P.n;
  return P.poff[P.n] + 48 * (P.n + 1) + 16 * (blocks + 1) + 8 * items + ((uint64_t) 64 << 20);
}

// what the later stages add once the counts are known
uint64_t device_bytes_lists(uint64_t matches, uint64_t n_fwd, uint64_t n_rev, uint64_t n_uncut, uint64_t text)
{
  return 8 * matches + 16 * n_fwd + 32 * (n_rev + n_uncut + 1) + 4 * n_uncut + text + ((uint64_t) 16 << 20);
}

// the check between the stages (the device is set; no testing aid): a device that does not report its memory sends the call to the
// host route here, where vsxp::device_fits at the start of the call fails it
bool fits(uint64_t need)
{
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void) hipGetLastError(); return false; }
  return need + VSX_DEVICE_RESERVE_BYTES <= free_b;
}

// *host = true: the lists do not fit the device beside the text; nothing of `out` is filled and the caller takes the host route
int device_run(vsx_ctx * ctx, hipStream_t st, const Plan & P, uint64_t blocks, DeviceBufs & B, vsx_cut_out & out, bool * host)
{
  const uint32_t n = (uint32_t) P.n, nb = (uint32_t) blocks;
  const uint64_t symbols = P.poff[P.n];
  VsxCutPattern pat {};
  pat.P = (uint32_t) P.code.size(); pat.cut_fwd = P.cut_fwd; pat.cut_rev = P.cut_rev;
  std::memcpy(pat.code, P.code.data(), P.code.size());

  // ---- tables and text
  double t0 = now_s();
  std::vector<uint32_t> bstart((size_t) n + 1);
  std::vector<uint64_t> item0((size_t) n + 1);
  std::vector<VsxCutItem> items;
  bool contiguous = true;
  for (uint32_t k = 0; k < n; ++k)
    {
      const uint32_t b = (uint32_t) (((uint64_t) P.len[k] + 63) / 64);
      bstart[k + 1] = bstart[k] + b;
      item0[k] = items.size();
      for (uint64_t b0 = 0; b0 < b; b0 += P.tile_blocks) items.push_back({ k, (uint32_t) b0 });
      if (k && P.off[k] != P.off[k - 1] + P.len[k - 1]) contiguous = false;
    }
  item0[n] = items.size();
  std::vector<char> packed;
  const char * src = n ? P.blob + P.off[0] : nullptr;
  if (!contiguous)
    {
      packed.resize(symbols);
      for (uint32_t k = 0; k < n; ++k) if (P.len[k]) std::memcpy(&packed[P.poff[k]], P.blob + P.off[k], P.len[k]);
      src = packed.data();
    }
  g_stats.items = items.size();
  g_stats.seconds_stage += now_s() - t0;

  t0 = now_s();
  VSX_HIP_AS(WHO, B.text.upload(ctx, reinterpret_cast<const uint8_t *>(src), symbols, st));
  VSX_HIP_AS(WHO, B.off.upload(ctx, P.poff.data(), (size_t) n + 1, st));
  VSX_HIP_AS(WHO, B.len.upload(ctx, P.len, n, st));
  VSX_HIP_AS(WHO, B.bstart.upload(ctx, bstart.data(), (size_t) n + 1, st));
  VSX_HIP_AS(WHO, B.items.upload(ctx, items.data(), items.size(), st));
  VSX_HIP_AS(WHO, B.bits.alloc(ctx, nb));
  VSX_HIP_AS(WHO, B.count.alloc(ctx, (size_t) nb + 1));
  VSX_HIP_AS(WHO, B.rank.alloc(ctx, (size_t) nb + 1));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  g_stats.seconds_h2d += now_s() - t0;

  // ---- match
  t0 = now_s();
  VSX_HIP_AS(WHO, hipMemsetAsync(B.count.p + nb, 0, sizeof(uint32_t), st));
  for (uint64_t k0 = 0; k0 < n; k0 += P.window)
    {
      const uint64_t k1 = std::min<uint64_t>(n, k0 + P.window);
      VSX_HIP_AS(WHO, vsx_launch_cut_match(B.text.p, B.off.p, B.len.p, B.bstart.p, B.items.p + item0[k0], (uint32_t) (item0[k1] - item0[k0]),
                                           (uint32_t) P.tile_blocks, pat, B.bits.p, B.count.p, st));
    }
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  g_stats.seconds_match += now_s() - t0;

  // ---- ranks and positions
  t0 = now_s();
  int rc = scan(vsx_launch_cut_scan32, ctx, B, B.count.p, B.rank.p, (uint64_t) nb + 1, st);
  if (rc != VSX_OK) return rc;
  uint32_t n_matches = 0;
  VSX_HIP_AS(WHO, hipMemcpyAsync(&n_matches, B.rank.p + nb, sizeof n_matches, hipMemcpyDeviceToHost, st));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  if ((uint64_t) n_matches > symbols) return fail(VSX_EHIP, "%s: the scan counts %u matches in %llu symbols", WHO, n_matches, (unsigned long long) symbols);
  if (!fits(device_bytes_lists(n_matches, 0, 0, 0, 0))) { *host = true; return VSX_OK; }
  VSX_HIP_AS(WHO, B.pos.alloc(ctx, n_matches));
  VSX_HIP_AS(WHO, vsx_launch_cut_compact(B.bits.p, B.rank.p, nb, B.pos.p, st));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  g_stats.seconds_rank += now_s() - t0;

  // ---- per-sequence counts, bases, records
  t0 = now_s();
  for (Scratch<uint32_t> * a : { &B.matches, &B.nfwd, &B.nrev, &B.uncut, &B.basef, &B.baser, &B.baseu }) VSX_HIP_AS(WHO, a->alloc(ctx, (size_t) n + 1));
  for (Scratch<uint32_t> * a : { &B.nfwd, &B.nrev, &B.uncut }) VSX_HIP_AS(WHO, hipMemsetAsync(a->p + n, 0, sizeof(uint32_t), st));
  VSX_HIP_AS(WHO, vsx_launch_cut_seqinfo(n, B.len.p, B.bstart.p, B.rank.p, B.pos.p, pat, B.matches.p, B.nfwd.p, B.nrev.p, B.uncut.p, st));
  if ((rc = scan(vsx_launch_cut_scan32, ctx, B, B.nfwd.p, B.basef.p, (uint64_t) n + 1, st)) != VSX_OK) return rc;
  if ((rc = scan(vsx_launch_cut_scan32, ctx, B, B.nrev.p, B.baser.p, (uint64_t) n + 1, st)) != VSX_OK) return rc;
  if ((rc = scan(vsx_launch_cut_scan32, ctx, B, B.uncut.p, B.baseu.p, (uint64_t) n + 1, st)) != VSX_OK) return rc;
  uint32_t totals[3] = { 0, 0, 0 };
  VSX_HIP_AS(WHO, hipMemcpyAsync(&totals[0], B.basef.p + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  VSX_HIP_AS(WHO, hipMemcpyAsync(&totals[1], B.baser.p + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  VSX_HIP_AS(WHO, hipMemcpyAsync(&totals[2], B.baseu.p + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  const uint64_t n_fwd = totals[0], n_rev = totals[1], n_uncut = totals[2];
  if (n_uncut > n || n_fwd > (uint64_t) n_matches + n || n_rev > (uint64_t) n_matches + n)
    return fail(VSX_EHIP, "%s: the scans count %llu + %llu fragments and %llu uncut sequences", WHO, (unsigned long long) n_fwd,
                (unsigned long long) n_rev, (unsigned long long) n_uncut);
  const bool text = P.rev_text() || P.disc_text();
  const bool pieces = P.rev() || text;
  const uint64_t n_pieces = n_rev + n_uncut;
  if (!fits(device_bytes_lists(0, n_fwd, n_rev, n_uncut, text ? symbols : 0))) { *host = true; return VSX_OK; }
  if (P.fwd()) VSX_HIP_AS(WHO, B.fwd.alloc(ctx, n_fwd));
  if (pieces) VSX_HIP_AS(WHO, B.prec.alloc(ctx, n_pieces));
  if (text) { VSX_HIP_AS(WHO, B.plen.alloc(ctx, n_pieces + 1)); VSX_HIP_AS(WHO, B.poffs.alloc(ctx, n_pieces + 1)); }
  VSX_HIP_AS(WHO, B.ulist.alloc(ctx, n_uncut));
  VSX_HIP_AS(WHO, vsx_launch_cut_fragments(n, n_matches, B.len.p, B.bstart.p, B.rank.p, B.pos.p, pat, B.basef.p, B.baser.p, P.fwd() ? B.fwd.p : nullptr,
                                           pieces ? B.prec.p : nullptr, text ? B.plen.p : nullptr, P.rev_text() ? 1 : 0, st));
  VSX_HIP_AS(WHO, vsx_launch_cut_uncut(n, B.len.p, B.matches.p, B.baseu.p, B.ulist.p, pieces ? B.prec.p + n_rev : nullptr,
                                       text ? B.plen.p + n_rev : nullptr, P.disc_text() ? 1 : 0, st));
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  g_stats.seconds_fragments += now_s() - t0;

  // ---- text
  t0 = now_s();
  std::vector<uint64_t> poffs;
  uint64_t text_bytes = 0;
  if (text)
    {
      VSX_HIP_AS(WHO, hipMemsetAsync(B.plen.p + n_pieces, 0, sizeof(uint64_t), st));
      if ((rc = scan(vsx_launch_cut_scan64, ctx, B, reinterpret_cast<const uint64_t *>(B.plen.p), reinterpret_cast<uint64_t *>(B.poffs.p), n_pieces + 1, st)) != VSX_OK) return rc;
      poffs.resize(n_pieces + 1);
      VSX_HIP_AS(WHO, hipMemcpyAsync(poffs.data(), B.poffs.p, (n_pieces + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
      VSX_HIP_AS(WHO, hipStreamSynchronize(st));
      text_bytes = poffs[n_pieces];
      if (text_bytes > 2 * symbols) return fail(VSX_EHIP, "%s: the scan counts %llu bytes of text", WHO, (unsigned long long) text_bytes);
      VSX_HIP_AS(WHO, B.otext.alloc(ctx, text_bytes));
      VSX_HIP_AS(WHO, vsx_launch_cut_emit(B.text.p, B.off.p, B.prec.p, B.poffs.p, n_pieces, text_bytes, B.otext.p, st));
      VSX_HIP_AS(WHO, hipStreamSynchronize(st));
    }
  g_stats.seconds_emit += now_s() - t0;

  // ---- results
  t0 = now_s();
  if ((rc = allocate(P, out, n_fwd, n_rev, n_uncut)) != VSX_OK) return rc;
  std::vector<uint32_t> ulist(n_uncut);
  if (n) VSX_HIP_AS(WHO, hipMemcpyAsync(out.matches, B.matches.p, (size_t) n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (P.fwd() && n_fwd) VSX_HIP_AS(WHO, hipMemcpyAsync(out.fwd, B.fwd.p, n_fwd * sizeof(vsx_cut_fragment), hipMemcpyDeviceToHost, st));
  if (P.rev() && n_rev) VSX_HIP_AS(WHO, hipMemcpyAsync(out.rev, B.prec.p, n_rev * sizeof(vsx_cut_fragment), hipMemcpyDeviceToHost, st));
  if (n_uncut) VSX_HIP_AS(WHO, hipMemcpyAsync(ulist.data(), B.ulist.p, n_uncut * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (text)
    {
      out.text = host_array<char>(text_bytes);
      if (!out.text) return fail(VSX_ENOMEM, "%s: out of memory", WHO);
      out.text_bytes = text_bytes;
      if (text_bytes) VSX_HIP_AS(WHO, hipMemcpyAsync(out.text, B.otext.p, text_bytes, hipMemcpyDeviceToHost, st));
      if (P.rev_text()) std::memcpy(out.rev_off, poffs.data(), (n_rev + 1) * sizeof(uint64_t));
      if (P.disc_text()) std::memcpy(out.discarded_off, poffs.data() + n_rev, (n_uncut + 1) * sizeof(uint64_t));
    }
  VSX_HIP_AS(WHO, hipStreamSynchronize(st));
  for (uint64_t x = 0; x < n_uncut; ++x) out.uncut[x] = ulist[x];
  out.cut = n - n_uncut; out.uncut_total = n_uncut; out.total_matches = n_matches;
  g_stats.seconds_output += now_s() - t0;
  return VSX_OK;
}

int device_route(vsx_ctx * ctx, const Plan & P, uint64_t blocks, vsx_cut_out & out, bool * host)
{
  hipStream_t st = vsx_internal_stream(ctx);
  DeviceBufs B;
  const int rc = device_run(ctx, st, P, blocks, B, out, host);
  (void) hipStreamSynchronize(st);                             // nothing of this call runs on once its blocks go back to the pool
  return rc;
}

int run(vsx_ctx * ctx, const vsx_cut_opts * o, uint64_t n, const char * blob, uint64_t blob_bytes, const uint64_t * offsets, const uint32_t * lengths,
        vsx_cut_out * out)
{
  g_stats = vsx_cut_stats {};
  const double t_begin = now_s();
  if (!o || !out) return fail(VSX_EINVAL, "%s: null argument", WHO);
  std::memset(out, 0, sizeof *out);
  if ((n && (!offsets || !lengths || (!blob && blob_bytes))) || (o->pattern_len && !o->pattern)) return fail(VSX_EINVAL, "%s: null argument", WHO);
  if (o->want & ~ALL_WANTS) return fail(VSX_EINVAL, "%s: unknown bit in want", WHO);
  if (o->window < 0 || o->threads < 0) return fail(VSX_EINVAL, "%s: threads and window cannot be negative", WHO);
  if (o->pattern_len > (uint64_t) INT32_MAX) return fail(VSX_EINVAL, "%s: a pattern of %llu bytes", WHO, (unsigned long long) o->pattern_len);
  Plan P;
  std::string stripped((size_t) o->pattern_len, '\0');
  uint64_t plen = 0;
  int32_t cut_fwd = 0, cut_rev = 0;
  const int cause = vsx_cut_pattern_check(o->pattern, o->pattern_len, &stripped[0], &plen, &cut_fwd, &cut_rev);
  if (cause != VSX_CUT_PATTERN_OK) return fail(VSX_EINVAL, "%s: %s", WHO, PATTERN_MESSAGE[cause]);
  P.code.resize(plen);
  for (uint64_t j = 0; j < plen; ++j) P.code[j] = vsxp::map4((unsigned char) stripped[j]);
  P.cut_fwd = (uint32_t) cut_fwd; P.cut_rev = (uint32_t) cut_rev;
  P.n = n; P.blob = blob; P.off = offsets; P.len = lengths; P.want = o->want;
  P.window = o->window > 0 ? (uint64_t) o->window : WINDOW_DEFAULT;
  P.nth = o->threads > 0 ? o->threads : std::max(1, std::min(vsxp::usable_cpus(), HOST_THREADS));
  const uint64_t tile = env_u64("VSX_CUT_TILE", TILE_DEFAULT);
  if (tile < 64 || tile % 64 || tile > ((uint64_t) 1 << 30)) return fail(VSX_EINVAL, "%s: VSX_CUT_TILE must be a multiple of 64 up to 2^30", WHO);
  P.tile_blocks = tile / 64;
  if (const int rc = vsxp::check_spans(WHO, "a sequence", n, offsets, lengths, blob_bytes)) return rc;
  P.poff.assign(n + 1, 0);
  for (uint64_t k = 0; k < n; ++k)
    {
      if (lengths[k] > (uint32_t) INT32_MAX) return fail(VSX_EINVAL, "%s: a sequence is longer than INT32_MAX", WHO);
      P.poff[k + 1] = P.poff[k] + lengths[k];
    }
  out->n = n;
  out->matches = static_cast<uint32_t *>(std::calloc(std::max<uint64_t>(n, 1), sizeof(uint32_t)));
  if (!out->matches) return fail(VSX_ENOMEM, "%s: out of memory", WHO);
  const uint64_t symbols = P.poff[n], blocks = count_blocks(P);
  g_stats.sequences = n; g_stats.symbols = symbols; g_stats.tile = tile; g_stats.pattern_length = plen;
  g_stats.seconds_stage += now_s() - t_begin;

  // ---- the route
  bool host = true;
  const uint64_t count_limit = std::min<uint64_t>(COUNT_LIMIT, env_u64("VSX_CUT_DEVICE_COUNT", COUNT_LIMIT));
  if (!ctx) g_stats.host_no_context = 1;
  else if (vsxp::env_is_host("VSX_CUT")) g_stats.host_environment = 1;
  else if (n > count_limit || symbols + n > count_limit) g_stats.host_count = 1;      // every list holds at most matches + sequences records
  else if (plen > VSX_CUT_DEVICE_MAX_PATTERN) g_stats.host_pattern_length = 1;
  else host = false;
  int rc = VSX_OK;
  if (!host && n)
    {
      // (the testing aid is read here, not by device_fits: in this command an empty value counts as unset)
      const uint64_t need = env_u64("VSX_CUT_PRETEND_BYTES", device_bytes(P, blocks));
      bool fit = false;
      if ((rc = vsxp::device_fits(ctx, WHO, need, nullptr, &fit)) != VSX_OK) { release(out); return rc; }
      if (!fit) { host = true; g_stats.host_memory = 1; }
    }
  if (!host && n)
    {
      g_stats.blocks = blocks;
      bool lists_do_not_fit = false;
      rc = device_route(ctx, P, blocks, *out, &lists_do_not_fit);
      if (rc == VSX_OK && lists_do_not_fit) { host = true; g_stats.host_memory = 1; g_stats.blocks = 0; g_stats.items = 0; }
    }
  if (rc == VSX_OK && (host || n == 0)) rc = host_route(P, *out);
  if (rc != VSX_OK) { release(out); return rc; }
  g_stats.seconds_total = now_s() - t_begin;
  return VSX_OK;
}

}  // namespace

extern "C" {

void vsx_cut_opts_default(vsx_cut_opts * o)
{
  std::memset(o, 0, sizeof *o);
  o->want = ALL_WANTS;
}

int vsx_cut_pattern_check(const char * pattern, uint64_t len, char * stripped, uint64_t * plen, int32_t * cut_fwd, int32_t * cut_rev)
{
  // commands/cut.cpp:315-384, in the order of cut(): the circumflex, the underscore, then the pattern without them
  uint64_t carets = 0, unders = 0;
  for (uint64_t x = 0; x < len; ++x) { carets += pattern[x] == '^'; unders += pattern[x] == '_'; }
  if (carets == 0) return VSX_CUT_PATTERN_NO_FWD;
  if (carets > 1) return VSX_CUT_PATTERN_MULTIPLE;
  if (unders == 0) return VSX_CUT_PATTERN_NO_REV;
  if (unders > 1) return VSX_CUT_PATTERN_MULTIPLE;
  if (len == 2) return VSX_CUT_PATTERN_EMPTY;
  uint64_t at = 0, fwd = 0, rev = 0;
  for (uint64_t x = 0; x < len; ++x)
    {
      if (pattern[x] == '^') fwd = at;                // symbols in front of it: its index once '_' is gone
      else if (pattern[x] == '_') rev = at;
      else
        {
          if (vsxp::map4((unsigned char) pattern[x]) == 0) return VSX_CUT_PATTERN_ILLEGAL;
          if (stripped) stripped[at] = pattern[x];
          ++at;
        }
    }
  if (plen) *plen = at;
  if (cut_fwd) *cut_fwd = (int32_t) fwd;
  if (cut_rev) *cut_rev = (int32_t) rev;
  return VSX_CUT_PATTERN_OK;
}

void vsx_cut_last_stats(vsx_cut_stats * out) { if (out) *out = g_stats; }

void vsx_cut_out_free(vsx_cut_out * out) { if (out) release(out); }

int vsx_cut(vsx_ctx * ctx, const vsx_cut_opts * opts, uint64_t n, const char * blob, uint64_t blob_bytes,
            const uint64_t * offsets, const uint32_t * lengths, vsx_cut_out * out)
{
  return run(ctx, opts, n, blob, blob_bytes, offsets, lengths, out);
}

}  // extern "C"
