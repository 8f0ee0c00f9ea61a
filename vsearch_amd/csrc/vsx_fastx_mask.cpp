// vsx_fastx_mask.cpp -- host side of vsx_fastx_mask (include/vsx_mask.h): option checks, the staging windows around the kernels of
// vsx_fastx_mask.hip, the routes, the verdicts and the host routes (the restatement itself lives in vsx_mask.cpp).
//
//   packing   the output is PACKED (sequence k at the sum of the lengths before it), so a window is staged packed too: a run of
//             consecutive sequences of at most WINDOW_BYTES symbols, copied sequence by sequence (one memcpy where the caller's spans
//             are contiguous already) behind `shift` = (packed offset of the window) % 64 bytes of padding.  With that shift the
//             64-bit words of the window's bitmap ARE words of the whole bitmap, and a word two windows share is OR-ed on the host.
//   routes    DUST of a sequence below long_min: the walk, one wave per sequence.  From long_min on: W(i) at every position in
//             chunks of CHUNK_POSITIONS (4 bytes per position + 65 bytes per segment), the chain's offset into the next chunk handed
//             on in device memory, so nothing waits for the host between chunks.  qmask none / soft run the apply kernel only.
//   host      VSX_MASK=host (every sequence), a window whose buffers do not fit the device, a long-route sequence whose working set
//             does not fit beside its window: vsx_internal_fastx_mask_one on the library's threads, each route with its counter.
//             VSX_MASK_DEVICE_BYTES (tests) caps what a call may take of the device.
//   verdicts  on the host from the counts: 100.0 * unmasked / len in double, as commands/fastx_mask.cpp:135-147.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "../../include/vsx_mask.h"
#include "vsx_fastx_mask_internal.h"
#include "vsx_private.h"

#pragma clang fp contract(off)

using vsxp::align64;
using vsxp::env_u64;
using vsxp::fail;
using vsxp::now_s;
using vsxp::DevBuf;
using vsxp::PinnedBuf;

namespace {

constexpr const char * WHO = "vsx_fastx_mask";
constexpr uint64_t WINDOW_BYTES = (uint64_t) 64 << 20;       // symbols of one staging window (a single sequence always fits)
constexpr uint64_t WINDOW_SEQUENCES = 262144;
constexpr uint64_t CHUNK_POSITIONS = (uint64_t) 4 << 20;     // positions of a long-route sequence evaluated at a time
// The route threshold, from bench_mask.py's one sequence on both routes (profiles/r19/): in kernel time the long route wins at every
// length measured (10 k: 0.16 ms against 1.08 ms), end to end the call's own fixed costs hide that up to 30 k (8.3 ms against 7.0 ms)
// and the long route is ahead from 100 k on (3.9 ms against 14.6 ms): the crossover lies between, and 64 Ki is inside that bracket.
// It is a per-sequence rule: 1 000 sequences of 20 k in one call are faster by the walk (a wave each), see DESIGN 7.ai.
constexpr uint64_t BUILTIN_LONG_MIN = 65536;
constexpr uint64_t BUILTIN_SEGMENT = 4096;

thread_local vsx_fastx_mask_stats g_stats {};

struct Input {
  uint64_t n;
  const char * blob;
  const uint64_t * off;
  const uint32_t * len;
  std::vector<uint64_t> poff;           // n + 1 packed offsets
};

// sequences [k0, k1) through the host restatement on the library's threads
void host_range(const vsx_fastx_mask_opts & o, const Input & in, uint64_t k0, uint64_t k1, vsx_fastx_mask_out & out)
{
  const uint64_t count = k1 - k0;
  int nth = vsxp::usable_cpus();
  if ((uint64_t) nth > count / 16 + 1) nth = (int) (count / 16 + 1);
  std::atomic<uint64_t> next { k0 }, windows { 0 };
  vsxp::run_pool(nth, [&](int) {
    std::vector<char> work, scratch;
    uint64_t mine = 0;
    for (;;)
      {
        const uint64_t b0 = next.fetch_add(16);
        if (b0 >= k1) break;
        for (uint64_t k = b0; k < std::min(k1, b0 + 16); ++k)
          out.rec[k].unmasked = vsx_internal_fastx_mask_one(in.blob + in.off[k], (int64_t) in.len[k], o.qmask, o.hardmask,
                                                            out.text ? out.text + in.poff[k] : nullptr, out.bits, in.poff[k], work, scratch, &mine);
      }
    windows += mine;
  });
  g_stats.dust_windows += windows.load();
}

struct Device {
  hipStream_t st = nullptr;
  hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };
  PinnedBuf<uint8_t> h_in, h_out;
  DevBuf<uint8_t> d_in, d_out, d_dbits, d_small, d_w, d_seg;
  ~Device()
  {
    if (st) (void) hipStreamSynchronize(st);
    for (hipEvent_t e : ev) if (e) (void) hipEventDestroy(e);
    if (st) (void) hipStreamDestroy(st);
  }
};

struct Layout {
  uint64_t shift, bytes, text_span, words;          // text_span: shift + bytes; words: 64-bit words of the window's bitmap
  uint64_t in_off, in_len, in_list, in_text, in_bytes;
  uint64_t out_count, out_text, out_bits, out_bytes;
  uint64_t dbits_bytes;
  uint64_t need() const { return in_bytes + out_bytes + dbits_bytes + 4096; }
};

Layout layout(const Input & in, uint64_t w0, uint64_t wn, uint32_t want, bool dust)
{
  Layout l {};
  l.shift = in.poff[w0] & 63;
  l.bytes = in.poff[w0 + wn] - in.poff[w0];
  l.text_span = l.shift + l.bytes;
  l.words = (l.text_span + 63) / 64;
  l.in_off = 0;
  l.in_len = l.in_off + align64(wn * 8);
  l.in_list = l.in_len + align64(wn * 4);
  l.in_text = l.in_list + align64(wn * 4);
  l.in_bytes = l.in_text + align64(l.text_span + VSX_MASK_PAD);
  l.out_count = 0;
  l.out_text = align64(wn * 4);
  l.out_bits = l.out_text + ((want & VSX_MASK_WANT_TEXT) ? align64(l.text_span) : 0);
  l.out_bytes = l.out_bits + ((want & VSX_MASK_WANT_BITS) ? l.words * 8 : 0);
  l.dbits_bytes = dust ? l.words * 8 : 0;
  return l;
}

uint64_t device_budget()
{
  size_t free_b = 0, total_b = 0;
  uint64_t budget = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = free_b > VSX_DEVICE_RESERVE_BYTES ? free_b - VSX_DEVICE_RESERVE_BYTES : 0;
  (void) hipGetLastError();
  return std::min(budget, env_u64("VSX_MASK_DEVICE_BYTES", UINT64_MAX));
}

// one staging window on the device; sequences it has to leave to the host come back in `host_long`
int device_window(Device & D, const vsx_fastx_mask_opts & o, const Input & in, uint64_t w0, uint64_t wn, bool contiguous, const Layout & l,
                  uint64_t budget, uint64_t long_min, uint64_t S, vsx_fastx_mask_out & out, std::vector<uint64_t> & host_long)
{
  const double t0 = now_s();
  const bool dust = o.qmask == VSX_MASK_DUST;
  const bool want_text = o.want & VSX_MASK_WANT_TEXT, want_bits = o.want & VSX_MASK_WANT_BITS;
  if (!D.h_in.p || l.in_bytes > D.h_in.n) VSX_HIP_AS(WHO, D.h_in.alloc(l.in_bytes));
  if (!D.h_out.p || l.out_bytes > D.h_out.n) VSX_HIP_AS(WHO, D.h_out.alloc(l.out_bytes));
  VSX_HIP_AS(WHO, D.d_in.ensure(l.in_bytes));
  VSX_HIP_AS(WHO, D.d_out.ensure(l.out_bytes));
  VSX_HIP_AS(WHO, D.d_dbits.ensure(l.dbits_bytes));
  VSX_HIP_AS(WHO, D.d_small.ensure(64));               // the window counter (8 bytes at 0) and the chain entry (4 bytes at 8)

  // the long-route sequences and their working set: W of one chunk, the exits and true entries of its segments
  const uint64_t base = in.poff[w0];
  uint64_t * h_off = reinterpret_cast<uint64_t *>(D.h_in.p + l.in_off);
  uint32_t * h_len = reinterpret_cast<uint32_t *>(D.h_in.p + l.in_len);
  uint32_t * h_list = reinterpret_cast<uint32_t *>(D.h_in.p + l.in_list);
  uint32_t n_short = 0;
  std::vector<uint64_t> longs;
  uint64_t chunk_max = 0;
  for (uint64_t j = 0; j < wn; ++j)
    {
      const uint64_t k = w0 + j;
      h_off[j] = l.shift + (in.poff[k] - base);
      h_len[j] = in.len[k];
      if (!dust) continue;
      if ((uint64_t) in.len[k] < long_min) { h_list[n_short++] = (uint32_t) j; continue; }
      const uint64_t chunk = std::min((uint64_t) (in.len[k] + S - 1) / S * S, std::max<uint64_t>(S, CHUNK_POSITIONS / S * S));
      const uint64_t need = chunk * 4 + (chunk / S) * (VSX_MASK_ENTRIES + 1) + 4096;
      if (l.need() + need > budget) { host_long.push_back(k); h_len[j] = 0; continue; }        // (the device skips a sequence of length 0)
      longs.push_back(j);
      chunk_max = std::max(chunk_max, chunk);
    }
  if (!longs.empty())
    {
      hipError_t e = D.d_w.ensure(chunk_max * 4);
      if (e == hipSuccess) e = D.d_seg.ensure((chunk_max / S) * (VSX_MASK_ENTRIES + 1));
      if (e == hipErrorOutOfMemory)
        {
          (void) hipGetLastError();
          for (uint64_t j : longs) { host_long.push_back(w0 + j); h_len[j] = 0; }
          longs.clear();
        }
      else if (e != hipSuccess) return vsxp::hip_fail(WHO, "the long route's working set", e, __FILE__, __LINE__);
    }

  uint8_t * h_text = D.h_in.p + l.in_text;
  std::memset(h_text, 0, l.shift);
  if (contiguous) std::memcpy(h_text + l.shift, in.blob + in.off[w0], l.bytes);
  else for (uint64_t j = 0; j < wn; ++j) std::memcpy(h_text + h_off[j], in.blob + in.off[w0 + j], in.len[w0 + j]);
  std::memset(h_text + l.text_span, 0, VSX_MASK_PAD);

  const uint8_t * d_text = D.d_in.p + l.in_text;
  const uint64_t * d_off = reinterpret_cast<const uint64_t *>(D.d_in.p + l.in_off);
  const uint32_t * d_len = reinterpret_cast<const uint32_t *>(D.d_in.p + l.in_len);
  const uint32_t * d_list = reinterpret_cast<const uint32_t *>(D.d_in.p + l.in_list);
  uint32_t * d_count = reinterpret_cast<uint32_t *>(D.d_out.p + l.out_count);
  uint8_t * d_otext = want_text ? D.d_out.p + l.out_text : nullptr;
  unsigned long long * d_obits = want_bits ? reinterpret_cast<unsigned long long *>(D.d_out.p + l.out_bits) : nullptr;
  uint32_t * d_dbits = reinterpret_cast<uint32_t *>(D.d_dbits.p);
  unsigned long long * d_counter = reinterpret_cast<unsigned long long *>(D.d_small.p);
  uint32_t * d_entry = reinterpret_cast<uint32_t *>(D.d_small.p + 8);

  VSX_HIP_AS(WHO, hipEventRecord(D.ev[0], D.st));
  VSX_HIP_AS(WHO, hipMemcpyAsync(D.d_in.p, D.h_in.p, l.in_text + l.text_span + VSX_MASK_PAD, hipMemcpyHostToDevice, D.st));
  VSX_HIP_AS(WHO, hipEventRecord(D.ev[1], D.st));
  VSX_HIP_AS(WHO, hipMemsetAsync(D.d_small.p, 0, 64, D.st));
  VSX_HIP_AS(WHO, hipMemsetAsync(d_count, 0, align64(wn * 4), D.st));
  if (want_bits) VSX_HIP_AS(WHO, hipMemsetAsync(d_obits, 0, l.words * 8, D.st));
  uint64_t positions = 0;
  if (dust)
    {
      VSX_HIP_AS(WHO, hipMemsetAsync(d_dbits, 0, l.dbits_bytes, D.st));
      VSX_HIP_AS(WHO, vsx_launch_mask_short(d_text, d_off, d_len, d_list, n_short, d_dbits, d_counter, D.st));
      uint8_t * d_exit = D.d_seg.p;
      for (uint64_t j : longs)
        {
          const uint32_t L = h_len[j];
          const uint64_t chunk = std::min((uint64_t) (L + S - 1) / S * S, std::max<uint64_t>(S, CHUNK_POSITIONS / S * S));
          uint8_t * d_true = D.d_seg.p + (chunk / S) * VSX_MASK_ENTRIES;
          VSX_HIP_AS(WHO, hipMemsetAsync(d_entry, 0, 4, D.st));
          for (uint64_t c0 = 0; c0 < L; c0 += chunk)
            {
              const uint32_t npos = (uint32_t) std::min<uint64_t>(chunk, L - c0);
              VSX_HIP_AS(WHO, vsx_launch_mask_eval(d_text + h_off[j], L, (uint32_t) c0, npos, reinterpret_cast<uint32_t *>(D.d_w.p), D.st));
              VSX_HIP_AS(WHO, vsx_launch_mask_chain(reinterpret_cast<const uint32_t *>(D.d_w.p), L, (uint32_t) c0, npos, (uint32_t) S, d_exit, d_true,
                                                    d_entry, d_dbits, h_off[j], D.st));
            }
          positions += L;
        }
    }
  VSX_HIP_AS(WHO, hipEventRecord(D.ev[2], D.st));
  VSX_HIP_AS(WHO, vsx_launch_mask_apply(d_text, d_off, d_len, (uint32_t) wn, o.qmask, o.hardmask, d_dbits, d_otext, d_obits, d_count, D.st));
  for (uint64_t j = 0; j < wn; ++j)
    if (h_len[j] > VSX_MASK_APPLY_WHOLE)
      VSX_HIP_AS(WHO, vsx_launch_mask_apply_long(d_text, h_off[j], h_len[j], (uint32_t) j, o.qmask, o.hardmask, d_dbits, d_otext, d_obits, d_count, D.st));
  VSX_HIP_AS(WHO, hipEventRecord(D.ev[3], D.st));
  VSX_HIP_AS(WHO, hipMemcpyAsync(D.h_out.p, D.d_out.p, l.out_bytes, hipMemcpyDeviceToHost, D.st));
  g_stats.seconds_stage += now_s() - t0;

  const double t1 = now_s();
  VSX_HIP_AS(WHO, hipStreamSynchronize(D.st));
  unsigned long long visited = 0;
  if (n_short) VSX_HIP_AS(WHO, hipMemcpy(&visited, d_counter, 8, hipMemcpyDeviceToHost));
  float ms = 0.f;
  VSX_HIP_AS(WHO, hipEventElapsedTime(&ms, D.ev[0], D.ev[1])); g_stats.seconds_h2d += ms * 1e-3;
  VSX_HIP_AS(WHO, hipEventElapsedTime(&ms, D.ev[1], D.ev[2])); g_stats.seconds_mask += ms * 1e-3;
  VSX_HIP_AS(WHO, hipEventElapsedTime(&ms, D.ev[2], D.ev[3])); g_stats.seconds_apply += ms * 1e-3;
  const uint32_t * h_count = reinterpret_cast<const uint32_t *>(D.h_out.p + l.out_count);
  for (uint64_t j = 0; j < wn; ++j) out.rec[w0 + j].unmasked = h_count[j];
  if (want_text && l.bytes) std::memcpy(out.text + base, D.h_out.p + l.out_text + l.shift, l.bytes);
  if (want_bits)
    {
      const uint64_t * w = reinterpret_cast<const uint64_t *>(D.h_out.p + l.out_bits);
      uint64_t * dst = reinterpret_cast<uint64_t *>(out.bits) + (base >> 6);
      for (uint64_t x = 0; x < l.words; ++x) dst[x] |= w[x];
    }
  g_stats.dust_windows += visited + positions;
  g_stats.sequences_long += longs.size();
  if (dust) g_stats.sequences_short += n_short; else g_stats.sequences_device_plain += wn;
  g_stats.seconds_d2h_output += now_s() - t1;
  return VSX_OK;
}

void release(vsx_fastx_mask_out * out)
{
  std::free(out->rec); std::free(out->text); std::free(out->bits);
  std::memset(out, 0, sizeof *out);
}

int run(vsx_ctx * ctx, const vsx_fastx_mask_opts & o, const Input & in, bool host_all, vsx_fastx_mask_out & out)
{
  const uint64_t n = in.n, total = in.poff[n];
  out.n = n;
  out.text_bytes = total;
  out.rec = static_cast<vsx_fastx_mask_record *>(std::calloc(std::max<uint64_t>(n, 1), sizeof(vsx_fastx_mask_record)));
  if (o.want & VSX_MASK_WANT_TEXT) out.text = static_cast<char *>(std::malloc(std::max<uint64_t>(total, 1)));
  if (o.want & VSX_MASK_WANT_BITS) out.bits = static_cast<uint8_t *>(std::calloc((total + 63) / 64 + 1, 8));     // whole 64-bit words
  if (!out.rec || ((o.want & VSX_MASK_WANT_TEXT) && !out.text) || ((o.want & VSX_MASK_WANT_BITS) && !out.bits))
    return fail(VSX_ENOMEM, "%s: out of memory", WHO);
  g_stats.sequences = n;
  g_stats.long_min = env_u64("VSX_MASK_LONG_MIN", BUILTIN_LONG_MIN);
  g_stats.segment = std::max<uint64_t>(VSX_MASK_ENTRIES, env_u64("VSX_MASK_SEGMENT", BUILTIN_SEGMENT));
  if (g_stats.segment > ((uint64_t) 1 << 24)) return fail(VSX_EINVAL, "%s: VSX_MASK_SEGMENT must be at most 2^24", WHO);

  if (host_all)
    {
      const double t0 = now_s();
      host_range(o, in, 0, n, out);
      g_stats.sequences_host_forced = n;
      g_stats.seconds_d2h_output += now_s() - t0;
    }
  else if (n)
    {
      VSX_HIP_AS(WHO, hipSetDevice(vsx_internal_device(ctx)));
      Device D;
      VSX_HIP_AS(WHO, hipStreamCreateWithFlags(&D.st, hipStreamNonBlocking));
      for (hipEvent_t & e : D.ev) VSX_HIP_AS(WHO, hipEventCreate(&e));
      const uint64_t budget = device_budget();
      const uint64_t window = o.window > 0 ? (uint64_t) o.window : WINDOW_SEQUENCES;
      std::vector<uint64_t> host_long;
      for (uint64_t w0 = 0; w0 < n;)
        {
          const double t0 = now_s();
          uint64_t wn = 0;
          bool contiguous = true;
          while (w0 + wn < n && wn < window && (wn == 0 || in.poff[w0 + wn + 1] - in.poff[w0] <= WINDOW_BYTES))
            {
              if (wn && in.off[w0 + wn] != in.off[w0 + wn - 1] + in.len[w0 + wn - 1]) contiguous = false;
              ++wn;
            }
          const Layout l = layout(in, w0, wn, o.want, o.qmask == VSX_MASK_DUST);
          g_stats.seconds_stage += now_s() - t0;
          ++g_stats.windows;
          if (l.need() > budget)
            {
              const double t1 = now_s();
              host_range(o, in, w0, w0 + wn, out);
              g_stats.sequences_host_memory += wn;
              g_stats.seconds_d2h_output += now_s() - t1;
            }
          else
            {
              host_long.clear();
              const int rc = device_window(D, o, in, w0, wn, contiguous, l, budget, g_stats.long_min, g_stats.segment, out, host_long);
              if (rc != VSX_OK) return rc;
              const double t1 = now_s();
              for (uint64_t k : host_long)
                {
                  // (the device skipped it: its text is whatever the buffer held, its bits and count are none)
                  host_range(o, in, k, k + 1, out);
                  ++g_stats.sequences_host_long;
                }
              g_stats.seconds_d2h_output += now_s() - t1;
            }
          w0 += wn;
        }
    }

  for (uint64_t k = 0; k < n; ++k)
    {
      const double pct = 100.0 * (double) out.rec[k].unmasked / (double) in.len[k];       // NaN for an empty sequence: kept
      uint32_t verdict = VSX_MASK_KEPT;
      if (pct < o.min_unmasked_pct) verdict = VSX_MASK_DISCARDED_LESS;
      else if (pct > o.max_unmasked_pct) verdict = VSX_MASK_DISCARDED_MORE;
      out.rec[k].verdict = verdict;
      ++(verdict == VSX_MASK_KEPT ? out.kept : verdict == VSX_MASK_DISCARDED_LESS ? out.discarded_less : out.discarded_more);
    }
  return VSX_OK;
}

// no two sequences share a blob byte: in order where the offsets rise (the common case), else by a sorted index
bool disjoint(uint64_t n, const uint64_t * off, const uint32_t * len)
{
  bool rising = true;
  for (uint64_t k = 1; k < n && rising; ++k) rising = off[k] >= off[k - 1] + len[k - 1];
  if (rising) return true;
  std::vector<uint64_t> idx;
  for (uint64_t k = 0; k < n; ++k) if (len[k]) idx.push_back(k);
  std::sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b) { return off[a] < off[b]; });
  for (size_t x = 1; x < idx.size(); ++x)
    if (off[idx[x]] < off[idx[x - 1]] + len[idx[x - 1]]) return false;
  return true;
}

}  // namespace

extern "C" {

void vsx_fastx_mask_opts_default(vsx_fastx_mask_opts * o)
{
  std::memset(o, 0, sizeof *o);
  o->qmask = VSX_MASK_DUST;
  o->hardmask = 0;
  o->min_unmasked_pct = 0.0;
  o->max_unmasked_pct = 100.0;
  o->want = VSX_MASK_WANT_TEXT | VSX_MASK_WANT_BITS;
}

void vsx_fastx_mask_last_stats(vsx_fastx_mask_stats * out) { if (out) *out = g_stats; }

void vsx_fastx_mask_out_free(vsx_fastx_mask_out * out) { if (out) release(out); }

int vsx_fastx_mask(vsx_ctx * ctx, const vsx_fastx_mask_opts * opts, uint64_t n, const char * blob, uint64_t blob_bytes,
                   const uint64_t * offsets, const uint32_t * lengths, vsx_fastx_mask_out * out)
{
  g_stats = vsx_fastx_mask_stats {};
  const double t_begin = now_s();
  if (!opts || !out) return fail(VSX_EINVAL, "%s: null argument", WHO);
  std::memset(out, 0, sizeof *out);
  if (n && (!offsets || !lengths || (!blob && blob_bytes))) return fail(VSX_EINVAL, "%s: null argument", WHO);
  const bool host_all = vsxp::env_is_host("VSX_MASK");
  if (!ctx && !host_all) return fail(VSX_EINVAL, "%s: no context (only VSX_MASK=host runs without one)", WHO);
  const vsx_fastx_mask_opts & o = *opts;
  if (o.qmask < VSX_MASK_NONE || o.qmask > VSX_MASK_DUST) return fail(VSX_EINVAL, "%s: qmask must be 0 (none), 1 (soft) or 2 (dust)", WHO);
  if (o.hardmask != 0 && o.hardmask != 1) return fail(VSX_EINVAL, "%s: hardmask must be 0 or 1", WHO);
  if (o.want & ~(VSX_MASK_WANT_TEXT | VSX_MASK_WANT_BITS)) return fail(VSX_EINVAL, "%s: unknown bit in want", WHO);
  if (o.window < 0) return fail(VSX_EINVAL, "%s: window cannot be negative", WHO);
  // cli.cc:4274-4286 (written so that a NaN is refused too)
  if (!(o.min_unmasked_pct >= 0.0 && o.min_unmasked_pct <= 100.0)) return fail(VSX_EINVAL, "%s: min_unmasked_pct must be between 0.0 and 100.0", WHO);
  if (!(o.max_unmasked_pct >= 0.0 && o.max_unmasked_pct <= 100.0)) return fail(VSX_EINVAL, "%s: max_unmasked_pct must be between 0.0 and 100.0", WHO);
  if (o.min_unmasked_pct > o.max_unmasked_pct) return fail(VSX_EINVAL, "%s: min_unmasked_pct cannot be larger than max_unmasked_pct", WHO);
  Input in { n, blob, offsets, lengths, {} };
  if (const int rc = vsxp::check_spans(WHO, "a sequence", n, offsets, lengths, blob_bytes)) return rc;
  in.poff.assign(n + 1, 0);
  for (uint64_t k = 0; k < n; ++k)
    {
      if (lengths[k] > (uint32_t) INT32_MAX) return fail(VSX_EINVAL, "%s: a sequence is longer than INT32_MAX", WHO);
      in.poff[k + 1] = in.poff[k] + lengths[k];
    }
  if (!disjoint(n, offsets, lengths)) return fail(VSX_EINVAL, "%s: masking needs sequences that do not overlap in the blob", WHO);
  const int rc = run(ctx, o, in, host_all, *out);
  if (rc != VSX_OK) { release(out); return rc; }
  g_stats.seconds_total = now_s() - t_begin;
  return VSX_OK;
}

}  // extern "C"
