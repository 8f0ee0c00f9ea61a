// vsx_hitout.hip -- alignment rows, symbol rows and SAM MD strings of search hits (include/vsx_hitout.h).
//
// The reference turns a CIGAR and two sequences into columns per hit, serially, under its output lock (core/showalign.cpp:
// get_alignment_row, putop, get_aligment_symbol; core/results.cpp: build_sam_strings).  Here one wavefront takes one hit and walks its
// columns in blocks of 64, lane = column.
//
//   run scan   the hit's run words are taken 64 at a time, one per lane; a wave-inclusive scan of the lengths gives every run its
//              first column, query position and target position, with carries from chunk to chunk (any number of runs).  A lane finds
//              the run of its column by a six-step binary search over the chunk's first columns, read from the other lanes' registers.
//   rows       the lane forms qpos and tpos, reads the two symbols and writes qrow, trow, the symbol and the --alnout query symbol as
//              bytes at its column.  For a minus-strand hit the --alnout row reads the plus strand at qlen - 1 - qpos, complemented.
//   MD         an event is an 'M' column whose symbols differ in their 4-bit codes, or the first column of an 'I' run.  Per block: a
//              ballot of the events and of the matching columns; the number an event prints is the popcount of the matches between
//              it and the event below it (the highest set bit below the lane), or since the carry when the block has none below; a
//              wave scan of the events' byte lengths places them.  The same walk runs twice: count (one length per hit), a device
//              exclusive scan (rocPRIM), fill.
//
// Integer and byte code only; every store is a plain vector store; no atomics: the bytes do not depend on scheduling.  Every shuffle
// is executed by all 64 lanes (no shuffle stands under a divergent branch).
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include "vsx_hitout_internal.h"
#include "vsx_devutil.h"
#include "vsx_symbols.h"

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;

#define DEV __device__ __forceinline__

constexpr int WAVES_PER_BLOCK = 4;

using vsxd::lane_id;
using vsxd::wave_incl_sum;
using vsxsym::complement;
using vsxsym::map4;

// get_aligment_symbol (showalign.cpp:122-137)
DEV u32 symbol(u32 qc, u32 tc, bool n_mismatch)
{
  const u32 q = map4(qc), t = map4(tc);
  if (n_mismatch && (q == 15u || t == 15u)) return ' ';
  if (q == t && (q == 1u || q == 2u || q == 4u || q == 8u)) return '|';
  if ((q & t) != 0u) return '+';
  return ' ';
}

DEV u32 ndigits(u32 v)
{
  u32 n = 1;
  while (v >= 10u) { v /= 10u; ++n; }
  return n;
}

DEV void put_number(uint8_t * dst, u32 v, u32 nd)
{
  for (u32 k = nd; k-- > 0;) { dst[k] = (uint8_t) ('0' + v % 10u); v /= 10u; }
}

// The runs of one hit, a chunk of 64 at a time: lane i holds run next - n + i of the chunk with its first column and first positions.
struct Runs {
  const u32 * words;
  u32 nruns;
  u32 next = 0;                    // first run behind the chunk
  u32 chunk_end = 0;               // first column behind the chunk
  u32 sum_q = 0, sum_t = 0;        // query and target symbols in front of run `next`
  u32 w = 0, col = 0xFFFFFFFFu, q = 0, t = 0;   // this lane's run of the chunk (col 0xFFFFFFFF: none)

  DEV Runs(const u32 * words_, u32 nruns_) : words(words_), nruns(nruns_) {}

  DEV void load_next()
  {
    const u32 i = next + lane_id();
    const bool have = i < nruns;
    w = have ? words[i] : 0u;
    const u32 len = w >> 2, op = w & 3u;
    const u32 dq = op != 1u ? len : 0u, dt = op != 2u ? len : 0u;
    const u32 il = wave_incl_sum(len), iq = wave_incl_sum(dq), it = wave_incl_sum(dt);
    col = have ? chunk_end + (il - len) : 0xFFFFFFFFu;
    q = sum_q + (iq - dq);
    t = sum_t + (it - dt);
    chunk_end += (u32) __shfl((int) il, 63, 64);
    sum_q += (u32) __shfl((int) iq, 63, 64);
    sum_t += (u32) __shfl((int) it, 63, 64);
    next = next + 64u < nruns ? next + 64u : nruns;
  }

  // The run of column c for every lane with need set: its word, first column, first query and target position.  The columns a wave
  // asks for never descend, so a chunk that was passed is never needed again.
  DEV void find(u32 c, bool need, u32 & rw, u32 & rcol, u32 & rq, u32 & rt)
  {
    bool found = !need;
    rw = 0; rcol = 0; rq = 0; rt = 0;
    for (;;)
      {
        u32 idx = 0;
#pragma unroll
        for (u32 s = 32; s >= 1; s >>= 1)
          {
            const u32 cand = idx + s;                                       // < 64: 32 + 16 + ... + 1 = 63
            const u32 v = (u32) __shfl((int) col, (int) cand, 64);
            if (v <= c) idx = cand;
          }
        const u32 fw = (u32) __shfl((int) w, (int) idx, 64), fc = (u32) __shfl((int) col, (int) idx, 64);
        const u32 fq = (u32) __shfl((int) q, (int) idx, 64), ft = (u32) __shfl((int) t, (int) idx, 64);
        if (!found && c < chunk_end) { rw = fw; rcol = fc; rq = fq; rt = ft; found = true; }
        if (!__any(!found) || next >= nruns) break;
        load_next();
      }
  }
};

__global__ void __launch_bounds__(64 * WAVES_PER_BLOCK)
vsx_hitout_rows_kernel(const VsxHitJob * __restrict__ jobs, u32 n, const uint8_t * __restrict__ qtext, const uint8_t * __restrict__ dbtext,
                       const u32 * __restrict__ runs, uint8_t * __restrict__ rows, int n_mismatch)
{
  const u32 h = blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
  if (h >= n) return;                                                        // the whole wave leaves
  const VsxHitJob J = jobs[h];
  Runs R(runs + J.run_off, J.nruns);
  const uint8_t * __restrict__ qs = qtext + J.q_off;
  const uint8_t * __restrict__ qp = qtext + J.qp_off;
  const uint8_t * __restrict__ ts = dbtext + J.t_off;
  const u32 end = J.c0 + J.ilen;
  for (u32 b = J.c0; b < end; b += 64u)
    {
      const u32 c = b + lane_id();
      const bool need = c < end;
      u32 rw, rcol, rq, rt;
      R.find(c, need, rw, rcol, rq, rt);
      if (!need) continue;
      const u32 op = rw & 3u, off = c - rcol;
      const u32 qpos = rq + (op != 1u ? off : 0u), tpos = rt + (op != 2u ? off : 0u);
      const u32 qc = op != 1u ? qs[qpos] : (u32) '-';
      const u32 tc = op != 2u ? ts[tpos] : (u32) '-';
      const u64 i = c - J.c0;
      if (J.qrow_off != VSX_HITJOB_NO) rows[J.qrow_off + i] = (uint8_t) qc;
      if (J.trow_off != VSX_HITJOB_NO) rows[J.trow_off + i] = (uint8_t) tc;
      if (J.sym_off != VSX_HITJOB_NO)
        {
          // what --alnout shows as the query: the strand's own text, or the plus strand read backwards through the complement
          u32 ac = qc;
          if (J.minus && op != 1u) ac = complement(qp[J.qlen - 1u - qpos]);
          rows[J.sym_off + i] = (uint8_t) (op == 0u ? symbol(ac, tc, n_mismatch != 0) : (u32) ' ');
          if (J.aln_off != VSX_HITJOB_NO) rows[J.aln_off + i] = (uint8_t) ac;
        }
    }
}

// build_sam_strings (results.cpp:791-920), the MD half.  FILL = false: md_len[h] only.
template <bool FILL>
__global__ void __launch_bounds__(64 * WAVES_PER_BLOCK)
vsx_hitout_md_kernel(const VsxHitJob * __restrict__ jobs, u32 n, const uint8_t * __restrict__ qtext, const uint8_t * __restrict__ dbtext,
                     const u32 * __restrict__ runs, u32 * __restrict__ md_len, const u64 * __restrict__ md_off, uint8_t * __restrict__ md)
{
  const u32 h = blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
  if (h >= n) return;
  const VsxHitJob J = jobs[h];
  Runs R(runs + J.run_off, J.nruns);
  const uint8_t * __restrict__ qs = qtext + J.q_off;
  const uint8_t * __restrict__ ts = dbtext + J.t_off;
  uint8_t * __restrict__ dst = FILL ? md + md_off[h] : nullptr;
  const u32 lane = lane_id();
  const u64 below = (1ull << lane) - 1ull;
  u32 carry = 0;                  // matching columns since the last event
  u32 text = 0;                   // bytes of the string so far
  u32 ibase = 0;                  // where the target symbols of the latest 'I' run begin
  for (u32 b = 0; b < J.ncols; b += 64u)
    {
      const u32 c = b + lane;
      const bool need = c < J.ncols;
      u32 rw, rcol, rq, rt;
      R.find(c, need, rw, rcol, rq, rt);
      const u32 op = rw & 3u, off = c - rcol;
      const bool is_m = need && op == 0u, is_i = need && op == 1u;
      const u32 tc = (is_m || is_i) ? ts[rt + off] : 0u;
      const bool mism = is_m && map4(qs[rq + off]) != map4(tc);
      const bool ifirst = is_i && off == 0u;
      const bool ev = mism || ifirst;
      const u64 evmask = __ballot(ev), mmask = __ballot(is_m && !mism), imask = __ballot(ifirst);
      const u64 prev = evmask & below;
      u32 cnt;
      if (prev)
        {
          const u32 p = 63u - (u32) __clzll((long long) prev);
          cnt = (u32) __popcll(mmask & below & ~((2ull << p) - 1ull));
        }
      else cnt = carry + (u32) __popcll(mmask & below);
      const u32 nd = ndigits(cnt);
      const u32 len = ev ? nd + 1u + (ifirst ? (rw >> 2) : 0u) : 0u;
      const u32 incl = wave_incl_sum(len);
      const u32 at = text + (incl - len);
      const u32 sym_base = at + nd + 1u;                                      // an 'I' event: behind the number and the '^'
      // the event that owns an 'I' column which does not open its run: in this block (its lane), or the latest one before it
      const u32 owner = (u32) __shfl((int) sym_base, (int) ((is_i && rcol >= b) ? rcol - b : lane), 64);
      if (FILL)
        {
          if (ev)
            {
              put_number(dst + at, cnt, nd);
              dst[at + nd] = (uint8_t) (mism ? tc : (u32) '^');
            }
          if (is_i) dst[(rcol >= b ? owner : ibase) + off] = (uint8_t) tc;
        }
      text += (u32) __shfl((int) incl, 63, 64);
      if (evmask)
        {
          const u32 last = 63u - (u32) __clzll((long long) evmask);
          carry = (u32) __popcll(mmask & ~((2ull << last) - 1ull));
        }
      else carry += (u32) __popcll(mmask);
      const u32 li = imask ? 63u - (u32) __clzll((long long) imask) : 0u;
      const u32 nb = (u32) __shfl((int) sym_base, (int) li, 64);
      if (imask) ibase = nb;
    }
  // a final number always follows
  const u32 nd = ndigits(carry);
  if (lane == 0)
    {
      if (FILL) put_number(dst + text, carry, nd);
      else md_len[h] = text + nd;
    }
}

inline unsigned blocks_for(uint32_t n) { return (n + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK; }

}  // namespace

extern "C" hipError_t vsx_launch_hitout_rows(const VsxHitJob * d_jobs, uint32_t n, const uint8_t * d_qtext, const uint8_t * d_dbtext, const uint32_t * d_runs,
                                             uint8_t * d_rows, int n_mismatch, hipStream_t st)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_hitout_rows_kernel, dim3(blocks_for(n)), dim3(64 * WAVES_PER_BLOCK), 0, st, d_jobs, n, d_qtext, d_dbtext, d_runs, d_rows, n_mismatch);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_hitout_md_count(const VsxHitJob * d_jobs, uint32_t n, const uint8_t * d_qtext, const uint8_t * d_dbtext, const uint32_t * d_runs,
                                                 uint32_t * d_md_len, hipStream_t st)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_hitout_md_kernel<false>, dim3(blocks_for(n)), dim3(64 * WAVES_PER_BLOCK), 0, st, d_jobs, n, d_qtext, d_dbtext, d_runs, d_md_len,
                     (const u64 *) nullptr, (uint8_t *) nullptr);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_hitout_md_scan(void * temp, size_t * temp_bytes, const uint32_t * d_md_len, uint64_t * d_md_off, uint32_t n, hipStream_t st)
{
  return rocprim::exclusive_scan(temp, *temp_bytes, d_md_len, (u64 *) d_md_off, (u64) 0, (size_t) n, rocprim::plus<u64>(), st);
}

extern "C" hipError_t vsx_launch_hitout_md_fill(const VsxHitJob * d_jobs, uint32_t n, const uint8_t * d_qtext, const uint8_t * d_dbtext, const uint32_t * d_runs,
                                                const uint64_t * d_md_off, uint8_t * d_md, hipStream_t st)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_hitout_md_kernel<true>, dim3(blocks_for(n)), dim3(64 * WAVES_PER_BLOCK), 0, st, d_jobs, n, d_qtext, d_dbtext, d_runs, (u32 *) nullptr,
                     (const u64 *) d_md_off, d_md);
  return hipGetLastError();
}
