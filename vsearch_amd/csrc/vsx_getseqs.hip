// vsx_getseqs.hip -- sequence extraction by label on gfx950 (--fastx_getseqs, --fastx_getseq, --fastx_getsubseq; include/vsx_getseqs.h).
//
//   insert    one wavefront per needle, lane = byte: the polynomial hash of vsx_getseqs_internal.h (every lane multiplies its
//             byte by the power of its position, a butterfly adds), then the needle enters an open-addressing table keyed by
//             (length, hash).  The wave reads 64 slots of the probe chain at once, lane 0 claims the first empty one by
//             compare-and-swap on the slot's number and writes key and length behind it; a lost race goes on from that slot.
//             Equal needles take a slot each: a longer chain, never another verdict.  Which needle sits where depends on the
//             race and shows nowhere: the match kernel asks only whether ANY slot verifies.
//   match     one wavefront per header, 64 bytes per step.
//             whole header (LABEL / LABELS): the hash of the folded header, one probe chain walked by the whole wave, every slot
//             whose key and length agree verified lane = byte.
//             occurrences (substr, WORD / WORDS): a wave scan leaves the prefix sums F[0 .. L] in LDS, so the hash of
//             header[p, p + l) is (F[p + l] - F[p]) * B^-p.  Lane = start position p; the wave walks the distinct needle lengths
//             (ascending, so it stops at the first that no position can hold), every lane probes the table with its own
//             (p, l), verifies a slot that agrees byte for byte and, in the word modes, tests the byte before and the byte
//             behind.  The wave leaves once any lane has a confirmed occurrence.  The work is headers x bytes x distinct
//             lengths; the number of labels enters only through the table's size.
//   records   after rocPRIM's inclusive sum over the verdicts: ordinal among the same verdict, start and length of the piece.
//
// Integer code only.  The only atomics are the slot claims and the two statistics counters (sums: no order shows).
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include "vsx_getseqs_internal.h"
#include "vsx_devutil.h"

namespace {

typedef unsigned long long u64;
using vsxd::shfl64;
using vsxd::shfl_up64;
using vsxd::wave_sum;

#define GS_WAVES   4
#define GS_THREADS (64 * GS_WAVES)

// P(s) over the whole wave: every lane returns the sum
__device__ inline u64 wave_poly(const uint8_t * s, uint32_t L, uint32_t lane, uint32_t fold)
{
  const u64 step = vsx_gs_pow(VSX_GS_BASE, 64);
  u64 pw = vsx_gs_pow(VSX_GS_BASE, lane), acc = 0;
  for (uint32_t j = lane; j < L; j += 64, pw *= step) acc += (u64) (vsx_gs_fold(s[j], fold) + 1u) * pw;
  return wave_sum(acc);
}

__global__ __launch_bounds__(GS_THREADS)
void vsx_getseqs_insert_kernel(VsxGetseqsTable T)
{
  const uint32_t i = __builtin_amdgcn_readfirstlane(blockIdx.x * GS_WAVES + (threadIdx.x >> 6));
  if (i >= T.n) return;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t L = T.len[i];
  const u64 key = vsx_gs_key(wave_poly(T.blob + T.off[i], L, lane, T.fold), L, T.hash_mask);
  uint32_t cur = (uint32_t) key & T.slot_mask;
  // the table has at least 2 n slots: an empty one is always ahead
  for (;;)
    {
      const uint32_t idx = (cur + lane) & T.slot_mask;
      const uint32_t seen = __atomic_load_n(&T.slots[idx].id1, __ATOMIC_RELAXED);
      const u64 empty = (u64) __ballot(seen == 0u);
      if (!empty) { cur += 64; continue; }
      const uint32_t f = (uint32_t) (__ffsll((long long) empty) - 1);
      const uint32_t at = (cur + f) & T.slot_mask;
      uint32_t won = 0;
      if (lane == 0)
        {
          won = atomicCAS(&T.slots[at].id1, 0u, i + 1u) == 0u ? 1u : 0u;
          if (won) { T.slots[at].key = key; T.slots[at].len = L; }
        }
      if (__shfl((int) won, 0)) break;
      cur += f;
    }
}

// the bytes of header[p, p + l) against needle `id`, folded alike (one lane on its own)
__device__ inline bool lane_equal(const uint8_t * h, const uint8_t * nd, uint32_t l, uint32_t fold)
{
  for (uint32_t j = 0; j < l; ++j)
    if (vsx_gs_fold(h[j], fold) != vsx_gs_fold(nd[j], fold)) return false;
  return true;
}

template <bool EXACT>
__global__ __launch_bounds__(GS_THREADS)
void vsx_getseqs_match_kernel(VsxGetseqsMatch M)
{
  extern __shared__ u64 gs_lds[];
  const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t local = __builtin_amdgcn_readfirstlane(blockIdx.x * GS_WAVES + w);
  const bool live = local < M.count;
  const uint32_t i = M.first + (live ? local : 0u);
  const uint32_t L = live ? M.len[i] : 0u;
  const uint8_t * const s = M.blob + (live ? M.off[i] : 0ull);
  const uint32_t fold = M.T.fold;
  const VsxGetseqsSlot * const slots = M.T.slots;
  const uint32_t slot_mask = M.T.slot_mask;
  u64 probes = 0, checks = 0;
  bool found = false;

  if (EXACT)
    {
      if (!live) return;
      const u64 key = vsx_gs_key(wave_poly(s, L, lane, fold), L, M.T.hash_mask);
      probes = lane == 0 ? 1 : 0;
      for (uint32_t at = (uint32_t) key & slot_mask;; at = (at + 1) & slot_mask)
        {
          const VsxGetseqsSlot sl = slots[at];                       // wave-uniform
          if (sl.id1 == 0u) break;
          if (sl.key != key || sl.len != L) continue;
          if (lane == 0) ++checks;
          const uint8_t * const nd = M.T.blob + M.T.off[sl.id1 - 1u];
          bool differ = false;
          for (uint32_t j = lane; j < L; j += 64) differ |= vsx_gs_fold(s[j], fold) != vsx_gs_fold(nd[j], fold);
          if (!__ballot(differ)) { found = true; break; }
        }
    }
  else
    {
      u64 * const F = gs_lds + (size_t) w * M.lds_entries;
      const bool scan = live && !M.empty_needle && M.n_lengths != 0 && L != 0 && L < M.lds_entries;     // (the host sizes F for the longest header)
      if (scan)
        {
          // F[0] = 0, F[j + 1] = F[j] + (fold(s[j]) + 1) * B^j
          const u64 step = vsx_gs_pow(VSX_GS_BASE, 64);
          u64 pw = vsx_gs_pow(VSX_GS_BASE, lane), carry = 0;
          if (lane == 0) F[0] = 0;
          for (uint32_t base = 0; base < L; base += 64, pw *= step)
            {
              const uint32_t j = base + lane;
              u64 v = j < L ? (u64) (vsx_gs_fold(s[j], fold) + 1u) * pw : 0ull;
#pragma unroll
              for (int d = 1; d < 64; d <<= 1)
                {
                  const u64 up = shfl_up64(v, d);
                  if (lane >= (uint32_t) d) v += up;
                }
              v += carry;
              if (j < L) F[j + 1] = v;
              carry = shfl64(v, 63);
            }
        }
      __syncthreads();                                               // every wave of the block arrives: none has left yet
      if (!live) return;
      if (M.empty_needle) found = L != 0;
      else if (scan)
        {
          const u64 inv_step = vsx_gs_pow(M.base_inv, 64);
          u64 ipw = vsx_gs_pow(M.base_inv, lane);
          for (uint32_t base = 0; base < L && !found; base += 64, ipw *= inv_step)
            {
              const uint32_t p = base + lane;
              const u64 Fp = p < L ? F[p] : 0ull;
              bool mine = false;
              for (uint32_t d = 0; d < M.n_lengths; ++d)
                {
                  const uint32_t l = M.lengths[d];                   // wave-uniform, ascending
                  if (l > L - base) break;                           // no position of this step holds it, nor a longer one
                  if (p < L && l <= L - p)
                    {
                      const u64 key = vsx_gs_key((F[p + l] - Fp) * ipw, l, M.T.hash_mask);
                      ++probes;
                      for (uint32_t at = (uint32_t) key & slot_mask;; at = (at + 1) & slot_mask)
                        {
                          const VsxGetseqsSlot sl = slots[at];
                          if (sl.id1 == 0u) break;
                          if (sl.key != key || sl.len != l) continue;
                          ++checks;
                          if (!lane_equal(s + p, M.T.blob + M.T.off[sl.id1 - 1u], l, fold)) continue;
                          bool ok = true;
                          if (M.bound == VSX_GS_BOUND_ALNUM)
                            ok = (p == 0 || !vsx_gs_alnum(s[p - 1])) && (p + l == L || !vsx_gs_alnum(s[p + l]));
                          else if (M.bound == VSX_GS_BOUND_SEMI)
                            ok = (p == 0 || s[p - 1] == (uint8_t) ';') && (p + l == L || s[p + l] == (uint8_t) ';');
                          // equal bytes at the same place have the same neighbours: another slot cannot decide otherwise
                          mine = ok;
                          break;
                        }
                    }
                  if (__ballot(mine)) { found = true; break; }
                }
            }
        }
    }
  probes = wave_sum(probes); checks = wave_sum(checks);
  if (lane == 0)
    {
      M.verdict[i] = found ? 1u : 0u;
      if (probes) atomicAdd(&M.counters[0], probes);
      if (checks) atomicAdd(&M.counters[1], checks);
    }
}

__global__ __launch_bounds__(256)
void vsx_getseqs_records_kernel(uint32_t n, const uint32_t * __restrict__ verdict, const uint32_t * __restrict__ incl,
                                const uint32_t * __restrict__ seqlen, long long sub_start, long long sub_end, uint4 * __restrict__ rec)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t m = verdict[i], len = seqlen[i];
  uint32_t start = 0, length = len;
  if (m && sub_start > 0)
    {
      const long long a = sub_start > 1 ? sub_start : 1, e = sub_end < (long long) len ? sub_end : (long long) len;
      if (e < a) { start = 0; length = 0; }
      else { start = (uint32_t) (a - 1); length = (uint32_t) (e - a + 1); }
    }
  rec[i] = make_uint4(m, m ? incl[i] : i + 1u - incl[i], start, length);
}

}  // namespace

extern "C" hipError_t vsx_launch_getseqs_insert(VsxGetseqsTable T, hipStream_t st)
{
  if (T.n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_getseqs_insert_kernel, dim3((T.n + GS_WAVES - 1) / GS_WAVES), dim3(GS_THREADS), 0, st, T);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_getseqs_match(VsxGetseqsMatch M, hipStream_t st)
{
  if (M.count == 0) return hipSuccess;
  const dim3 grid((M.count + GS_WAVES - 1) / GS_WAVES);
  if (M.exact) hipLaunchKernelGGL(vsx_getseqs_match_kernel<true>, grid, dim3(GS_THREADS), 0, st, M);
  else
    {
      const size_t lds = (size_t) GS_WAVES * M.lds_entries * sizeof(u64);
      if (lds > 65536) return hipErrorInvalidValue;
      hipLaunchKernelGGL(vsx_getseqs_match_kernel<false>, grid, dim3(GS_THREADS), lds, st, M);
    }
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_getseqs_scan(void * temp, size_t * temp_bytes, const uint32_t * d_verdict, uint32_t * d_incl, uint32_t n, hipStream_t st)
{
  return rocprim::inclusive_scan(temp, *temp_bytes, d_verdict, d_incl, (size_t) n, rocprim::plus<uint32_t>(), st);
}

extern "C" hipError_t vsx_launch_getseqs_records(uint32_t n, const uint32_t * d_verdict, const uint32_t * d_incl, const uint32_t * d_seqlen,
                                                 int64_t subseq_start, int64_t subseq_end, uint32_t * d_rec, hipStream_t st)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_getseqs_records_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, n, d_verdict, d_incl, d_seqlen, (long long) subseq_start,
                     (long long) subseq_end, reinterpret_cast<uint4 *>(d_rec));
  return hipGetLastError();
}
