// vsx_cut.hip -- restriction-site cutting on gfx950 (--cut; include/vsx_cut.h).
//
//   match      a wavefront per work item (sequence, tile of blocks), lane = position of a 64-position block.  Every lane loads its
//              byte (none beyond the sequence's end: the packed neighbour is never read) and maps it to its 4-bit code.  For pattern
//              position j the ballot B_j of "pattern[j] accepts my code" is a 64-bit word; position i of the block matches when bit
//              i + j of B_j is set for every j, and bit i + j lies in this block's B_j or in the next block's.  So a block's match
//              word is  AND_j (B_j >> j | ones above)  from its own ballots and  AND_j (B_j << (64 - j) | ones below)  from the next
//              block's: P ballots per block, all in scalar registers, and one block more per tile.  Positions above L - P are cleared.
//   compact    rocPRIM's exclusive sum over the block popcounts ranks the matches; a lane per block writes the positions
//              64 * block + bit of its set bits at rank, rank + 1, ...
//   seqinfo    a lane per sequence: matches (from the ranks at its first block and at the next sequence's), the number of printed
//              forward and reverse fragments  k + 1 - [first cut at 0] - [last cut at L],  the uncut flag.
//   fragments  after three exclusive sums over the sequences: a lane per match finds its sequence (binary search over the first
//              ranks), and writes the piece that ends at its cut straight into slot base + j - [first cut at 0]; the last match of a
//              sequence also writes the tail.  The uncut kernel writes the list of sequences without a match.
//   emit       a wavefront per 64 output bytes: the piece of the first byte by binary search, the lanes walk on from there; the
//              byte is read from the mirrored position and complemented through chrmap_complement's table in LDS.
//
// Integer code only, no atomics: two calls give identical bytes.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include "vsx_cut_internal.h"
#include "vsx_symbols.h"

namespace {

typedef unsigned long long u64;
typedef uint32_t u32;

#define CUT_WAVES   4
#define CUT_THREADS (64 * CUT_WAVES)

__global__ __launch_bounds__(CUT_THREADS)
void vsx_cut_match_kernel(const uint8_t * __restrict__ text, const u64 * __restrict__ off, const u32 * __restrict__ len,
                          const u32 * __restrict__ bstart, const VsxCutItem * __restrict__ items, u32 n_items, u32 tile_blocks,
                          VsxCutPattern pat, u64 * __restrict__ bits, u32 * __restrict__ count)
{
  __shared__ uint8_t code4[256];
  code4[threadIdx.x] = (uint8_t) vsxsym::map4(threadIdx.x);      // chrmap_4bit as a 256-entry table
  __syncthreads();
  const u32 item = __builtin_amdgcn_readfirstlane(blockIdx.x * CUT_WAVES + (threadIdx.x >> 6));
  if (item >= n_items) return;
  const u32 lane = threadIdx.x & 63u;
  const u32 seq = items[item].seq, b0 = items[item].block0;
  const u32 L = len[seq], P = pat.P;
  const u64 base = off[seq];
  const u32 g0 = bstart[seq];
  const u32 nb = (L + 63u) >> 6;
  const u32 b1 = min(b0 + tile_blocks, nb);
  const long long valid = (long long) L - (long long) P + 1;          // positions 0 .. valid - 1 can hold a match
  u64 own_prev = 0;
  for (u32 b = b0; b <= b1; ++b)
    {
      u64 own = ~0ull, nxt = ~0ull;
      if (b < nb)
        {
          const u32 pos = b * 64u + lane;
          const u32 code = pos < L ? code4[text[base + pos]] : 0u;
          for (u32 j = 0; j < P; ++j)
            {
              const u64 B = (u64) __ballot((pat.code[j] & code) != 0u);
              if (j == 0) own &= B;
              else { own &= (B >> j) | (~0ull << (64u - j)); nxt &= (B << (64u - j)) | (~0ull >> j); }
            }
        }
      if (b > b0)
        {
          const long long v = valid - (long long) (b - 1u) * 64;
          const u64 mask = v >= 64 ? ~0ull : v <= 0 ? 0ull : ((1ull << v) - 1ull);
          const u64 m = own_prev & nxt & mask;
          if (lane == 0) { bits[g0 + b - 1u] = m; count[g0 + b - 1u] = (u32) __popcll(m); }
        }
      own_prev = own;
    }
}

__global__ __launch_bounds__(256)
void vsx_cut_compact_kernel(const u64 * __restrict__ bits, const u32 * __restrict__ rank, u32 n_blocks, u64 * __restrict__ pos)
{
  const u32 g = blockIdx.x * 256u + threadIdx.x;
  if (g >= n_blocks) return;
  u64 m = bits[g];
  u32 r = rank[g];
  while (m)
    {
      pos[r++] = (u64) g * 64u + (u32) (__ffsll((long long) m) - 1);
      m &= m - 1;
    }
}

__global__ __launch_bounds__(256)
void vsx_cut_seqinfo_kernel(u32 n, const u32 * __restrict__ len, const u32 * __restrict__ bstart, const u32 * __restrict__ rank,
                            const u64 * __restrict__ pos, VsxCutPattern pat, u32 * __restrict__ matches, u32 * __restrict__ nfwd,
                            u32 * __restrict__ nrev, u32 * __restrict__ uncut)
{
  const u32 k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  const u32 r0 = rank[bstart[k]], m = rank[bstart[k + 1]] - r0;
  u32 f = 0, r = 0;
  if (m)
    {
      const u64 base = (u64) bstart[k] * 64u;
      const u32 first = (u32) (pos[r0] - base), last = (u32) (pos[r0 + m - 1u] - base), L = len[k];
      f = m + 1u - (first + pat.cut_fwd == 0u ? 1u : 0u) - (last + pat.cut_fwd == L ? 1u : 0u);
      r = m + 1u - (first + pat.cut_rev == 0u ? 1u : 0u) - (last + pat.cut_rev == L ? 1u : 0u);
    }
  matches[k] = m; nfwd[k] = f; nrev[k] = r; uncut[k] = m ? 0u : 1u;
}

__device__ __forceinline__ void cut_put(VsxCutRec * rec, u64 * plen, int text, u32 slot, u32 seq, u32 start, u32 length)
{
  if (rec) { VsxCutRec v; v.seq = seq; v.seq_hi = 0u; v.start = start; v.length = length; rec[slot] = v; }
  if (plen) plen[slot] = text ? (u64) length : 0ull;
}

__global__ __launch_bounds__(256)
void vsx_cut_fragments_kernel(u32 n, u32 n_matches, const u32 * __restrict__ len, const u32 * __restrict__ bstart, const u32 * __restrict__ rank,
                              const u64 * __restrict__ pos, VsxCutPattern pat, const u32 * __restrict__ basef, const u32 * __restrict__ baser,
                              VsxCutRec * __restrict__ fwd, VsxCutRec * __restrict__ rev, u64 * __restrict__ plen, int rev_text)
{
  const u32 r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n_matches) return;
  // the sequence of match r: the last k with rank[bstart[k]] <= r (a sequence without a match shares its first rank with the next)
  u32 lo = 0, hi = n;                                                 // rank[bstart[lo]] <= r < rank[bstart[hi]] (= n_matches at n)
  while (hi - lo > 1u)
    {
      const u32 mid = lo + ((hi - lo) >> 1);
      if (rank[bstart[mid]] <= r) lo = mid; else hi = mid;
    }
  const u32 k = lo, r0 = rank[bstart[k]], m = rank[bstart[k + 1]] - r0, j = r - r0, L = len[k];
  const u64 base = (u64) bstart[k] * 64u;
  const u32 i = (u32) (pos[r] - base), first = (u32) (pos[r0] - base);
  const u32 before = j ? (u32) (pos[r - 1u] - base) : 0u;
  for (int strand = 0; strand < 2; ++strand)
    {
      VsxCutRec * const rec = strand ? rev : fwd;
      u64 * const pl = strand ? plen : nullptr;
      if (!rec && !pl) continue;
      const u32 cut = strand ? pat.cut_rev : pat.cut_fwd;
      const u32 z = first + cut == 0u ? 1u : 0u;
      const u32 slot0 = (strand ? baser[k] : basef[k]);
      const u32 c = i + cut, c_before = j ? before + cut : 0u;
      if (c > c_before) cut_put(rec, pl, rev_text, slot0 + j - z, k, c_before, c - c_before);
      if (j + 1u == m && c < L) cut_put(rec, pl, rev_text, slot0 + m - z, k, c, L - c);
    }
}

__global__ __launch_bounds__(256)
void vsx_cut_uncut_kernel(u32 n, const u32 * __restrict__ len, const u32 * __restrict__ matches, const u32 * __restrict__ baseu,
                          u32 * __restrict__ list, VsxCutRec * __restrict__ prec, u64 * __restrict__ plen, int want_text)
{
  const u32 k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n || matches[k]) return;
  const u32 slot = baseu[k];
  list[slot] = k;
  cut_put(prec, plen, want_text, slot, k, 0u, len[k]);
}

__global__ __launch_bounds__(CUT_THREADS)
void vsx_cut_emit_kernel(const uint8_t * __restrict__ text, const u64 * __restrict__ off, const VsxCutRec * __restrict__ prec,
                         const u64 * __restrict__ poff, u64 n_pieces, u64 total, uint8_t * __restrict__ out)
{
  __shared__ unsigned char comp[256];
  comp[threadIdx.x] = (unsigned char) vsxsym::complement(threadIdx.x);      // chrmap_complement as a 256-entry table
  __syncthreads();
  const u64 o0 = ((u64) blockIdx.x * CUT_WAVES + (threadIdx.x >> 6)) * 64u;        // wave-uniform
  if (o0 >= total) return;
  // the piece that holds byte o0: the last p with poff[p] <= o0 (empty pieces share their offset with the next: the last one is not empty)
  u64 lo = 0, hi = n_pieces;                                           // poff[lo] <= o0 < poff[hi] (= total at n_pieces)
  while (hi - lo > 1u)
    {
      const u64 mid = lo + ((hi - lo) >> 1);
      if (poff[mid] <= o0) lo = mid; else hi = mid;
    }
  const u64 o = o0 + (threadIdx.x & 63u);
  if (o >= total) return;
  u64 p = lo;
  while (poff[p + 1u] <= o) ++p;                                       // o < total = poff[n_pieces]: ends at the latest at n_pieces - 1
  const VsxCutRec r = prec[p];
  const u32 t = (u32) (o - poff[p]);
  out[o] = comp[text[off[r.seq] + r.start + (r.length - 1u - t)]];
}

}  // namespace

extern "C" hipError_t vsx_launch_cut_match(const uint8_t * d_text, const uint64_t * d_off, const uint32_t * d_len, const uint32_t * d_bstart,
                                           const VsxCutItem * d_items, uint32_t n_items, uint32_t tile_blocks, VsxCutPattern pat,
                                           unsigned long long * d_bits, uint32_t * d_count, hipStream_t st)
{
  if (n_items == 0) return hipSuccess;
  if (pat.P == 0 || pat.P > VSX_CUT_MAX_P || tile_blocks == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vsx_cut_match_kernel, dim3((n_items + CUT_WAVES - 1) / CUT_WAVES), dim3(CUT_THREADS), 0, st, d_text, (const u64 *) d_off, d_len,
                     d_bstart, d_items, n_items, tile_blocks, pat, d_bits, d_count);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_cut_scan32(void * temp, size_t * temp_bytes, const uint32_t * d_in, uint32_t * d_out, uint64_t count, hipStream_t st)
{
  return rocprim::exclusive_scan(temp, *temp_bytes, d_in, d_out, (uint32_t) 0, (size_t) count, rocprim::plus<uint32_t>(), st);
}

extern "C" hipError_t vsx_launch_cut_scan64(void * temp, size_t * temp_bytes, const uint64_t * d_in, uint64_t * d_out, uint64_t count, hipStream_t st)
{
  return rocprim::exclusive_scan(temp, *temp_bytes, d_in, d_out, (uint64_t) 0, (size_t) count, rocprim::plus<uint64_t>(), st);
}

extern "C" hipError_t vsx_launch_cut_compact(const unsigned long long * d_bits, const uint32_t * d_rank, uint32_t n_blocks, unsigned long long * d_pos,
                                             hipStream_t st)
{
  if (n_blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_cut_compact_kernel, dim3((n_blocks + 255u) / 256u), dim3(256), 0, st, d_bits, d_rank, n_blocks, d_pos);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_cut_seqinfo(uint32_t n, const uint32_t * d_len, const uint32_t * d_bstart, const uint32_t * d_rank,
                                             const unsigned long long * d_pos, VsxCutPattern pat, uint32_t * d_matches, uint32_t * d_nfwd,
                                             uint32_t * d_nrev, uint32_t * d_uncut, hipStream_t st)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_cut_seqinfo_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, n, d_len, d_bstart, d_rank, d_pos, pat, d_matches, d_nfwd,
                     d_nrev, d_uncut);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_cut_fragments(uint32_t n, uint32_t n_matches, const uint32_t * d_len, const uint32_t * d_bstart, const uint32_t * d_rank,
                                               const unsigned long long * d_pos, VsxCutPattern pat, const uint32_t * d_basef, const uint32_t * d_baser,
                                               VsxCutRec * d_fwd, VsxCutRec * d_rev, unsigned long long * d_plen, int rev_text, hipStream_t st)
{
  if (n_matches == 0 || n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_cut_fragments_kernel, dim3((n_matches + 255u) / 256u), dim3(256), 0, st, n, n_matches, d_len, d_bstart, d_rank, d_pos, pat,
                     d_basef, d_baser, d_fwd, d_rev, d_plen, rev_text);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_cut_uncut(uint32_t n, const uint32_t * d_len, const uint32_t * d_matches, const uint32_t * d_baseu, uint32_t * d_list,
                                           VsxCutRec * d_prec, unsigned long long * d_plen, int want_text, hipStream_t st)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_cut_uncut_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, n, d_len, d_matches, d_baseu, d_list, d_prec, d_plen, want_text);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_cut_emit(const uint8_t * d_text, const uint64_t * d_off, const VsxCutRec * d_prec, const unsigned long long * d_poff,
                                          uint64_t n_pieces, uint64_t total_bytes, uint8_t * d_out, hipStream_t st)
{
  if (total_bytes == 0 || n_pieces == 0) return hipSuccess;
  const uint64_t waves = (total_bytes + 63u) / 64u;
  const uint64_t blocks = (waves + CUT_WAVES - 1) / CUT_WAVES;
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vsx_cut_emit_kernel, dim3((uint32_t) blocks), dim3(CUT_THREADS), 0, st, d_text, (const u64 *) d_off, d_prec, d_poff,
                     (u64) n_pieces, (u64) total_bytes, d_out);
  return hipGetLastError();
}
