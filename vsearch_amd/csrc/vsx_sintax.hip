// vsx_sintax.hip -- the three kernels of SINTAX classification on gfx950 (include/vsx_sintax.h; host side: vsx_sintax.cpp).
//
//   sample  one lane per query walks the query's SplitMix64 stream through both strands: 100 rounds of 32 bounded draws into the
//           strand's word list (first-occurrence order, from the host), repeated indices dropped.  The 32 draws of a round stay
//           in registers (both loops unrolled), so the repeat test needs no memory.  Out: per (strand, round) the sampled words.
//   count   one block per (query strand, tile) on the packed postings of the search index (vsx_kmer.hip, read through
//           VsxKmerView; neither the format nor its kernels change).  The tile's 8-bit counters live in LDS (32 KB, 512 threads,
//           four blocks per CU).  Per round: wave w streams the buckets of words 4 w .. 4 w + 3 (ranges loaded one round ahead by
//           lanes 0 .. 3 and broadcast with v_readlane: no LDS read between the ds_add_u32 of the stream); then every thread reads
//           its own 16 counter dwords, the block agrees on the largest count, the threads that hold it read theirs once more and
//           build the 64-bit key (count, ~length, ~sequence number; vsx_sintax_internal.h) of each such sequence, and every thread
//           zeroes its own dwords for the next round (holding the 16 dwords in registers across the barrier spilled: 64 VGPRs at
//           eight waves per SIMD).  One key per (round, tile) goes out -- 8 bytes where the record form of the search kernels
//           would return every sequence tied at the top, and reference sets are full of near-identical sequences.
//           No global atomic at all: the tiles' keys are combined by the vote kernel, so runs repeat bit for bit.
//           The dummies of the packed format (every 252nd counter: the top byte of dword 62 mod 63) are masked as they are read;
//           which of a thread's 16 dwords hold one never changes, so that is a 16-bit mask computed once.
//   vote    one wave per query: max over the tiles per round, the kept rounds compacted in round order into the strand's candidate
//           list (ballot prefix), strand choice, then the nine ranks: a candidate counts the still included candidates that
//           share its name id and finds the first of them; the first-in-order candidate of the largest group wins and the
//           others leave.  <= 100 candidates, two per lane.
#include <hip/hip_runtime.h>
#define SX_DEVICE_MULHI 1
#include "vsx_sintax_internal.h"
#include "vsx_kmer_pack.h"
#include "vsx_devutil.h"

typedef unsigned int u32;
typedef unsigned long long u64;
using vsxd::wave_max;

#define SX_THREADS 512
#define SX_WAVES 8
#define SX_NDW 8192                      // dwords of 8-bit counters of a tile (32 768 counters >= 130 * 252)
#define SX_DW_PER_THREAD (SX_NDW / SX_THREADS)

__global__ void __launch_bounds__(64)
vsx_sintax_sample_kernel(u32 nq, const u64 * __restrict__ wstart, const u32 * __restrict__ words, const u64 * __restrict__ query_no, u64 seed,
                         u32 * __restrict__ samples, uint8_t * __restrict__ nsample)
{
  const u32 q = blockIdx.x * 64u + threadIdx.x;
  if (q >= nq) return;
  uint64_t state = sx_substream(seed, query_no[q]);
  for (u32 s = 0; s < 2; ++s)
    {
      const size_t list = (size_t) q * 2 + s;
      const u64 k0 = wstart[list], K = wstart[list + 1] - k0;
      u32 * __restrict__ out = samples + list * (SX_ROUNDS * SX_SUBSET);
      uint8_t * __restrict__ nout = nsample + list * SX_ROUNDS;
      if (K < SX_SUBSET)                                             // skipped: no draws
        {
          for (int r = 0; r < SX_ROUNDS; ++r) nout[r] = 0;
          continue;
        }
      for (int r = 0; r < SX_ROUNDS; ++r)
        {
          u32 taken[SX_SUBSET];
          u32 n = 0;
#pragma unroll
          for (int j = 0; j < SX_SUBSET; ++j)
            {
              const u32 x = (u32) sx_bounded(state, K);
              bool dup = false;
#pragma unroll
              for (int i = 0; i < j; ++i) dup = dup || (taken[i] == x);
              taken[j] = dup ? 0xffffffffu : x;                      // (an index is below K < 2^32)
              if (!dup) { out[r * SX_SUBSET + (int) n] = words[k0 + x]; ++n; }
            }
          for (u32 i = n; i < SX_SUBSET; ++i) out[r * SX_SUBSET + (int) i] = SX_NO_WORD;
          nout[r] = (uint8_t) n;
        }
    }
}

__global__ void __launch_bounds__(SX_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8)))
vsx_sintax_count_kernel(const uint4 * __restrict__ postings, const u64 * __restrict__ bucket_start, u32 ntiles, u32 nseq,
                        const u32 * __restrict__ dblen, const u32 * __restrict__ samples, const uint8_t * __restrict__ nsample,
                        u64 * __restrict__ keys)
{
  __shared__ __attribute__((aligned(16))) u32 cnt[SX_NDW];
  __shared__ u32 wave_top[SX_WAVES];
  __shared__ u64 wave_key[SX_WAVES];
  const int tid = (int) threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t list = blockIdx.x;
  const u32 tile = blockIdx.y;
  u64 * __restrict__ kout = keys + list * SX_ROUNDS * ntiles + tile;           // round r: kout[r * ntiles]
  if (nsample[list * SX_ROUNDS] == 0)                                          // a skipped strand (every round is empty)
    {
      if (tid < SX_ROUNDS) kout[(size_t) tid * ntiles] = 0;
      return;
    }
  {
    uint4 * c4 = reinterpret_cast<uint4 *>(cnt);
    for (int x = tid; x < SX_NDW / 4; x += SX_THREADS) c4[x] = make_uint4(0, 0, 0, 0);
  }
  // which of this thread's 16 dwords (uint4 g4 * 512 + tid, dword j) carry a dummy in their top byte
  u32 dummy = 0;
#pragma unroll
  for (int i = 0; i < SX_DW_PER_THREAD; ++i)
    {
      const u32 dw = (u32) ((i >> 2) * SX_THREADS + tid) * 4u + (u32) (i & 3);
      if (dw % 63u == 62u) dummy |= 1u << i;
    }
  const u32 * __restrict__ smp = samples + list * (SX_ROUNDS * SX_SUBSET);
  const u32 seq0 = tile * KM_PK_TILE_SEQS;
  // lanes 0 .. 3 of wave w: the bucket of the round's word 4 w + lane in this tile, as (first unit, units)
  auto range_of = [&](int r) -> uint2 {
    uint2 g = make_uint2(0u, 0u);
    if (lane < 4 && r < SX_ROUNDS)
      {
        const u32 word = smp[r * SX_SUBSET + wave * 4 + lane];
        if (word != SX_NO_WORD)
          {
            const size_t b = (size_t) word * ntiles + tile;
            const u64 first = bucket_start[b];
            g = make_uint2((u32) first, (u32) (bucket_start[b + 1] - first));
          }
      }
    return g;
  };
  auto bump = [&](u32 x) __attribute__((always_inline)) { atomicAdd(&cnt[x >> 2], 1u << ((x & 3u) << 3)); };
  auto consume = [&](const uint4 & v) __attribute__((always_inline)) {
    u32 acc = v.x & 0xffffu;
    bump(acc);
    acc += (v.x >> 16) & 0xffu; bump(acc);
    acc += v.x >> 24; bump(acc);
    const u32 d3[3] = {v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 3; ++e)
#pragma unroll
      for (int b = 0; b < 4; ++b)
        {
          acc += (d3[e] >> (8 * b)) & 0xffu;
          bump(acc);
        }
  };
  uint2 nxt = range_of(0);
  __syncthreads();                                                             // counters cleared
#pragma unroll 1
  for (int r = 0; r < SX_ROUNDS; ++r)
    {
      const uint2 mine = nxt;
      nxt = range_of(r + 1);
      // ---- stream: the first 64 units of the wave's four buckets in flight together, longer buckets finish in a tail loop
      uint4 v4[4];
      bool on[4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        {
          const u32 n = (u32) __builtin_amdgcn_readlane((int) mine.y, u);
          const u32 r0 = (u32) __builtin_amdgcn_readlane((int) mine.x, u);
          on[u] = (u32) lane < n;
          if (on[u]) v4[u] = postings[r0 + (u32) lane];
        }
#pragma unroll
      for (int u = 0; u < 4; ++u) if (on[u]) consume(v4[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        {
          const u32 n = (u32) __builtin_amdgcn_readlane((int) mine.y, u);
          if (n > 64u)
            {
              const u32 r0 = (u32) __builtin_amdgcn_readlane((int) mine.x, u);
              for (u32 i = 64u + (u32) lane; i < n; i += 64u) consume(postings[r0 + i]);
            }
        }
      __syncthreads();
      // ---- the largest count of the tile.  A thread reads its own 16 counter dwords (dummies masked) here and, where it holds
      // the largest count, once more below; nobody else reads them, so it zeroes them for the next round right after
      uint4 * c4 = reinterpret_cast<uint4 *>(cnt);
      auto own = [&](int g4) __attribute__((always_inline)) -> uint4 {
        uint4 t = c4[g4 * SX_THREADS + tid];
        const u32 dm = dummy >> (4 * g4);
        if (dm & 1u) t.x &= 0x00ffffffu;
        if (dm & 2u) t.y &= 0x00ffffffu;
        if (dm & 4u) t.z &= 0x00ffffffu;
        if (dm & 8u) t.w &= 0x00ffffffu;
        return t;
      };
      u32 mytop = 0;
#pragma unroll
      for (int g4 = 0; g4 < SX_DW_PER_THREAD / 4; ++g4)
        {
          const uint4 t = own(g4);
          if (t.x | t.y | t.z | t.w)
            {
              const u32 d4[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
              for (int j = 0; j < 4; ++j)
                {
                  const u32 v = d4[j];
                  const u32 a = v & 0xffu, b = (v >> 8) & 0xffu, c = (v >> 16) & 0xffu, d = v >> 24;
                  const u32 m1 = a > b ? a : b, m2 = c > d ? c : d;
                  const u32 m = m1 > m2 ? m1 : m2;
                  mytop = m > mytop ? m : mytop;
                }
            }
        }
      const u32 top = wave_max(mytop);
      if (lane == 0) wave_top[wave] = top;
      __syncthreads();
      u32 cmax = 0;
#pragma unroll
      for (int w2 = 0; w2 < SX_WAVES; ++w2) { const u32 t = wave_top[w2]; cmax = t > cmax ? t : cmax; }
      // ---- the best sequence among those at the largest count (a round whose winner counts <= 1 is dropped anyway)
      u64 best = 0;
      if (cmax > 1u && mytop == cmax)
        {
          const u32 pattern = cmax * 0x01010101u;
#pragma unroll 1
          for (int i = 0; i < SX_DW_PER_THREAD; ++i)
            {
              const u32 dw = (u32) ((i >> 2) * SX_THREADS + tid) * 4u + (u32) (i & 3);
              u32 v = cnt[dw];
              if ((dummy >> i) & 1u) v &= 0x00ffffffu;
              const u32 z = v ^ pattern;                               // a zero byte where the counter equals cmax
              if (((z - 0x01010101u) & ~z & 0x80808080u) == 0u) continue;
#pragma unroll 1
              for (u32 h = 0; h < 4; ++h)
                if (((v >> (8 * h)) & 0xffu) == cmax)
                  {
                    const u32 x = dw * 4u + h;
                    const u32 seq = seq0 + km_pk_seq_of(x);
                    if (x < KM_PK_ROWS * KM_PK_PERIOD && seq < nseq)
                      {
                        const u64 k = sx_key(cmax, dblen[seq], seq);
                        best = k > best ? k : best;
                      }
                  }
            }
        }
#pragma unroll
      for (int g4 = 0; g4 < SX_DW_PER_THREAD / 4; ++g4) c4[g4 * SX_THREADS + tid] = make_uint4(0, 0, 0, 0);
      if (cmax > 1u)
        {
          best = wave_max(best);
          if (lane == 0) wave_key[wave] = best;
        }
      __syncthreads();
      if (tid == 0)
        {
          u64 k = 0;
          if (cmax > 1u)
            {
#pragma unroll
              for (int w2 = 0; w2 < SX_WAVES; ++w2) { const u64 t = wave_key[w2]; k = t > k ? t : k; }
            }
          kout[(size_t) r * ntiles] = k;
        }
    }
}

__global__ void __launch_bounds__(64)
vsx_sintax_vote_kernel(u32 nq, u32 ntiles, const u64 * __restrict__ keys, const u32 * __restrict__ taxid, int strand_both,
                       SxVote * __restrict__ out, u32 * __restrict__ cand_out)
{
  __shared__ u32 cand[2][SX_ROUNDS];
  __shared__ u32 ids[SX_ROUNDS];
  __shared__ u32 incl[SX_ROUNDS];
  const u32 q = blockIdx.x;
  const int lane = (int) threadIdx.x;
  if (q >= nq) return;
  u32 boot[2] = {0u, 0u}, bestc[2] = {0u, 0u};
  const u64 below = (1ull << lane) - 1ull;
  for (int s = 0; s < (strand_both ? 2 : 1); ++s)
    {
      const u64 * __restrict__ kin = keys + ((size_t) q * 2 + (size_t) s) * SX_ROUNDS * ntiles;
      u32 n = 0, bc = 0;
      for (int half = 0; half < 2; ++half)
        {
          const int r = half * 64 + lane;
          u64 key = 0;
          if (r < SX_ROUNDS)
            for (u32 t = 0; t < ntiles; ++t) { const u64 k = kin[(size_t) r * ntiles + t]; key = k > key ? k : key; }
          const u32 c = sx_key_count(key);
          const bool kept = c > 1u;
          const u64 ballot = __ballot(kept);
          if (kept) cand[s][n + (u32) __popcll(ballot & below)] = sx_key_seq(key);
          n += (u32) __popcll(ballot);
          const u32 m = wave_max(kept ? c : 0u);
          bc = m > bc ? m : bc;
        }
      boot[s] = n;
      bestc[s] = bc;
    }
  int strand = 0;
  if (strand_both)
    {
      if (bestc[0] > bestc[1]) strand = 0;
      else if (bestc[1] > bestc[0]) strand = 1;
      else strand = boot[0] >= boot[1] ? 0 : 1;
    }
  const u32 count = boot[strand];
  const bool classified = count >= (SX_ROUNDS + 1) / 2;
  __syncthreads();
  SxVote * __restrict__ o = out + q;
  if (lane == 0)
    {
      o->strand = strand; o->classified = classified ? 1 : 0;
      o->boot_count[0] = boot[0]; o->boot_count[1] = boot[1];
      o->best_count[0] = bestc[0]; o->best_count[1] = bestc[1];
    }
  if (cand_out)
    for (int x = lane; x < 2 * SX_ROUNDS; x += 64)
      {
        const int s = x / SX_ROUNDS, i = x % SX_ROUNDS;
        cand_out[(size_t) q * 2 * SX_ROUNDS + x] = ((u32) i < boot[s]) ? cand[s][i] : VSX_SINTAX_NONE;
      }
  if (!classified)
    {
      if (lane < SX_RANKS) { o->rank_seq[lane] = VSX_SINTAX_NONE; o->rank_count[lane] = 0; }
      return;
    }
  const u32 * cs = cand[strand];
  for (int i = lane; i < SX_ROUNDS; i += 64) incl[i] = ((u32) i < count) ? 1u : 0u;
  for (int k = 0; k < SX_RANKS; ++k)
    {
      for (u32 i = (u32) lane; i < count; i += 64) ids[i] = taxid[(size_t) cs[i] * SX_RANKS + (size_t) k];
      __syncthreads();
      u32 vote = 0;                                                  // group size << 7 | 127 - index, for the first of a group
      for (u32 i = (u32) lane; i < count; i += 64)
        if (incl[i])
          {
            const u32 id = ids[i];
            u32 members = 0, first = i;
            for (u32 j = 0; j < count; ++j)
              if (incl[j] && ids[j] == id) { ++members; first = j < first ? j : first; }
            if (first == i)
              {
                const u32 v = (members << 7) | (127u - i);
                vote = v > vote ? v : vote;
              }
          }
      vote = wave_max(vote);
      const u32 winner = vote ? 127u - (vote & 127u) : 0u;           // (candidate 0's group always votes)
      const u32 wid = ids[winner];
      __syncthreads();
      for (u32 i = (u32) lane; i < count; i += 64) if (ids[i] != wid) incl[i] = 0u;
      if (lane == 0) { o->rank_seq[k] = cs[winner]; o->rank_count[k] = vote >> 7; }
      __syncthreads();
    }
}

extern "C" hipError_t vsx_sintax_launch_sample(uint32_t nq, const uint64_t * wstart, const uint32_t * words, const uint64_t * query_no,
                                               uint64_t seed, uint32_t * samples, uint8_t * nsample, hipStream_t st)
{
  if (nq == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_sintax_sample_kernel, dim3((nq + 63) / 64), dim3(64), 0, st, nq, (const u64 *) wstart, words, (const u64 *) query_no,
                     (u64) seed, samples, nsample);
  return hipGetLastError();
}

extern "C" hipError_t vsx_sintax_launch_count(const void * postings, const uint64_t * bucket_start, uint32_t ntiles, uint32_t nseq,
                                              const uint32_t * dblen, uint32_t nstrands, const uint32_t * samples, const uint8_t * nsample,
                                              uint64_t * keys, hipStream_t st)
{
  if (nstrands == 0 || ntiles == 0) return hipSuccess;
  if (ntiles > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vsx_sintax_count_kernel, dim3(nstrands, ntiles), dim3(SX_THREADS), 0, st, (const uint4 *) postings, (const u64 *) bucket_start,
                     ntiles, nseq, dblen, samples, nsample, (u64 *) keys);
  return hipGetLastError();
}

extern "C" hipError_t vsx_sintax_launch_vote(uint32_t nq, uint32_t ntiles, const uint64_t * keys, const uint32_t * taxid, int strand_both,
                                             SxVote * out, uint32_t * cand, hipStream_t st)
{
  if (nq == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_sintax_vote_kernel, dim3(nq), dim3(64), 0, st, nq, ntiles, (const u64 *) keys, taxid, strand_both, out, cand);
  return hipGetLastError();
}
