// vsx_sintax_internal.h -- what vsx_sintax.cpp (host) and vsx_sintax.hip (kernels) share: the stream of draws, the selection key
// and the kernels' entry points.  Included by those two files alone.
#ifndef VSX_SINTAX_INTERNAL_H
#define VSX_SINTAX_INTERNAL_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>
#include "../../include/vsx_sintax.h"

#if defined(__HIPCC__)
#define SX_HD __host__ __device__ __forceinline__
#else
#define SX_HD inline
#endif

#define SX_ROUNDS VSX_SINTAX_ROUNDS
#define SX_SUBSET VSX_SINTAX_SUBSET
#define SX_RANKS  VSX_SINTAX_RANKS

// ---- the query's stream (utils/random.{hpp,cpp}): SplitMix64, the substream seed, Lemire's bounded draw with rejection ----------
#define SX_GAMMA 0x9E3779B97F4A7C15ull
SX_HD uint64_t sx_mix(uint64_t z)
{
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
SX_HD uint64_t sx_next(uint64_t & state) { state += SX_GAMMA; return sx_mix(state); }
// the state a query's stream starts from
SX_HD uint64_t sx_substream(uint64_t base, uint64_t index)
{
  uint64_t s = base ^ (index * SX_GAMMA);
  return sx_next(s);
}
SX_HD uint64_t sx_mulhi(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__) && defined(SX_DEVICE_MULHI)      // (the kernels' file: it has the device headers)
  return __umul64hi(a, b);
#else
  return (uint64_t) (((unsigned __int128) a * b) >> 64);
#endif
}
// unbiased value in [0, range), range > 0
SX_HD uint64_t sx_bounded(uint64_t & state, uint64_t range)
{
  uint64_t x = sx_next(state);
  uint64_t low = x * range;
  if (low < range)
    {
      const uint64_t threshold = (0 - range) % range;               // 2^64 mod range
      while (low < threshold)
        {
          x = sx_next(state);
          low = x * range;
        }
    }
  return sx_mulhi(x, range);
}

// ---- the selection key of one (round, tile): count in the top byte, then the complement of the length (24 bits: shorter is
// larger), then the complement of the sequence number (lower is larger).  Tiles combine with a 64-bit max; 0 = nothing counted.
SX_HD uint64_t sx_key(uint32_t count, uint32_t length, uint32_t seq)
{
  return ((uint64_t) count << 56) | ((uint64_t) (~length & 0xffffffu) << 32) | (uint64_t) (~seq);
}
SX_HD uint32_t sx_key_count(uint64_t key) { return (uint32_t) (key >> 56); }
SX_HD uint32_t sx_key_seq(uint64_t key) { return ~(uint32_t) key; }

// what one query strand hands the count kernel per round: its sampled words (unused slots hold SX_NO_WORD)
#define SX_NO_WORD 0xffffffffu

// per query, as the vote kernel writes it (the host copies it into vsx_sintax_record)
struct SxVote {
  int32_t  strand, classified;
  uint32_t boot_count[2], best_count[2];
  uint32_t rank_seq[SX_RANKS], rank_count[SX_RANKS];
};

extern "C" {
// one lane per query: walks the query's stream over both strands.  wstart[2 * nq + 1]: the strands' word lists in `words`
// (strand s of query q = list 2 q + s; an absent strand is an empty list).  samples[(2 q + s) * 100 + r][32], nsample[...]
hipError_t vsx_sintax_launch_sample(uint32_t nq, const uint64_t * wstart, const uint32_t * words, const uint64_t * query_no, uint64_t seed,
                                    uint32_t * samples, uint8_t * nsample, hipStream_t st);
// one block per (query strand, tile): per round clear, count, select.  keys[((2 q + s) * 100 + r) * ntiles + tile]
hipError_t vsx_sintax_launch_count(const void * postings, const uint64_t * bucket_start, uint32_t ntiles, uint32_t nseq, const uint32_t * dblen,
                                   uint32_t nstrands, const uint32_t * samples, const uint8_t * nsample, uint64_t * keys, hipStream_t st);
// one wave per query: tiles combined, strand chosen, the nine-rank vote.  cand (or NULL): nq x 2 x 100
hipError_t vsx_sintax_launch_vote(uint32_t nq, uint32_t ntiles, const uint64_t * keys, const uint32_t * taxid, int strand_both, SxVote * out,
                                  uint32_t * cand, hipStream_t st);
}

#endif
