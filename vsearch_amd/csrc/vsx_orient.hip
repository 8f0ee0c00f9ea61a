// vsx_orient.hip -- the kernels of sequence orientation on gfx950 (include/vsx_orient.h; host side: vsx_orient.cpp).
//
//   build   the match-count table mc[4^w] (uint32, w <= 12): how many database sequences contain each word.  The database is read
//           through the searcher's sequence set (4-bit codes, one per byte) and its case bitmap.  Per chunk of consecutive
//           sequences: every position's 64-bit key (chunk-local sequence << 2 w | word; positions without a valid word get the
//           sequence number one past the chunk) -> rocPRIM radix sort of the bits in use -> the first key of each run of equal
//           keys is one distinct (word, sequence) pair and adds one to mc[word].  One method for every word length 3 .. 12.
//           Integer atomics only: two builds give the same table.
//   count   one wavefront (queries of <= 512 symbols) or one block (<= 4 096: 256 threads, <= 16 384: 1 024 threads) per query.
//           A lane forms the word at each of its positions from the query's text as given (U = T; an ambiguous symbol, and under
//           soft masking a lower-case one, poisons the words over it) and claims it in the query's distinct-word set in LDS: open
//           addressing, linear probing, slots claimed with an LDS compare-and-swap on OR_EMPTY.  The lane that newly claims a
//           word gathers mc[word] and mc[rc(word)] (rc = complement, bit reversal, pair swap, shift) and applies the reference's
//           two 32-bit comparisons.  Counts are reduced across the wave (and through LDS across a block's waves); one lane writes
//           the record.  A set has twice as many slots as the class's longest query has symbols: never more than half full.
//   emit    one wavefront per read: copies the text, or reverse-complements it through a 256-entry table (chrmap_complement:
//           IUPAC, case kept) in LDS, and reverses the qualities of a - read.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <rocprim/device/device_radix_sort.hpp>
#include "vsx_orient_internal.h"
#include "vsx_devutil.h"
#include "vsx_symbols.h"

typedef unsigned int u32;
typedef unsigned long long u64;
using vsxd::wave_sum;

// ---- build -------------------------------------------------------------------------------------------------------------------
// the word of w symbols at s[p ..]; false where a symbol is ambiguous or (lower != NULL) masked.  i = the blob byte of s[p].
__device__ __forceinline__ bool or_db_word(const uint8_t * __restrict__ s, int w, const uint8_t * __restrict__ lower, u64 i, u32 & word)
{
  u32 v = 0;
  bool ok = true;
  for (int x = 0; x < w; ++x)
    {
      const u32 c = s[x];
      ok = ok && (c == 1u || c == 2u || c == 4u || c == 8u);
      v = (v << 2) | ((c >> 1) - (c >> 3));
    }
  word = v;
  if (lower)
    {
      // bits i .. i + w - 1 of the bitmap: the bytes that hold them and no other (w <= 12: at most three)
      const uint8_t * __restrict__ b = lower + (i >> 3);
      const u32 sh = (u32) (i & 7), nb = (sh + (u32) w + 7u) >> 3;
      u32 bits = b[0];
      if (nb > 1) bits |= (u32) b[1] << 8;
      if (nb > 2) bits |= (u32) b[2] << 16;
      ok = ok && (((bits >> sh) & ((1u << w) - 1u)) == 0u);
    }
  return ok;
}

// blockIdx.x = chunk-local sequence, blockIdx.y = one of gridDim.y interleaved position strides
__global__ void __launch_bounds__(256)
vsx_orient_keys_kernel(const uint8_t * __restrict__ codes, const u64 * __restrict__ off, const u32 * __restrict__ len,
                       const uint8_t * __restrict__ lower, const u64 * __restrict__ slot_of, u32 first_seq, u32 nseq, int w,
                       u64 * __restrict__ keys)
{
  const u32 local = blockIdx.x;
  if (local >= nseq) return;
  const u32 sid = first_seq + local;
  const u64 base = off[sid];
  const u32 L = len[sid];
  const uint8_t * __restrict__ s = codes + base;
  u64 * __restrict__ out = keys + (slot_of[sid] - slot_of[first_seq]);
  const u64 none = (u64) nseq << (2 * w);
  for (u64 p = (u64) blockIdx.y * 256u + threadIdx.x; p < L; p += (u64) gridDim.y * 256u)
    {
      u32 word = 0;
      u64 key = none;
      if (p + (u64) w <= L && or_db_word(s + p, w, lower, base + p, word)) key = ((u64) local << (2 * w)) | word;
      out[p] = key;
    }
}

__global__ void __launch_bounds__(256)
vsx_orient_runs_kernel(const u64 * __restrict__ keys, u64 n, u32 nseq, int w, u32 * __restrict__ mc)
{
  const u64 i = (u64) blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const u64 k = keys[i];
  if ((k >> (2 * w)) >= nseq) return;                                 // no valid word at that position
  if (i > 0 && keys[i - 1] == k) return;                              // a repeat of the word inside its sequence
  atomicAdd(&mc[(u32) (k & ((1ull << (2 * w)) - 1ull))], 1u);
}

// ---- count -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u32 or_rc(u32 word, int w)
{
  u32 x = __brev(~word);                                              // symbols reversed and complemented, the bits of each pair swapped
  x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
  return x >> (32 - 2 * w);
}

// TPQ threads per query (64: a wave of the block per query; else the whole block), SLOTS per set
template <int TPQ, int SLOTS>
__global__ void __launch_bounds__(TPQ < 256 ? 256 : TPQ)
vsx_orient_count_kernel(u32 nq, const u32 * __restrict__ list, const char * __restrict__ text, const u64 * __restrict__ qoff,
                        const u32 * __restrict__ qlen, int w, int soft, u32 hash_mask, const u32 * __restrict__ mc, OrRec * __restrict__ rec)
{
  extern __shared__ __attribute__((aligned(16))) u32 or_lds[];
  constexpr int BLOCK = TPQ < 256 ? 256 : TPQ;
  constexpr int QPB = BLOCK / TPQ;                                   // queries per block
  constexpr u32 SLOT_MASK = (u32) SLOTS - 1u;
  const int tid = (int) threadIdx.x;
  const int sub = tid / TPQ, t = tid % TPQ;
  const u32 qi = blockIdx.x * (u32) QPB + (u32) sub;
  const bool live = qi < nq;                                           // (uniform per wave; per block where TPQ >= 256)
  u32 * __restrict__ set = or_lds + (size_t) sub * SLOTS;
  u32 * __restrict__ sums = or_lds + (size_t) QPB * SLOTS;             // TPQ > 64: count_fwd, count_rev, distinct of the block's query
  for (int x = t; x < SLOTS; x += TPQ) set[x] = OR_EMPTY;
  if (TPQ > 64)
    {
      if (tid < 3) sums[tid] = 0;
      __syncthreads();
    }
  u32 nf = 0, nr = 0, nd = 0;
  u32 slot_q = 0;
  if (live)
    {
      slot_q = list[qi];
      const char * __restrict__ s = text + qoff[slot_q];
      const int L = (int) qlen[slot_q];
      const u32 wmask = (w < 16) ? ((1u << (2 * w)) - 1u) : 0xffffffffu;
      for (int p = t; p + w <= L; p += TPQ)
        {
          u32 word = 0;
          bool ok = true;
          for (int x = 0; x < w; ++x)
            {
              const u32 c = (unsigned char) s[p + x];
              const u32 lc = c | 0x20u;
              const u32 code = lc == 'a' ? 0u : lc == 'c' ? 1u : lc == 'g' ? 2u : (lc == 't' || lc == 'u') ? 3u : 4u;
              // only ACGTU of either case are symbols (c | 0x20 maps no other byte onto those letters); soft: upper case only
              ok = ok && code < 4u && !(soft && c == lc);
              word = (word << 2) | (code & 3u);
            }
          if (!ok) continue;
          word &= wmask;
          u32 slot = ((word * 0x9E3779B1u) >> (32 - __builtin_ctz((u32) SLOTS))) & hash_mask;
          bool fresh = false;
          for (;;)
            {
              const u32 old = atomicCAS(&set[slot], OR_EMPTY, word);
              if (old == OR_EMPTY) { fresh = true; break; }
              if (old == word) break;
              slot = (slot + 1u) & SLOT_MASK;
            }
          if (fresh)
            {
              const u32 hf = mc[word], hr = mc[or_rc(word, w)];
              ++nd;
              if (hf > 8u * hr) ++nf;
              else if (hr > 8u * hf) ++nr;
            }
        }
    }
  nf = wave_sum(nf); nr = wave_sum(nr); nd = wave_sum(nd);
  if (TPQ > 64)
    {
      if ((tid & 63) == 0) { atomicAdd(&sums[0], nf); atomicAdd(&sums[1], nr); atomicAdd(&sums[2], nd); }
      __syncthreads();
      nf = sums[0]; nr = sums[1]; nd = sums[2];
    }
  if (live && t == 0)
    {
      int strand = 2;
      if (nf >= 1u && nf >= 4u * nr) strand = 0;
      else if (nr >= 1u && nr >= 4u * nf) strand = 1;
      OrRec o;
      o.count_fwd = nf; o.count_rev = nr; o.strand = strand; o.distinct = nd;
      rec[slot_q] = o;
    }
}

// ---- emit --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
vsx_orient_emit_kernel(u32 nq, const char * __restrict__ text, const char * __restrict__ qual, const u64 * __restrict__ qoff,
                       const u32 * __restrict__ qlen, const OrRec * __restrict__ rec, char * __restrict__ out_text, char * __restrict__ out_qual)
{
  __shared__ unsigned char comp[256];
  comp[threadIdx.x] = (unsigned char) vsxsym::complement(threadIdx.x);      // chrmap_complement as a 256-entry table
  __syncthreads();
  const u32 q = blockIdx.x * 4u + (threadIdx.x >> 6);
  const u32 lane = threadIdx.x & 63u;
  if (q >= nq) return;
  const u64 base = qoff[q];
  const u32 L = qlen[q];
  const bool minus = rec[q].strand == 1;
  for (u32 p = lane; p < L; p += 64u)
    {
      const u32 src = minus ? L - 1u - p : p;
      const unsigned char c = (unsigned char) text[base + src];
      out_text[base + p] = (char) (minus ? comp[c] : c);
      if (qual) out_qual[base + p] = qual[base + src];
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
extern "C" hipError_t vsx_orient_launch_keys(const uint8_t * codes, const uint64_t * off, const uint32_t * len, const uint8_t * lower_bits,
                                             const uint64_t * slot_of, uint32_t first_seq, uint32_t nseq, uint32_t maxlen, int w,
                                             uint64_t * keys, hipStream_t st)
{
  if (nseq == 0 || maxlen == 0) return hipSuccess;
  if (w < 3 || w > VSX_ORIENT_MAX_DEVICE_WORDLENGTH) return hipErrorInvalidValue;
  const u32 strides = (u32) std::min<u64>(64u, ((u64) maxlen + 2047u) / 2048u);
  hipLaunchKernelGGL(vsx_orient_keys_kernel, dim3(nseq, strides), dim3(256), 0, st, codes, (const u64 *) off, len, lower_bits,
                     (const u64 *) slot_of, first_seq, nseq, w, (u64 *) keys);
  return hipGetLastError();
}

extern "C" hipError_t vsx_orient_sort_keys(void * temp, size_t * temp_bytes, uint64_t * keys_in, uint64_t * keys_out, uint64_t n,
                                           unsigned end_bit, hipStream_t st)
{
  return rocprim::radix_sort_keys(temp, *temp_bytes, (u64 *) keys_in, (u64 *) keys_out, (size_t) n, 0u, end_bit, st);
}

extern "C" hipError_t vsx_orient_launch_runs(const uint64_t * keys, uint64_t n, uint32_t nseq, int w, uint32_t * mc, hipStream_t st)
{
  if (n == 0) return hipSuccess;
  if (w < 3 || w > VSX_ORIENT_MAX_DEVICE_WORDLENGTH) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vsx_orient_runs_kernel, dim3((unsigned) ((n + 255u) / 256u)), dim3(256), 0, st, (const u64 *) keys, (u64) n, nseq, w, mc);
  return hipGetLastError();
}

template <int TPQ, int SLOTS>
static hipError_t or_launch_count(uint32_t nq, const uint32_t * list, const char * text, const uint64_t * qoff, const uint32_t * qlen, int w,
                                  int soft, u32 hash_mask, const uint32_t * mc, OrRec * rec, hipStream_t st)
{
  constexpr int BLOCK = TPQ < 256 ? 256 : TPQ;
  constexpr int QPB = BLOCK / TPQ;
  constexpr size_t lds = ((size_t) QPB * SLOTS + 4) * sizeof(u32);
  if (lds > 64u * 1024u)
    {
      // (per call: the attribute belongs to the device's copy of the kernel, and a process may use several devices)
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&vsx_orient_count_kernel<TPQ, SLOTS>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
      if (e != hipSuccess) return e;
    }
  hipLaunchKernelGGL((vsx_orient_count_kernel<TPQ, SLOTS>), dim3((nq + QPB - 1) / QPB), dim3(BLOCK), lds, st, nq, list, text, (const u64 *) qoff,
                     qlen, w, soft, hash_mask, mc, rec);
  return hipGetLastError();
}

extern "C" hipError_t vsx_orient_launch_count(int cls, uint32_t nq, const uint32_t * list, const char * text, const uint64_t * qoff,
                                              const uint32_t * qlen, int w, int soft, int hash_bits, const uint32_t * mc, OrRec * rec,
                                              hipStream_t st)
{
  if (nq == 0) return hipSuccess;
  if (w < 3 || w > VSX_ORIENT_MAX_DEVICE_WORDLENGTH) return hipErrorInvalidValue;
  const u32 hash_mask = (hash_bits > 0 && hash_bits < 32) ? ((1u << hash_bits) - 1u) : 0xffffffffu;
  switch (cls)
    {
    case 0: return or_launch_count<64, 1024>(nq, list, text, qoff, qlen, w, soft, hash_mask, mc, rec, st);
    case 1: return or_launch_count<256, 8192>(nq, list, text, qoff, qlen, w, soft, hash_mask, mc, rec, st);
    case 2: return or_launch_count<1024, 32768>(nq, list, text, qoff, qlen, w, soft, hash_mask, mc, rec, st);
    default: return hipErrorInvalidValue;
    }
}

extern "C" hipError_t vsx_orient_launch_emit(uint32_t nq, const char * text, const char * qual, const uint64_t * qoff, const uint32_t * qlen,
                                             const OrRec * rec, char * out_text, char * out_qual, hipStream_t st)
{
  if (nq == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_orient_emit_kernel, dim3((nq + 3u) / 4u), dim3(256), 0, st, nq, text, qual, (const u64 *) qoff, qlen, rec, out_text,
                     out_qual);
  return hipGetLastError();
}
