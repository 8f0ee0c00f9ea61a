// vsx_exact.hip -- exact sequence search on gfx950 (--search_exact): hash, index build, probe and compare.
//
// The reference (core/dbhash.cpp, commands/search_exact.cpp) hashes every normalised sequence, keeps the database in an
// open-addressing table and, for a query strand, walks the slots from its hash on, comparing the sequences whose hash agrees.
// Here the three steps are three kernels over 4-bit codes (chrmap_4bit, the codes utils/seqcmp.cpp compares):
//
//   hash     one wavefront per sequence.  A lane takes VSX_EXACT_CHUNK = 16 symbols with one 16-byte load, turns them into one
//            64-bit word of codes (symbol i in bits 4i .. 4i+3), stores the word and mixes it with its position; the wave adds
//            the lanes' values and mixes in the length.  A reverse strand is read backwards: the lane loads the 16 bytes that
//            END where its chunk begins (two aligned loads and a byte shift), packs them in text order and bit-reverses the
//            word -- reversing 64 bits reverses the 16 nibbles and, inside each, swaps A<->T and C<->G, which is the complement of
//            every IUPAC code.  So the words, and with them the hash, of a reverse strand are those of its reverse-complemented
//            text, which is what the database side stores.  The sum over chunks is commutative: the order of lanes is free.
//   insert   one thread per database sequence: linear probing with a 32-bit compare-and-swap on the slot's sequence number;
//            hash and length are ordinary stores behind it (the probe kernel is a later launch).  The order in which equal
//            hashes land varies from run to run; the host sorts every query's matches, so the results do not.
//   probe    one wavefront per query strand.  The wave reads 64 slots at a time (one 16-byte load per lane), stops at the first
//            free one, and for every slot whose hash and length agree compares the code words, 32 symbols per lane and load.
//            Count, then fill: a first walk counts the matches, lane 0 reserves that many places with one 64-bit atomic add,
//            and a second walk (only for strands that matched, only when the places lie below the capacity) stores the targets.
//            Nothing is written past the buffer; the host reads the space asked for and launches again if it was short.
//
// Integer code only; no kernel waits for another workgroup.
#include <hip/hip_runtime.h>
#include "vsx_exact_internal.h"
#include "vsx_devutil.h"
#include "vsx_symbols.h"

namespace {

typedef unsigned long long u64;
using vsxd::shfl_xor64;
using vsxsym::mix64;

// chrmap_4bit for 'a' .. 'p' and 'q' .. 'z', one nibble per letter
constexpr u64 table_of(const char * codes, int first)
{
  u64 t = 0;
  for (int k = 0; k < 16 && first + k < 26; ++k) t |= (u64) (unsigned char) codes[first + k] << (4 * k);
  return t;
}
//                                  a  b   c  d   e  f  g  h   i  j  k   l  m  n   o  p  q  r  s  t  u  v  w  x  y   z
constexpr char kCodes[26] = {1, 14, 2, 13, 0, 0, 4, 11, 0, 0, 12, 0, 3, 15, 0, 0, 0, 5, 6, 8, 8, 7, 9, 0, 10, 0};
constexpr u64 kTableLo = table_of(kCodes, 0), kTableHi = table_of(kCodes, 16);

__device__ inline uint32_t code_of(uint32_t byte)
{
  const uint32_t idx = (byte | 0x20u) - (uint32_t) 'a';
  const u64 t = idx < 16u ? kTableLo : kTableHi;
  const uint32_t c = (uint32_t) (t >> ((idx & 15u) * 4u)) & 15u;
  return idx < 26u ? c : 0u;
}

// the codes of eight text bytes, byte i in nibble i; `zero_as`: the code a symbol outside the alphabet gets
__device__ inline uint32_t pack8(u64 bytes, uint32_t zero_as)
{
  uint32_t w = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i)
    {
      uint32_t c = code_of((uint32_t) (bytes >> (8 * i)) & 255u);
      if (c == 0u) c = zero_as;
      w |= c << (4 * i);
    }
  return w;
}

__global__ __launch_bounds__(VSX_EXACT_THREADS)
void vsx_exact_hash_kernel(const VsxExactItem * __restrict__ items, uint32_t n_items, const uint8_t * __restrict__ text, u64 hash_mask,
                           u64 * __restrict__ words, u64 * __restrict__ hash)
{
  const uint32_t item = __builtin_amdgcn_readfirstlane(blockIdx.x * VSX_EXACT_WAVES + (threadIdx.x >> 6));
  if (item >= n_items) return;
  const int lane = threadIdx.x & 63;
  const VsxExactItem it = items[item];
  const int64_t len = it.len;
  const int64_t nwords = (len + VSX_EXACT_CHUNK - 1) / VSX_EXACT_CHUNK;
  const uint8_t * const base = text + it.off;                 // 16-byte aligned; the slot is round_up(len, 16) + 16 bytes
  u64 * const out = words + it.woff;
  u64 acc = 0;
  for (int64_t c = lane; c < nwords; c += 64)
    {
      // s: text position of the 16 bytes this chunk is made of (reverse: they end where the chunk begins, s > -16)
      const int64_t s = it.reverse ? len - VSX_EXACT_CHUNK * c - VSX_EXACT_CHUNK : VSX_EXACT_CHUNK * c;
      const int64_t a = s & ~(int64_t) 15;                    // rounds down, also below zero
      const int sh = (int) (s - a);
      uint4 lo = make_uint4(0, 0, 0, 0), hi = make_uint4(0, 0, 0, 0);
      if (a >= 0) lo = *reinterpret_cast<const uint4 *>(base + a);
      if (sh != 0) hi = *reinterpret_cast<const uint4 *>(base + a + 16);        // a + 16 <= len: inside the slot's padding at most
      u64 w0 = ((u64) lo.y << 32) | lo.x, w1 = ((u64) lo.w << 32) | lo.z, w2 = ((u64) hi.y << 32) | hi.x;
      const u64 w3 = ((u64) hi.w << 32) | hi.z;
      int shb = sh;
      if (shb >= 8) { w0 = w1; w1 = w2; w2 = w3; shb -= 8; }
      if (shb != 0)
        {
          w0 = (w0 >> (8 * shb)) | (w1 << (64 - 8 * shb));
          w1 = (w1 >> (8 * shb)) | (w2 << (64 - 8 * shb));
        }
      // nibble i = text position s + i; the positions inside the sequence
      const int first = s < 0 ? (int) -s : 0;
      const int64_t left = len - s;
      const int last = left < 16 ? (int) left : 16;
      // a symbol outside the alphabet complements to 'N' (chrmap_complement), and stays code 0 on the plus strand
      const uint32_t zero_as = it.reverse ? 15u : 0u;
      u64 word = ((u64) pack8(w1, zero_as) << 32) | pack8(w0, zero_as);
      u64 keep = ~0ull;
      if (first > 0) keep &= ~0ull << (4 * first);
      if (last < 16) keep &= ~(~0ull << (4 * last));
      word &= keep;
      if (it.reverse) word = __brevll(word);
      out[c] = word;
      acc += mix64(word ^ ((u64) (c + 1) * vsxsym::kGolden));
    }
  if ((nwords & 1) && lane == 0) out[nwords] = 0;            // the pad word: the compare loop reads pairs
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) acc += shfl_xor64(acc, m);
  if (lane == 0) hash[item] = mix64(acc ^ ((u64) len * vsxsym::kLengthMul)) & hash_mask;
}

__global__ __launch_bounds__(256)
void vsx_exact_insert_kernel(const u64 * __restrict__ hash, const uint32_t * __restrict__ len, uint32_t first, uint32_t n,
                             VsxExactSlot * table, u64 table_size)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t l = len[i];
  if (l == 0) return;                                         // a zero-length database sequence matches nothing
  const u64 h = hash[i], mask = table_size - 1;
  u64 j = h & mask;
  // at most 2/3 of the slots are ever taken: a free one comes up
  for (u64 step = 0; step < table_size; ++step)
    {
      const uint32_t old = atomicCAS(&table[j].seq, VSX_EXACT_EMPTY, first + i);
      if (old == VSX_EXACT_EMPTY) { table[j].hash = h; table[j].len = l; return; }
      j = (j + 1) & mask;
    }
}

// one walk of a strand's chain; FILL: store the targets at dst[0 ...), else count only
template <bool FILL>
__device__ inline uint32_t walk(const VsxExactSlot * __restrict__ table, u64 table_size, u64 h, uint32_t len, const uint4 * __restrict__ q4,
                                const u64 * __restrict__ dbwords, const u64 * __restrict__ dbwoff, int lane, uint32_t * dst,
                                u64 & visited, u64 & compared)
{
  const u64 mask = table_size - 1;
  const uint32_t npairs = ((len + VSX_EXACT_CHUNK - 1) / VSX_EXACT_CHUNK + 1) / 2;
  const u64 rounds = (table_size + 63) / 64 + 1;
  uint32_t m = 0;
  u64 j = h & mask;
  for (u64 r = 0; r < rounds; ++r, j += 64)
    {
      const uint4 slot = *reinterpret_cast<const uint4 *>(table + ((j + (u64) lane) & mask));
      const bool empty = slot.z == VSX_EXACT_EMPTY;
      const u64 b_empty = __ballot(empty);
      u64 b_cand = __ballot(!empty && slot.x == (uint32_t) h && slot.y == (uint32_t) (h >> 32) && slot.w == len);
      // a table of fewer than 64 slots wraps inside one load: the lanes before the first free slot are distinct slots
      if (b_empty)
        {
          const int stop = __ffsll(b_empty) - 1;
          b_cand &= (1ull << stop) - 1;
          visited += (u64) stop + 1;
        }
      else visited += 64;
      while (b_cand)
        {
          const int k = __ffsll(b_cand) - 1;
          b_cand &= b_cand - 1;
          const uint32_t target = (uint32_t) __shfl((int) slot.z, k);
          const uint4 * const t4 = reinterpret_cast<const uint4 *>(dbwords + dbwoff[target]);
          bool differ = false;
          for (uint32_t p = lane; p < npairs; p += 64)
            {
              const uint4 a = q4[p], b = t4[p];
              differ |= (a.x != b.x) | (a.y != b.y) | (a.z != b.z) | (a.w != b.w);
            }
          ++compared;
          if (__ballot(differ) == 0)
            {
              if (FILL && lane == 0) dst[m] = target;
              ++m;
            }
        }
      if (b_empty) break;
    }
  return m;
}

__global__ __launch_bounds__(VSX_EXACT_THREADS)
void vsx_exact_probe_kernel(const VsxExactItem * __restrict__ items, uint32_t n_items, const u64 * __restrict__ qwords,
                            const u64 * __restrict__ qhash, const VsxExactSlot * __restrict__ table, u64 table_size,
                            const u64 * __restrict__ dbwords, const u64 * __restrict__ dbwoff, uint32_t * __restrict__ cnt,
                            u64 * __restrict__ start, uint32_t * __restrict__ hits, u64 hit_cap, VsxExactCounters * counters)
{
  const uint32_t item = __builtin_amdgcn_readfirstlane(blockIdx.x * VSX_EXACT_WAVES + (threadIdx.x >> 6));
  if (item >= n_items) return;
  const int lane = threadIdx.x & 63;
  const VsxExactItem it = items[item];
  uint32_t m = 0;
  u64 at = 0, visited = 0, compared = 0;
  if (it.len != 0)                                            // a zero-length query has no hits
    {
      const uint4 * const q4 = reinterpret_cast<const uint4 *>(qwords + it.woff);
      const u64 h = qhash[item];
      m = walk<false>(table, table_size, h, it.len, q4, dbwords, dbwoff, lane, nullptr, visited, compared);
      if (m != 0)
        {
          u64 mine = 0;
          if (lane == 0) mine = atomicAdd(&counters->hits, (u64) m);
          at =((u64) (uint32_t) __shfl((int) (uint32_t) (mine >> 32), 0) << 32) | (uint32_t) __shfl((int) (uint32_t) mine, 0);
          if (at + m <= hit_cap)
            {
              u64 v2 = 0, c2 = 0;
              (void) walk<true>(table, table_size, h, it.len, q4, dbwords, dbwoff, lane, hits + at, v2, c2);
            }
        }
    }
  if (lane == 0)
    {
      cnt[item] = m;
      start[item] = at;
      if (visited) atomicAdd(&counters->slots_visited, visited);
      if (compared) atomicAdd(&counters->candidates_compared, compared);
    }
}

}  // namespace

extern "C" hipError_t vsx_launch_exact_hash(const VsxExactItem * d_items, uint32_t n_items, const uint8_t * d_text, uint64_t hash_mask,
                                            uint64_t * d_words, uint64_t * d_hash, hipStream_t st)
{
  if (n_items == 0) return hipSuccess;
  const uint32_t blocks = (n_items + VSX_EXACT_WAVES - 1) / VSX_EXACT_WAVES;
  hipLaunchKernelGGL(vsx_exact_hash_kernel, dim3(blocks), dim3(VSX_EXACT_THREADS), 0, st, d_items, n_items, d_text, (u64) hash_mask,
                     reinterpret_cast<u64 *>(d_words), reinterpret_cast<u64 *>(d_hash));
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_exact_insert(const uint64_t * d_hash, const uint32_t * d_len, uint32_t first, uint32_t n,
                                              VsxExactSlot * d_table, uint64_t table_size, hipStream_t st)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_exact_insert_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, reinterpret_cast<const u64 *>(d_hash), d_len, first, n,
                     d_table, (u64) table_size);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_exact_probe(const VsxExactItem * d_items, uint32_t n_items, const uint64_t * d_qwords, const uint64_t * d_qhash,
                                             const VsxExactSlot * d_table, uint64_t table_size, const uint64_t * d_dbwords,
                                             const uint64_t * d_dbwoff, uint32_t * d_cnt, uint64_t * d_start, uint32_t * d_hits,
                                             uint64_t hit_cap, VsxExactCounters * d_counters, hipStream_t st)
{
  if (n_items == 0) return hipSuccess;
  const uint32_t blocks = (n_items + VSX_EXACT_WAVES - 1) / VSX_EXACT_WAVES;
  hipLaunchKernelGGL(vsx_exact_probe_kernel, dim3(blocks), dim3(VSX_EXACT_THREADS), 0, st, d_items, n_items,
                     reinterpret_cast<const u64 *>(d_qwords), reinterpret_cast<const u64 *>(d_qhash), d_table, (u64) table_size,
                     reinterpret_cast<const u64 *>(d_dbwords), reinterpret_cast<const u64 *>(d_dbwoff), d_cnt, reinterpret_cast<u64 *>(d_start), d_hits, (u64) hit_cap,
                     d_counters);
  return hipGetLastError();
}
