// vsx_exact_internal.h -- shared between the exact-search kernels (vsx_exact.hip), their host side (vsx_exact.cpp) and
// dereplication (vsx_derep.hip, vsx_derep.cpp), which reuses the hash kernel and the staging plan.
#ifndef VSX_EXACT_INTERNAL_H
#define VSX_EXACT_INTERNAL_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>

#define VSX_EXACT_WAVES    4                 // one wavefront per sequence (strand), four per workgroup
#define VSX_EXACT_THREADS  (64 * VSX_EXACT_WAVES)
#define VSX_EXACT_CHUNK    16                // symbols one lane hashes at a time: one 16-byte load, one 64-bit word of 4-bit codes
#define VSX_EXACT_PAIR     32                // symbols one lane compares at a time: two words, one 16-byte load per side
#define VSX_EXACT_PASS     (64 * VSX_EXACT_CHUNK)    // symbols one pass of the hash kernel's wave covers (1 024)
#define VSX_EXACT_CMP_PASS (64 * VSX_EXACT_PAIR)     // symbols one pass of the compare loop covers (2 048)
#define VSX_EXACT_TEXT_PAD 16                // bytes behind every staged sequence (slot = round_up(len, 16) + 16)
#define VSX_EXACT_EMPTY    0xFFFFFFFFu       // VsxExactSlot.seq of a free slot

// one sequence (strand) of a staged window
struct VsxExactItem {
  uint64_t off;        // of its text in the staged buffer, a multiple of 16
  uint64_t woff;       // of its code words in the word buffer, a multiple of 2
  uint32_t len;
  uint32_t reverse;    // 1: the item is the reverse complement of the text at `off` (read backwards, codes complemented)
};

// one slot of the open-addressing table (16 bytes: one load per lane)
struct VsxExactSlot {
  uint64_t hash;
  uint32_t seq;        // database sequence number, VSX_EXACT_EMPTY when free
  uint32_t len;
};

// counters of one probe launch (device, 64-bit)
struct VsxExactCounters {
  unsigned long long hits, slots_visited, candidates_compared, pad;
};

#ifdef __cplusplus
extern "C" {
#endif
// code words (16 four-bit codes each, symbol i in bits 4i .. 4i+3, unused nibbles and the pad word zero) and the 64-bit hash,
// cut to hash_mask, of every item
hipError_t vsx_launch_exact_hash(const VsxExactItem * d_items, uint32_t n_items, const uint8_t * d_text, uint64_t hash_mask,
                                 uint64_t * d_words, uint64_t * d_hash, hipStream_t st);
// the sequences first .. first + n - 1 (lengths d_len[0 .. n), hashes d_hash[0 .. n)) into the table of table_size slots
hipError_t vsx_launch_exact_insert(const uint64_t * d_hash, const uint32_t * d_len, uint32_t first, uint32_t n, VsxExactSlot * d_table,
                                   uint64_t table_size, hipStream_t st);
// every item against the table: d_cnt[item] matches; when they fit below hit_cap their targets lie at d_hits[d_start[item] ...).
// d_counters->hits is the space the launch asked for: above hit_cap nothing of the overflow was written, and the caller
// launches again with a larger buffer.
hipError_t vsx_launch_exact_probe(const VsxExactItem * d_items, uint32_t n_items, const uint64_t * d_qwords, const uint64_t * d_qhash,
                                  const VsxExactSlot * d_table, uint64_t table_size, const uint64_t * d_dbwords, const uint64_t * d_dbwoff,
                                  uint32_t * d_cnt, uint64_t * d_start, uint32_t * d_hits, uint64_t hit_cap, VsxExactCounters * d_counters,
                                  hipStream_t st);
#ifdef __cplusplus
}
#endif

#ifdef __cplusplus
// ---- the staging plan of a window of sequences, shared by the hosts of the kernels (vsx_exact.cpp, vsx_derep.cpp) -----------------
#include <cstdlib>
namespace vsxe {

inline uint64_t round_up(uint64_t v, uint64_t m) { return (v + m - 1) / m * m; }
inline uint64_t words_of(uint32_t len) { return round_up(((uint64_t) len + VSX_EXACT_CHUNK - 1) / VSX_EXACT_CHUNK, 2); }
inline uint64_t slot_of(uint32_t len) { return round_up(len, 16) + VSX_EXACT_TEXT_PAD; }

// the reference's table: a power of two, at most 2/3 full (core/dbhash.cpp: dbhash_open)
inline uint64_t table_size_for(uint64_t n)
{
  uint64_t size = 1;
  while (3 * n > 2 * size) size *= 2;
  return size;
}

// the hashes cut to the low `bits` bits named by the variable (tests: the comparison alone decides); unset or out of range: all 64
inline uint64_t hash_mask_from_env(const char * name)
{
  const char * e = std::getenv(name);
  if (!e) return ~0ull;
  const long bits = std::strtol(e, nullptr, 10);
  if (bits < 1 || bits >= 64) return ~0ull;
  return (1ull << bits) - 1;
}

// the items of a window of sequences: text slots, word slots; both: items [n, 2n) are the minus strands, staged as text of
// their own (own_minus: they are masked on their own) or read backwards from the plus strand's slot
struct Plan { uint64_t n = 0, ns = 0, text_bytes = 0, words = 0; bool both = false, own_minus = false; };

template <typename FLen>
Plan plan_items(uint64_t n, FLen len, bool both, bool own_minus, VsxExactItem * items)
{
  Plan P;
  P.n = n; P.ns = both ? 2 * n : n; P.both = both; P.own_minus = own_minus;
  uint64_t t = 0, w = 0;
  for (uint64_t k = 0; k < n; ++k)
    {
      items[k] = VsxExactItem {t, w, len(k), 0u};
      t += slot_of(len(k)); w += words_of(len(k));
    }
  if (both)
    for (uint64_t k = 0; k < n; ++k)
      {
        if (own_minus) { items[n + k] = VsxExactItem {t, w, len(k), 0u}; t += slot_of(len(k)); }
        else items[n + k] = VsxExactItem {items[k].off, w, len(k), 1u};
        w += words_of(len(k));
      }
  P.text_bytes = t; P.words = w;
  return P;
}

}  // namespace vsxe
#endif

#endif
