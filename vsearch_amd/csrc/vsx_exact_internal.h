// vsx_exact_internal.h -- shared between the exact-search kernels (vsx_exact.hip) and their host side (vsx_exact.cpp).
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

#endif
