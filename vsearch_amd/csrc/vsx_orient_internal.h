// vsx_orient_internal.h -- what vsx_orient.cpp (host) and vsx_orient.hip (kernels) share: the record the count kernel writes, the
// length classes and the kernels' entry points.  Included by those two files alone.
#ifndef VSX_ORIENT_INTERNAL_H
#define VSX_ORIENT_INTERNAL_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>
#include "../../include/vsx_orient.h"

// per query, as the count kernel writes it (the host copies it into vsx_orient_record and sums `distinct`)
struct OrRec {
  uint32_t count_fwd, count_rev;
  int32_t  strand;
  uint32_t distinct;
};

// The length classes of the count kernel.  A query of L symbols has at most L distinct words, and a class's set has twice as
// many slots as its longest query has symbols, so a set is never more than half full and a probe always ends.
//   class 0   <=    512 symbols   one wavefront per query, four queries per block    1 024 slots (4 KB) per wave
//   class 1   <=  4 096 symbols   one block of 256 threads per query                 8 192 slots (32 KB)
//   class 2   <= 16 384 symbols   one block of 1 024 threads per query              32 768 slots (128 KB of the CU's 160 KB)
#define OR_CLASSES VSX_ORIENT_CLASSES
static const uint32_t kOrClassQlen[OR_CLASSES] = {512u, 4096u, VSX_ORIENT_MAX_QLEN};
#define OR_EMPTY 0xffffffffu             // an empty slot: no word of <= 30 bits equals it

extern "C" {
// ---- the match-count build: one chunk of consecutive database sequences [first_seq, first_seq + nseq)
// keys[slot_of[seq] - slot_of[first_seq] + p] = (chunk-local sequence << 2 w) | word at p, or (nseq << 2 w) where no valid word starts
hipError_t vsx_orient_launch_keys(const uint8_t * codes, const uint64_t * off, const uint32_t * len, const uint8_t * lower_bits,
                                  const uint64_t * slot_of, uint32_t first_seq, uint32_t nseq, uint32_t maxlen, int w, uint64_t * keys,
                                  hipStream_t st);
// rocPRIM radix sort of the low end_bit bits; temp == nullptr: only *temp_bytes is set
hipError_t vsx_orient_sort_keys(void * temp, size_t * temp_bytes, uint64_t * keys_in, uint64_t * keys_out, uint64_t n, unsigned end_bit,
                                hipStream_t st);
// the first key of each run of equal keys adds one to mc[word] (integer atomic)
hipError_t vsx_orient_launch_runs(const uint64_t * keys, uint64_t n, uint32_t nseq, int w, uint32_t * mc, hipStream_t st);

// ---- the count kernel of one length class: list[0 .. nq) = the class's queries as slots into qoff / qlen / rec
hipError_t vsx_orient_launch_count(int cls, uint32_t nq, const uint32_t * list, const char * text, const uint64_t * qoff, const uint32_t * qlen,
                                   int w, int soft, int hash_bits, const uint32_t * mc, OrRec * rec, hipStream_t st);
// ---- the emit kernel: one wavefront per read; qual / out_qual may be NULL
hipError_t vsx_orient_launch_emit(uint32_t nq, const char * text, const char * qual, const uint64_t * qoff, const uint32_t * qlen,
                                  const OrRec * rec, char * out_text, char * out_qual, hipStream_t st);
}

#endif
