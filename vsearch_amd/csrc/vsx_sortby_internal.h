// vsx_sortby_internal.h -- what vsx_sortby.cpp and vsx_sortby.hip share: the launchers of one refinement step.
//
// An "active" array holds the records whose place is still open, in output-position order.  Record a carries item[a] (its input
// number) and g[a] (the first output position of its group: the records it still ties with sit at positions g, g + 1, ...).
// A step sorts the active records stably by (g, chunk) and splits every group where the chunk changes.
#ifndef VSX_SORTBY_INTERNAL_H
#define VSX_SORTBY_INTERNAL_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

// rocPRIM (temp == NULL: the size of the temporary storage): exclusive sum, inclusive maximum, stable radix sorts of (key, value) pairs
hipError_t vsx_launch_sortby_scan_sum(void * temp, size_t * temp_bytes, const uint32_t * d_in, uint32_t * d_out, uint64_t count, hipStream_t st);
hipError_t vsx_launch_sortby_scan_max(void * temp, size_t * temp_bytes, const uint32_t * d_in, uint32_t * d_out, uint64_t count, hipStream_t st);
hipError_t vsx_launch_sortby_sort64(void * temp, size_t * temp_bytes, const unsigned long long * d_kin, unsigned long long * d_kout,
                                    const uint32_t * d_vin, uint32_t * d_vout, uint64_t count, uint32_t end_bit, hipStream_t st);
hipError_t vsx_launch_sortby_sort32(void * temp, size_t * temp_bytes, const uint32_t * d_kin, uint32_t * d_kout, const uint32_t * d_vin,
                                    uint32_t * d_vout, uint64_t count, uint32_t end_bit, hipStream_t st);

// keep[i] = 1 when record i is in the deck (order VSX_SORTBY_SIZE: minsize <= size <= maxsize; else every record)
hipError_t vsx_launch_sortby_select(uint32_t n, int order, long long minsize, long long maxsize, const uint32_t * d_size, uint32_t * d_keep,
                                    hipStream_t st);
// the deck in input order: item, numeric key (descending fields complemented) and group start 0, at slot[i] of every kept record
hipError_t vsx_launch_sortby_keys(uint32_t n, int order, const uint32_t * d_seqlen, const uint32_t * d_size, const uint32_t * d_keep,
                                  const uint32_t * d_slot, uint32_t * d_item, unsigned long long * d_key, uint32_t * d_g, hipStream_t st);
// idx[a] = a
hipError_t vsx_launch_sortby_iota(uint32_t m, uint32_t * d_idx, hipStream_t st);
// chunk[a] = bytes [8 round, 8 round + 8) of the header of item[a], first byte highest, zero beyond the header's end
hipError_t vsx_launch_sortby_chunk(uint32_t m, uint32_t round, const uint8_t * d_blob, const uint64_t * d_off, const uint32_t * d_len,
                                   const uint32_t * d_item, unsigned long long * d_chunk, hipStream_t st);
// out[a] = in[idx[a]]
hipError_t vsx_launch_sortby_gather32(uint32_t m, const uint32_t * d_in, const uint32_t * d_idx, uint32_t * d_out, hipStream_t st);
// the records in their new order (idx) and the marks of the first record of every old group: first[a] = a there, else 0
hipError_t vsx_launch_sortby_gather(uint32_t m, const uint32_t * d_idx, const unsigned long long * d_chunk, const uint32_t * d_item,
                                    const uint32_t * d_g2, unsigned long long * d_chunk2, uint32_t * d_item2, uint32_t * d_first, hipStream_t st);
// (first = the inclusive maximum of the marks: the index of the group's first record)  position p = g2 + a - first; order[p] = item2;
// mark[a] = p where a new group begins (the old group's start or a change of chunk), else 0
hipError_t vsx_launch_sortby_place(uint32_t m, const uint32_t * d_g2, const uint32_t * d_first, const unsigned long long * d_chunk2,
                                   const uint32_t * d_item2, uint32_t * d_order, uint32_t * d_mark, hipStream_t st);
// (ng = the inclusive maximum of the marks: the start of the new group)  open[a] = 1 when the new group has more than one member and,
// in a label round, its chunk does not end in a zero byte (a zero there: every member's header has ended, they are equal)
hipError_t vsx_launch_sortby_open(uint32_t m, int label_round, const uint32_t * d_ng, const unsigned long long * d_chunk2, uint32_t * d_open,
                                  hipStream_t st);
// the open records, in order, at slot[a]: item and group start for the next round
hipError_t vsx_launch_sortby_compact(uint32_t m, const uint32_t * d_open, const uint32_t * d_slot, const uint32_t * d_item2, const uint32_t * d_ng,
                                     uint32_t * d_item, uint32_t * d_g, hipStream_t st);

#ifdef __cplusplus
}
#endif
#endif
