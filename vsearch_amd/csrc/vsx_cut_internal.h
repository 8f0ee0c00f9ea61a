// vsx_cut_internal.h -- what vsx_cut.cpp and vsx_cut.hip share: the pattern as the kernels take it and the launchers.
#ifndef VSX_CUT_INTERNAL_H
#define VSX_CUT_INTERNAL_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#define VSX_CUT_MAX_P 64u           // pattern symbols on the device: a window spans at most two 64-position blocks

// the pattern: 4-bit codes (chrmap_4bit) and the two cut offsets
typedef struct VsxCutPattern {
  uint8_t  code[VSX_CUT_MAX_P];
  uint32_t P;
  uint32_t cut_fwd, cut_rev;
} VsxCutPattern;

// one work item of the match kernel: blocks [block0, block0 + tile_blocks) of sequence seq
typedef struct VsxCutItem {
  uint32_t seq, block0;
} VsxCutItem;

// a fragment record as the device writes it: include/vsx_cut.h's vsx_cut_fragment with the sequence number in the low word
typedef struct VsxCutRec {
  uint32_t seq, seq_hi, start, length;
} VsxCutRec;

#ifdef __cplusplus
extern "C" {
#endif

// match: a wave per item; the match word and its popcount of every block of the item (block g = bstart[seq] + block in sequence)
hipError_t vsx_launch_cut_match(const uint8_t * d_text, const uint64_t * d_off, const uint32_t * d_len, const uint32_t * d_bstart,
                                const VsxCutItem * d_items, uint32_t n_items, uint32_t tile_blocks, VsxCutPattern pat,
                                unsigned long long * d_bits, uint32_t * d_count, hipStream_t st);
// rocPRIM exclusive sums (temp == NULL: the size of the temporary storage)
hipError_t vsx_launch_cut_scan32(void * temp, size_t * temp_bytes, const uint32_t * d_in, uint32_t * d_out, uint64_t count, hipStream_t st);
hipError_t vsx_launch_cut_scan64(void * temp, size_t * temp_bytes, const uint64_t * d_in, uint64_t * d_out, uint64_t count, hipStream_t st);
// compaction: position 64 * g + bit of every match, at its rank
hipError_t vsx_launch_cut_compact(const unsigned long long * d_bits, const uint32_t * d_rank, uint32_t n_blocks, unsigned long long * d_pos, hipStream_t st);
// per sequence: matches, printed forward and reverse fragments, uncut flag (each array has n + 1 entries; the launcher leaves entry n to the caller)
hipError_t vsx_launch_cut_seqinfo(uint32_t n, const uint32_t * d_len, const uint32_t * d_bstart, const uint32_t * d_rank, const unsigned long long * d_pos,
                                  VsxCutPattern pat, uint32_t * d_matches, uint32_t * d_nfwd, uint32_t * d_nrev, uint32_t * d_uncut, hipStream_t st);
// a lane per match: its forward and reverse fragment records (and the tail pieces behind a sequence's last match); d_fwd / d_rev may be
// NULL; d_plen (may be NULL) takes every reverse record's piece length for the emit kernel: its length, or 0 when !rev_text
hipError_t vsx_launch_cut_fragments(uint32_t n, uint32_t n_matches, const uint32_t * d_len, const uint32_t * d_bstart, const uint32_t * d_rank,
                                    const unsigned long long * d_pos, VsxCutPattern pat, const uint32_t * d_basef, const uint32_t * d_baser,
                                    VsxCutRec * d_fwd, VsxCutRec * d_rev, unsigned long long * d_plen, int rev_text, hipStream_t st);
// a lane per sequence: the uncut list, and (d_prec / d_plen not NULL) the whole sequence as a piece with its length (0 when !want_text)
hipError_t vsx_launch_cut_uncut(uint32_t n, const uint32_t * d_len, const uint32_t * d_matches, const uint32_t * d_baseu, uint32_t * d_list,
                                VsxCutRec * d_prec, unsigned long long * d_plen, int want_text, hipStream_t st);
// emit: a wave per 64 output bytes; piece p (d_prec[p], d_poff[p] .. d_poff[p + 1]) reversed and complemented
hipError_t vsx_launch_cut_emit(const uint8_t * d_text, const uint64_t * d_off, const VsxCutRec * d_prec, const unsigned long long * d_poff,
                               uint64_t n_pieces, uint64_t total_bytes, uint8_t * d_out, hipStream_t st);

#ifdef __cplusplus
}
#endif
#endif
