// vsx_fastx_mask_internal.h -- what vsx_fastx_mask.cpp and vsx_fastx_mask.hip share: the launchers of the masking kernels.
#ifndef VSX_FASTX_MASK_INTERNAL_H
#define VSX_FASTX_MASK_INTERNAL_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#define VSX_MASK_PAD 64u            // bytes readable behind a window's packed text
#define VSX_MASK_ENTRIES 64u        // entry offsets of a segment: a chain step is at most 62
#define VSX_MASK_APPLY_TILE 4096u   // symbols of a long sequence one wave of the apply kernel takes
#define VSX_MASK_APPLY_WHOLE 16384u // a sequence up to this length is applied by one wave

// per position i of a long-route sequence: next(i) - i (bits 0-5), the interval [a, b] of W(i) (bits 6-11, 12-17), v > 20 (bit 18)
#define VSX_MASK_W_STEP(w) ((w) & 63u)
#define VSX_MASK_W_A(w) (((w) >> 6) & 63u)
#define VSX_MASK_W_B(w) (((w) >> 12) & 63u)
#define VSX_MASK_W_MASKED(w) (((w) >> 18) & 1u)

#ifdef __cplusplus
extern "C" {
#endif

// short route: one wave per listed sequence walks its windows in order and ORs the intervals into dbits; *counter += windows visited
hipError_t vsx_launch_mask_short(const uint8_t * d_text, const uint64_t * d_off, const uint32_t * d_len, const uint32_t * d_list, uint32_t n_list,
                                 uint32_t * d_dbits, unsigned long long * d_counter, hipStream_t st);
// long route, positions [c0, c0 + npos) of the sequence of L symbols at d_seq: W(i) of every position into d_w[i - c0]
hipError_t vsx_launch_mask_eval(const uint8_t * d_seq, uint32_t L, uint32_t c0, uint32_t npos, uint32_t * d_w, hipStream_t st);
// the chain through the chunk: segment walks from every entry offset, the serial pick of each segment's true entry (reads and
// rewrites *d_entry, the chain's offset into the chunk), and the marking walk that ORs the chain's intervals into dbits at bit0 + position
hipError_t vsx_launch_mask_chain(const uint32_t * d_w, uint32_t L, uint32_t c0, uint32_t npos, uint32_t S, uint8_t * d_exit, uint8_t * d_true,
                                 uint32_t * d_entry, uint32_t * d_dbits, uint64_t bit0, hipStream_t st);
// apply: text + DUST bits -> masked text (or none), the bits of the symbols that do not count (or none), the unmasked counts.
// whole: one wave per sequence, every sequence of at most VSX_MASK_APPLY_WHOLE symbols; tiles: one long sequence, counts added to d_unmasked[k]
hipError_t vsx_launch_mask_apply(const uint8_t * d_text, const uint64_t * d_off, const uint32_t * d_len, uint32_t n, int qmask, int hard,
                                 const uint32_t * d_dbits, uint8_t * d_out, unsigned long long * d_obits, uint32_t * d_unmasked, hipStream_t st);
hipError_t vsx_launch_mask_apply_long(const uint8_t * d_text, uint64_t off, uint32_t len, uint32_t k, int qmask, int hard,
                                      const uint32_t * d_dbits, uint8_t * d_out, unsigned long long * d_obits, uint32_t * d_unmasked, hipStream_t st);

#ifdef __cplusplus
}
#endif
#endif
