// vsx_tbtext.h -- result marshalling of one pair: run words -> CIGAR text, record -> the output arrays.  Shared by the traceback
// epilogues (vsx_device.hip), which format a pair while its record is in registers and its run words pass through them on their way
// to the dense run buffer, and by vsx_cigar_text_kernel (vsx_tbtext.hip), which formats from out[] / runs[] when only the text has
// to be made again.
//
// Text of a pair: for each run in TEXT order (= reverse run order) the decimal length if > 1, then 'M' / 'I' / 'D'; a terminating NUL;
// padded with zeros to a multiple of 4, so every store is a whole dword (pushop / finishop, align_simd.cpp:1013-1049).  The run
// words are in traceback order, so the string is written BACK TO FRONT, like the reference's: one pass over the words in the order
// they are stored, once the string's length is known.
#ifndef VSX_TBTEXT_H
#define VSX_TBTEXT_H

#include <hip/hip_runtime.h>
#include "vsx_internal.h"

__host__ __device__ inline uint32_t vsx_cigar_ndigits(uint32_t v)
{
  return v >= 10000u ? 5u : v >= 1000u ? 4u : v >= 100u ? 3u : v >= 10u ? 2u : 1u;
}

// text bytes of one run word: the count only when the run is longer than 1, then the letter
__host__ __device__ inline uint32_t vsx_cigar_run_len(uint32_t w)
{
  const uint32_t n = w >> 2;
  return 1u + (n > 1u ? vsx_cigar_ndigits(n) : 0u);
}

// bytes of the string of runs[0 .. nruns), the NUL included, not padded
__host__ __device__ inline uint32_t vsx_cigar_len(const uint32_t * runs, uint32_t nruns)
{
  uint32_t len = 1;                                      // NUL
  for (uint32_t x = 0; x < nruns; ++x) len += vsx_cigar_run_len(runs[x]);
  return len;
}

// Writes a string of `len` bytes (NUL included) as (len + 3) / 4 whole dwords at dst, last byte first: begin(), then run() for
// every run word in traceback order.  Bytes wait in `acc` until their dword is complete; the padding bytes stay zero.
struct VsxCigarWriter {
  uint32_t * dst;
  uint32_t acc;
  int p;                                                 // position of the next byte
  __host__ __device__ VsxCigarWriter(uint32_t * d, uint32_t len) : dst(d), acc(0), p((int) len - 1) {}
  __host__ __device__ void put(uint32_t ch)
  {
    acc |= ch << (8u * ((uint32_t) p & 3u));
    if ((p & 3) == 0) { dst[p >> 2] = acc; acc = 0; }
    --p;
  }
  __host__ __device__ void begin() { put(0u); }          // the NUL (and the padding above it)
  __host__ __device__ void run(uint32_t w)
  {
    uint32_t n = w >> 2;
    put((w & 3u) == 0u ? 'M' : (w & 3u) == 1u ? 'I' : 'D');
    if (n > 1u)
      do { put('0' + n % 10u); n /= 10u; } while (n);
  }
};

// the string of runs[0 .. nruns) as (vsx_cigar_len() + 3) / 4 whole dwords at dst
__host__ __device__ inline void vsx_cigar_format(const uint32_t * runs, uint32_t nruns, uint32_t * dst)
{
  VsxCigarWriter W(dst, vsx_cigar_len(runs, nruns));
  W.begin();
  for (uint32_t x = 0; x < nruns; ++x) W.run(runs[x]);
}

#ifdef __HIPCC__
// Wave collective -- EVERY lane of the wave must get here together, a lane without a pair with len4 = 0: the wave allocates the
// strings of its 64 pairs (len4 = padded bytes) with ONE atomic on the text cursor; they end up back to back in lane order.
// Returns the lane's offset.  The cursor grows whether the text will fit or not: the host sizes its re-run from it.
__device__ inline unsigned long long vsx_text_alloc(uint32_t len4, unsigned long long * text_cursor)
{
  const uint32_t lane = (uint32_t) threadIdx.x & 63u;
  uint32_t incl = len4;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1)
    {
      const uint32_t v = (uint32_t) __shfl_up((int) incl, d, 64);
      if ((int) lane >= d) incl += v;
    }
  const uint32_t total = (uint32_t) __shfl((int) incl, 63, 64);
  unsigned long long base = 0;
  if (lane == 0 && total) base = atomicAdd(text_cursor, (unsigned long long) total);
  base = (unsigned long long) __shfl((long long) base, 0, 64);
  return base + (unsigned long long) (incl - len4);
}

__device__ inline void vsx_soa_store(const VsxSoaOut & soa, uint32_t pid, const VsxPairOut & o, unsigned long long text_off)
{
  soa.score[pid] = o.score;
  soa.aligned[pid] = o.aligned;
  soa.matches[pid] = o.matches;
  soa.mismatches[pid] = o.mismatches;
  soa.gaps[pid] = o.gaps;
  soa.verdict[pid] = (uint8_t) o.pad;
  soa.text_off[pid] = text_off;
}

// The end of a traceback epilogue, one lane per pair (valid == false: a lane without one); EVERY lane of the wave must get here
// together.  o = the pair's final record; my = its run words in the lane's slab; nw = how many of them leave the kernel: o.nruns, or
// 0 when they did not fit the dense run buffer (the host runs the plan again; the pair has the lone NUL meanwhile); text_len = bytes
// of their string, the NUL included (vsx_cigar_run_len summed while the epilogue replayed the runs).  ONE pass over the words copies
// them to runs[o.run_off ..) and, if the string fits the text buffer, formats them on the way.
__device__ inline void vsx_marshal_pair(bool valid, uint32_t pid, const VsxPairOut & o, const uint32_t * my, uint32_t nw, uint32_t text_len,
                                        uint32_t * runs, const VsxTextOut & tx)
{
  if (nw == 0) text_len = 1;
  const uint32_t len4 = valid ? ((text_len + 3u) & ~3u) : 0u;
  const unsigned long long off = vsx_text_alloc(len4, tx.text_cursor);
  if (!valid) return;
  const bool fits = off + len4 <= tx.text_capacity;
  VsxCigarWriter W(reinterpret_cast<uint32_t *>(tx.text + off), text_len);
  if (fits) W.begin();
  for (uint32_t x = 0; x < nw; ++x)
    {
      const uint32_t w = my[x];
      runs[o.run_off + x] = w;
      if (fits) W.run(w);
    }
  vsx_soa_store(tx.soa, pid, o, off);
}
#endif

#endif
