// vsx_tbtext.hip -- result marshalling on the device: run lists -> CIGAR text, records -> the five output arrays.
//
// The reference builds the CIGAR string inside its traceback (pushop / finishop, src/core/align_simd.cpp:1013-1049:
// run-length text written right to left, the count omitted when it is 1) and hands every caller five arrays
// (pscores / paligned / pmatches / pmismatches / pgaps, align_simd.hpp:99-108).  Here the traceback kernels
// (vsx_device.hip) do the same in their epilogue (vsx_tbtext.h) and also leave 24-byte records and a dense buffer of
// run words ((length << 2) | op, traceback order = last column first); the kernel below makes the text and the arrays
// from those: after settle() has enlarged a text buffer that was too small, and in a build without VSX_TB_FUSED_TEXT
// after every traceback.  HBM-bound byte work, one lane per pair, strings dword-aligned so every store is a full dword.
#include <hip/hip_runtime.h>
#include "vsx_internal.h"
#include "vsx_tbtext.h"

typedef unsigned int u32;

// One lane per GPU pair (k-th entry of pair_ids): the pair's record and its words of the dense run buffer -> text and arrays
__global__ void __launch_bounds__(256)
vsx_cigar_text_kernel(const VsxPairOut * __restrict__ out, const u32 * __restrict__ pair_ids, u32 npairs,
                      const u32 * __restrict__ runs, uint64_t runs_capacity,
                      uint8_t * __restrict__ text, uint64_t text_capacity, unsigned long long * text_cursor,
                      VsxSoaOut soa)
{
  const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = k < npairs;
  const u32 pid = valid ? pair_ids[k] : 0u;
  VsxPairOut o {};
  if (valid) o = out[pid];
  const bool have_runs = valid && (o.run_off + o.nruns <= runs_capacity);    // an overflowed run buffer is re-run by the host
  const u32 * __restrict__ my = runs + o.run_off;
  const u32 nruns = have_runs ? o.nruns : 0u;
  const u32 len4 = valid ? ((vsx_cigar_len(my, nruns) + 3u) & ~3u) : 0u;
  const unsigned long long off = vsx_text_alloc(len4, text_cursor);
  if (!valid) return;
  if (off + len4 <= text_capacity) vsx_cigar_format(my, nruns, reinterpret_cast<u32 *>(text + off));
  vsx_soa_store(soa, pid, o, off);
}

// the formatter on the host (tests): the string of runs[0 .. nruns) into dst if its padded size fits dst_bytes; returns that size
extern "C" uint32_t vsx_internal_cigar_format(const uint32_t * runs, uint32_t nruns, uint8_t * dst, uint32_t dst_bytes)
{
  const uint32_t len4 = (vsx_cigar_len(runs, nruns) + 3u) & ~3u;
  if (len4 <= dst_bytes) vsx_cigar_format(runs, nruns, reinterpret_cast<uint32_t *>(dst));
  return len4;
}

// ---------------------------------------------------------------------------------------------
// Reverse complement in the 4-bit code domain (utils/reverse_complement.cpp:70-82 + chrmap_complement, utils/maps.cpp:
// 121-150): the complement of an IUPAC set code is its bit reversal (A1 <-> T8, C2 <-> G4, R5 <-> Y10, ...); a symbol
// that is no IUPAC letter (code 0) complements to 'N' = 15, as the reference's table does.  One workgroup per sequence:
// sequence k of `src` is read backwards and written forwards as sequence k of `dst`.  HBM-bound, 1 B in / 1 B out.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
vsx_revcomp_kernel(const uint8_t * __restrict__ codes, const uint64_t * __restrict__ src_off, const uint64_t * __restrict__ dst_off,
                   const uint32_t * __restrict__ len)
{
  const uint64_t k = blockIdx.x;
  const uint8_t * __restrict__ s = codes + src_off[k];
  uint8_t * __restrict__ d = const_cast<uint8_t *>(codes) + dst_off[k];
  const u32 L = len[k];
  for (u32 x = threadIdx.x; x < L; x += 256)
    {
      const u32 c = s[L - 1 - x] & 15u;
      const u32 r = ((c & 1u) << 3) | ((c & 2u) << 1) | ((c & 4u) >> 1) | ((c & 8u) >> 3);
      d[x] = (uint8_t) (c == 0u ? 15u : r);
    }
}

extern "C" hipError_t vsx_launch_revcomp(uint8_t * d_codes, const uint64_t * d_src_off, const uint64_t * d_dst_off,
                                         const uint32_t * d_len, uint64_t nseq, hipStream_t st)
{
  if (nseq == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_revcomp_kernel, dim3((unsigned) nseq), dim3(256), 0, st, d_codes, d_src_off, d_dst_off, d_len);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_cigar_text(const VsxPairOut * d_out, const uint32_t * d_pair_ids, uint32_t npairs,
                                            const uint32_t * d_runs, uint64_t runs_capacity,
                                            uint8_t * d_text, uint64_t text_capacity, unsigned long long * d_text_cursor,
                                            VsxSoaOut soa, hipStream_t st)
{
  if (npairs == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_cigar_text_kernel, dim3((npairs + 255) / 256), dim3(256), 0, st,
                     d_out, d_pair_ids, npairs, d_runs, runs_capacity, d_text, text_capacity, d_text_cursor, soa);
  return hipGetLastError();
}
