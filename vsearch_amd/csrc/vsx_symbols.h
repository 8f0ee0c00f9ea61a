// vsx_symbols.h -- the symbol maps of the reference (utils/maps.cpp) and the hash finaliser, stated once for host and device: a
// command's kernel and its host restatement agree bit for bit because both call these.
//
// Left alone on purpose:
//   sx_mix (vsx_sintax_internal.h)         restates the reference's random generator and changes with that, not with the hash tables
//   code_of (vsx_exact.hip)                a packed 64-bit constant lookup inside the hashing loop
//   vsx_mg_* (vsx_merge_internal.h)        other semantics: upper case only
//   two_bit (vsx_fastx_mask.hip)           a 2-bit code of its own
//   vsx_device.hip, vsx_kmer.hip, vsx_msa.hip, vsx_tbtext.h, vsx_accept.h      the DP and traceback kernels are tuned to the instruction
#ifndef VSX_SYMBOLS_H
#define VSX_SYMBOLS_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define VSX_SYM_HD __host__ __device__ inline
#else
#define VSX_SYM_HD inline
#endif

namespace vsxsym {

// the multipliers the hashes put in front of mix64: of a word's position, and of the length
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull, kLengthMul = 0xC2B2AE3D27D4EB4Full;

// splitmix64's finaliser
VSX_SYM_HD uint64_t mix64(uint64_t x)
{
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// chrmap_4bit: IUPAC in either case, U = T, every other byte 0
VSX_SYM_HD uint32_t map4(uint32_t c)
{
  //                      a  b   c  d   e  f  g  h   i  j  k   l  m  n   o  p  q  r  s  t  u  v  w  x  y   z
  const uint8_t t[26] = { 1, 14, 2, 13, 0, 0, 4, 11, 0, 0, 12, 0, 3, 15, 0, 0, 0, 5, 6, 8, 8, 7, 9, 0, 10, 0 };
  const uint32_t l = (c | 0x20u) - 'a';
  return l < 26u ? t[l] : 0u;
}

VSX_SYM_HD bool ambiguous4(uint32_t code) { return code != 1u && code != 2u && code != 4u && code != 8u; }      // chrmap_ambiguous_4bit

// chrmap_complement: the complement of A .. Z, case kept for the letters the table has in lower case, every other byte 'N'
VSX_SYM_HD uint32_t complement(uint32_t c)
{
  const char up[] = "TVGHNNCDNNMNKNNNNYSAABWNRN";
  if (c >= 'A' && c <= 'Z') return (unsigned char) up[c - 'A'];
  if (c >= 'a' && c <= 'z')
    {
      const uint32_t kept = 0x17E34CFu;                                 // bit (c - 'a') of: a b c d g h k m n r s t u v w y
      return ((kept >> (c - 'a')) & 1u) ? (unsigned char) (up[c - 'a'] | 0x20) : (unsigned char) 'N';
    }
  return (unsigned char) 'N';
}

// chrmap_upcase: a letter in upper case, 'N' for every other byte
VSX_SYM_HD uint32_t upcase(uint32_t c)
{
  const uint32_t u = (c | 0x20u) - 'a';
  return u < 26u ? (c & 0xDFu) : (uint32_t) 'N';
}

}  // namespace vsxsym

#endif
