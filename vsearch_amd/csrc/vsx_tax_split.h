// vsx_tax_split.h -- tax_parse + tax_split of the reference (core/tax.cpp:70-186), restated once for vsx_sintax.cpp and vsx_lca.cpp:
// where the nine rank names lie in a header.  Host-only C++.  This is the specification of the split, quirks included: the loop
// bound `offset < hlen - 4`, the `offset += 5` skip after a tax= that no ';' precedes, a later field of a rank overwriting an
// earlier one, the comma search that is not bounded by the end of the tax= field, tolower on the rank letter.
//
// The header is the span h[0 .. hlen): it holds no NUL, and every search ends at hlen as the reference's strstr / strchr end at the
// terminator.  A NUL-terminated header with hlen = strlen(h) gives what the reference gives.
#ifndef VSX_TAX_SPLIT_H
#define VSX_TAX_SPLIT_H

#include <cctype>
#include <cstring>

namespace vsxtax {

constexpr int kLevels = 9;
constexpr char kRanks[] = "dkpcofgst";

// strchr(h + from, c) - h, or -1
inline int find_byte(const char * h, int from, int hlen, char c)
{
  if (from >= hlen) return -1;
  const void * p = std::memchr(h + from, c, (size_t) (hlen - from));
  return p ? (int) (static_cast<const char *>(p) - h) : -1;
}

// strstr(h + from, "tax=") - h, or -1
inline int find_tax(const char * h, int from, int hlen)
{
  for (int p = from; p + 4 <= hlen; ++p)
    {
      p = find_byte(h, p, hlen - 3, 't');
      if (p < 0) return -1;
      if (h[p + 1] == 'a' && h[p + 2] == 'x' && h[p + 3] == '=') return p;
    }
  return -1;
}

// the level of a rank letter, or -1
inline int level_of(unsigned char c)
{
  const char * r = static_cast<const char *>(std::memchr(kRanks, std::tolower(c), (size_t) kLevels));
  return r ? (int) (r - kRanks) : -1;
}

// start/len stay 0 for a rank the header does not name
inline void tax_split(const char * h, int hlen, int * start, int * len)
{
  for (int k = 0; k < kLevels; ++k) start[k] = len[k] = 0;
  int tax_start = 0, tax_end = 0;
  bool found = false;
  int offset = 0;
  while (offset < hlen - 4)
    {
      const int p = find_tax(h, offset, hlen);
      if (p < 0) break;
      offset = p;
      if (offset > 0 && h[offset - 1] != ';') { offset += 5; continue; }
      tax_start = offset;
      const int e = find_byte(h, offset + 4, hlen, ';');
      tax_end = e >= 0 ? e : hlen;
      found = true;
      break;
    }
  if (!found) return;
  offset = tax_start + 4;
  while (offset < tax_end)
    {
      const int level = level_of((unsigned char) h[offset]);
      if (level >= 0 && offset + 1 < hlen && h[offset + 1] == ':')
        {
          start[level] = offset + 2;
          const int comma = find_byte(h, offset + 2, hlen, ',');        // not bounded by the end of the field
          len[level] = comma >= 0 ? comma - offset - 2 : tax_end - offset - 2;
        }
      const int comma = find_byte(h, offset, hlen, ',');
      offset = comma >= 0 ? comma + 1 : tax_end;
    }
}

}  // namespace vsxtax

#endif
