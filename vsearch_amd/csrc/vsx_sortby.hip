// vsx_sortby.hip -- the reference's sort orders on gfx950 (--sortbysize, --sortbylength; include/vsx_sortby.h).
//
// The order is (numeric key, header by strcmp, input position).  The numeric key is one 64-bit word; the header is compared in
// rounds of eight bytes.  Every round is the same step over the records whose place is still open (vsx_sortby_internal.h):
//
//   key        numeric round: the key word (descending fields complemented).  Label round r: bytes [8r, 8r + 8) of the header,
//              first byte highest, zero beyond the header's end -- a lane per record, byte loads, none beyond the header (so none
//              beyond the blob).  Headers hold no NUL (the host refuses them), so a shorter header sorts first.
//   sort       rocPRIM's stable radix sort by the key, then (label rounds) by the group start g: stable, so equal (g, key) keep
//              the order they had, which is input order from the first compaction on.
//   place      the index of a group's first record by an inclusive maximum over marks; position = g + index in the group; the
//              item goes to order[position].  A new group begins where g or the key changes; its start is again an inclusive
//              maximum, over the positions at those marks (positions rise along the array).
//   open       a record stays for the next round when its new group has a second member and -- label rounds -- the key does not
//              end in a zero byte: then every member has ended and they are equal, already in input order.
//   compact    rocPRIM's exclusive sum over the open flags; the open records move up in order.
//
// Integer code, no atomics, a lane per record, no LDS of its own: two calls give identical bytes.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include "../../include/vsx_sortby.h"
#include "vsx_sortby_internal.h"

namespace {

typedef unsigned long long u64;
typedef uint32_t u32;

#define SORTBY_THREADS 256

__global__ __launch_bounds__(SORTBY_THREADS)
void vsx_sortby_select_kernel(u32 n, int order, long long minsize, long long maxsize, const u32 * __restrict__ size, u32 * __restrict__ keep)
{
  const u32 i = blockIdx.x * SORTBY_THREADS + threadIdx.x;
  if (i >= n) return;
  const long long s = (long long) size[i];
  keep[i] = (order != VSX_SORTBY_SIZE || (s >= minsize && s <= maxsize)) ? 1u : 0u;
}

__global__ __launch_bounds__(SORTBY_THREADS)
void vsx_sortby_keys_kernel(u32 n, int order, const u32 * __restrict__ seqlen, const u32 * __restrict__ size, const u32 * __restrict__ keep,
                            const u32 * __restrict__ slot, u32 * __restrict__ item, u64 * __restrict__ key, u32 * __restrict__ g)
{
  const u32 i = blockIdx.x * SORTBY_THREADS + threadIdx.x;
  if (i >= n || !keep[i]) return;
  const u32 j = slot[i];
  const u64 by_size = (u64) (~size[i]);
  u64 k = by_size;
  if (order == VSX_SORTBY_LENGTH) k = ((u64) (~seqlen[i]) << 32) | by_size;
  else if (order == VSX_SORTBY_LENGTH_ASC) k = ((u64) seqlen[i] << 32) | by_size;
  item[j] = i; key[j] = k; g[j] = 0u;
}

__global__ __launch_bounds__(SORTBY_THREADS)
void vsx_sortby_iota_kernel(u32 m, u32 * __restrict__ idx)
{
  const u32 a = blockIdx.x * SORTBY_THREADS + threadIdx.x;
  if (a < m) idx[a] = a;
}

__global__ __launch_bounds__(SORTBY_THREADS)
void vsx_sortby_chunk_kernel(u32 m, u32 round, const uint8_t * __restrict__ blob, const u64 * __restrict__ off, const u32 * __restrict__ len,
                             const u32 * __restrict__ item, u64 * __restrict__ chunk)
{
  const u32 a = blockIdx.x * SORTBY_THREADS + threadIdx.x;
  if (a >= m) return;
  const u32 i = item[a], L = len[i];
  const u64 first = (u64) round * 8u;
  u64 c = 0;
  if (first < (u64) L)
    {
      const uint8_t * p = blob + off[i] + first;
      const u32 have = (u32) min((u64) 8, (u64) L - first);
#pragma unroll
      for (u32 b = 0; b < 8u; ++b) c = (c << 8) | (b < have ? (u64) p[b] : 0ull);
    }
  chunk[a] = c;
}

__global__ __launch_bounds__(SORTBY_THREADS)
void vsx_sortby_gather32_kernel(u32 m, const u32 * __restrict__ in, const u32 * __restrict__ idx, u32 * __restrict__ out)
{
  const u32 a = blockIdx.x * SORTBY_THREADS + threadIdx.x;
  if (a < m) out[a] = in[idx[a]];
}

__global__ __launch_bounds__(SORTBY_THREADS)
void vsx_sortby_gather_kernel(u32 m, const u32 * __restrict__ idx, const u64 * __restrict__ chunk, const u32 * __restrict__ item,
                              const u32 * __restrict__ g2, u64 * __restrict__ chunk2, u32 * __restrict__ item2, u32 * __restrict__ first)
{
  const u32 a = blockIdx.x * SORTBY_THREADS + threadIdx.x;
  if (a >= m) return;
  const u32 from = idx[a];
  chunk2[a] = chunk[from];
  item2[a] = item[from];
  first[a] = (a > 0u && g2[a] != g2[a - 1u]) ? a : 0u;
}

__global__ __launch_bounds__(SORTBY_THREADS)
void vsx_sortby_place_kernel(u32 m, const u32 * __restrict__ g2, const u32 * __restrict__ first, const u64 * __restrict__ chunk2,
                             const u32 * __restrict__ item2, u32 * __restrict__ order, u32 * __restrict__ mark)
{
  const u32 a = blockIdx.x * SORTBY_THREADS + threadIdx.x;
  if (a >= m) return;
  const u32 p = g2[a] + (a - first[a]);
  order[p] = item2[a];
  const bool head = a == first[a] || chunk2[a] != chunk2[a - 1u];
  mark[a] = head ? p : 0u;
}

__global__ __launch_bounds__(SORTBY_THREADS)
void vsx_sortby_open_kernel(u32 m, int label_round, const u32 * __restrict__ ng, const u64 * __restrict__ chunk2, u32 * __restrict__ open)
{
  const u32 a = blockIdx.x * SORTBY_THREADS + threadIdx.x;
  if (a >= m) return;
  const u32 mine = ng[a];
  const bool alone = (a == 0u || ng[a - 1u] != mine) && (a + 1u == m || ng[a + 1u] != mine);
  const bool ended = label_round && (chunk2[a] & 0xFFull) == 0ull;
  open[a] = (alone || ended) ? 0u : 1u;
}

__global__ __launch_bounds__(SORTBY_THREADS)
void vsx_sortby_compact_kernel(u32 m, const u32 * __restrict__ open, const u32 * __restrict__ slot, const u32 * __restrict__ item2,
                               const u32 * __restrict__ ng, u32 * __restrict__ item, u32 * __restrict__ g)
{
  const u32 a = blockIdx.x * SORTBY_THREADS + threadIdx.x;
  if (a >= m || !open[a]) return;
  const u32 j = slot[a];
  item[j] = item2[a];
  g[j] = ng[a];
}

inline dim3 grid_of(u32 count) { return dim3((u32) (((u64) count + SORTBY_THREADS - 1u) / SORTBY_THREADS)); }

}  // namespace

extern "C" hipError_t vsx_launch_sortby_scan_sum(void * temp, size_t * temp_bytes, const uint32_t * d_in, uint32_t * d_out, uint64_t count, hipStream_t st)
{
  return rocprim::exclusive_scan(temp, *temp_bytes, d_in, d_out, (uint32_t) 0, (size_t) count, rocprim::plus<uint32_t>(), st);
}

extern "C" hipError_t vsx_launch_sortby_scan_max(void * temp, size_t * temp_bytes, const uint32_t * d_in, uint32_t * d_out, uint64_t count, hipStream_t st)
{
  return rocprim::inclusive_scan(temp, *temp_bytes, d_in, d_out, (size_t) count, rocprim::maximum<uint32_t>(), st);
}

extern "C" hipError_t vsx_launch_sortby_sort64(void * temp, size_t * temp_bytes, const unsigned long long * d_kin, unsigned long long * d_kout,
                                               const uint32_t * d_vin, uint32_t * d_vout, uint64_t count, uint32_t end_bit, hipStream_t st)
{
  if (end_bit == 0 || end_bit > 64) return hipErrorInvalidValue;
  return rocprim::radix_sort_pairs(temp, *temp_bytes, d_kin, d_kout, d_vin, d_vout, (size_t) count, 0u, end_bit, st);
}

extern "C" hipError_t vsx_launch_sortby_sort32(void * temp, size_t * temp_bytes, const uint32_t * d_kin, uint32_t * d_kout, const uint32_t * d_vin,
                                               uint32_t * d_vout, uint64_t count, uint32_t end_bit, hipStream_t st)
{
  if (end_bit == 0 || end_bit > 32) return hipErrorInvalidValue;
  return rocprim::radix_sort_pairs(temp, *temp_bytes, d_kin, d_kout, d_vin, d_vout, (size_t) count, 0u, end_bit, st);
}

extern "C" hipError_t vsx_launch_sortby_select(uint32_t n, int order, long long minsize, long long maxsize, const uint32_t * d_size, uint32_t * d_keep,
                                               hipStream_t st)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_sortby_select_kernel, grid_of(n), dim3(SORTBY_THREADS), 0, st, n, order, minsize, maxsize, d_size, d_keep);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_sortby_keys(uint32_t n, int order, const uint32_t * d_seqlen, const uint32_t * d_size, const uint32_t * d_keep,
                                             const uint32_t * d_slot, uint32_t * d_item, unsigned long long * d_key, uint32_t * d_g, hipStream_t st)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_sortby_keys_kernel, grid_of(n), dim3(SORTBY_THREADS), 0, st, n, order, d_seqlen, d_size, d_keep, d_slot, d_item, d_key, d_g);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_sortby_iota(uint32_t m, uint32_t * d_idx, hipStream_t st)
{
  if (m == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_sortby_iota_kernel, grid_of(m), dim3(SORTBY_THREADS), 0, st, m, d_idx);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_sortby_chunk(uint32_t m, uint32_t round, const uint8_t * d_blob, const uint64_t * d_off, const uint32_t * d_len,
                                              const uint32_t * d_item, unsigned long long * d_chunk, hipStream_t st)
{
  if (m == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_sortby_chunk_kernel, grid_of(m), dim3(SORTBY_THREADS), 0, st, m, round, d_blob, (const u64 *) d_off, d_len, d_item, d_chunk);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_sortby_gather32(uint32_t m, const uint32_t * d_in, const uint32_t * d_idx, uint32_t * d_out, hipStream_t st)
{
  if (m == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_sortby_gather32_kernel, grid_of(m), dim3(SORTBY_THREADS), 0, st, m, d_in, d_idx, d_out);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_sortby_gather(uint32_t m, const uint32_t * d_idx, const unsigned long long * d_chunk, const uint32_t * d_item,
                                               const uint32_t * d_g2, unsigned long long * d_chunk2, uint32_t * d_item2, uint32_t * d_first,
                                               hipStream_t st)
{
  if (m == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_sortby_gather_kernel, grid_of(m), dim3(SORTBY_THREADS), 0, st, m, d_idx, d_chunk, d_item, d_g2, d_chunk2, d_item2, d_first);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_sortby_place(uint32_t m, const uint32_t * d_g2, const uint32_t * d_first, const unsigned long long * d_chunk2,
                                              const uint32_t * d_item2, uint32_t * d_order, uint32_t * d_mark, hipStream_t st)
{
  if (m == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_sortby_place_kernel, grid_of(m), dim3(SORTBY_THREADS), 0, st, m, d_g2, d_first, d_chunk2, d_item2, d_order, d_mark);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_sortby_open(uint32_t m, int label_round, const uint32_t * d_ng, const unsigned long long * d_chunk2, uint32_t * d_open,
                                             hipStream_t st)
{
  if (m == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_sortby_open_kernel, grid_of(m), dim3(SORTBY_THREADS), 0, st, m, label_round, d_ng, d_chunk2, d_open);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_sortby_compact(uint32_t m, const uint32_t * d_open, const uint32_t * d_slot, const uint32_t * d_item2,
                                                const uint32_t * d_ng, uint32_t * d_item, uint32_t * d_g, hipStream_t st)
{
  if (m == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_sortby_compact_kernel, grid_of(m), dim3(SORTBY_THREADS), 0, st, m, d_open, d_slot, d_item2, d_ng, d_item, d_g);
  return hipGetLastError();
}
