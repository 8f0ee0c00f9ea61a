// vsx_devutil.h -- the wave and workgroup helpers the kernels share: 64-bit shuffles, butterfly reductions, the inclusive scans.
// Device code only, included by the .hip files alone.  A wave is 64 lanes (gfx950); every helper here holds shuffles, so ALL 64
// lanes of the wave must call it (no call under a divergent branch), and block_scan also holds barriers: all threads of the block.
// vsx_device.hip, vsx_kmer.hip, vsx_msa.hip and vsx_tbtext.h keep their own, tuned to the instruction.
#ifndef VSX_DEVUTIL_H
#define VSX_DEVUTIL_H

#include <hip/hip_runtime.h>

namespace vsxd {

typedef unsigned int u32;
typedef unsigned long long u64;

#define VSXD_DEV __device__ __forceinline__

VSXD_DEV u32 lane_id() { return threadIdx.x & 63u; }

// a 64-bit value of lane `src` / of the lane d below / of lane ^ m, as two 32-bit shuffles; all lanes call
VSXD_DEV u64 shfl64(u64 v, int src)
{
  const int lo = __shfl((int) (uint32_t) v, src), hi = __shfl((int) (uint32_t) (v >> 32), src);
  return ((u64) (uint32_t) hi << 32) | (uint32_t) lo;
}
VSXD_DEV u64 shfl_up64(u64 v, int d)
{
  const int lo = __shfl_up((int) (uint32_t) v, d), hi = __shfl_up((int) (uint32_t) (v >> 32), d);
  return ((u64) (uint32_t) hi << 32) | (uint32_t) lo;
}
VSXD_DEV u64 shfl_xor64(u64 v, int m)
{
  const int lo = __shfl_xor((int) (uint32_t) v, m), hi = __shfl_xor((int) (uint32_t) (v >> 32), m);
  return ((u64) (uint32_t) hi << 32) | (uint32_t) lo;
}

// the value of lane ^ m, for the types the reductions take
VSXD_DEV int lane_xor(int v, int m) { return __shfl_xor(v, m, 64); }
VSXD_DEV u32 lane_xor(u32 v, int m) { return (u32) __shfl_xor((int) v, m, 64); }
VSXD_DEV u64 lane_xor(u64 v, int m) { return shfl_xor64(v, m); }

// butterfly reductions over the wave (int, u32, u64): all lanes call, every lane returns the result
template <typename T>
VSXD_DEV T wave_sum(T v)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += lane_xor(v, m);
  return v;
}
template <typename T>
VSXD_DEV T wave_min(T v)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { const T o = lane_xor(v, m); v = o < v ? o : v; }
  return v;
}
template <typename T>
VSXD_DEV T wave_max(T v)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { const T o = lane_xor(v, m); v = o > v ? o : v; }
  return v;
}

// inclusive sum over the wave: lane i returns v of lanes 0 .. i; all lanes call
VSXD_DEV u32 wave_incl_sum(u32 v)
{
#pragma unroll
  for (int d = 1; d < 64; d <<= 1)
    {
      const u32 o = (u32) __shfl_up((int) v, d, 64);
      if ((int) lane_id() >= d) v += o;
    }
  return v;
}

// inclusive scan over a workgroup of WAVES waves; *total = the sum of all threads' values.  Every thread of the block calls (two
// barriers); s_wsum: WAVES words of LDS, free again on return
template <int WAVES>
VSXD_DEV u64 block_scan(u64 v, u64 * s_wsum, u64 * total)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1)
    {
      const u64 o = __shfl_up(v, d, 64);
      if (lane >= d) v += o;
    }
  if (lane == 63) s_wsum[wave] = v;
  __syncthreads();
  u64 pre = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) { if (w < wave) pre += s_wsum[w]; tot += s_wsum[w]; }
  __syncthreads();
  *total = tot;
  return v + pre;
}

#undef VSXD_DEV

}  // namespace vsxd

#endif
