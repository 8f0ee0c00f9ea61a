// vsx_fastx_mask.hip -- the kernels of vsx_fastx_mask (include/vsx_mask.h) on gfx950: DUST over TEXT by two routes, and the apply
// kernel that turns text + intervals into the masked text, the bitmap and the unmasked counts of all five modes.
//
//   window    dust_window() is vsx_mask.hip's window over text instead of 4-bit codes: lane = start offset, 64 one-byte 3-mer counters
//             per lane in LDS ([word][lane], as there), first maximum of 10 * pairs / j by the exact magic division, a wave reduction to
//             the maximum with the smallest start offset.  W(i) = (v, a, b) is a pure function of text[i, i + 64).
//   short     one wave per sequence walks the reference's window loop in order (mask.cpp:160-186).
//   long      W(i) at EVERY position i, one wave per position (all independent), stored as a dword with next(i) - i; then the chain
//             0, next(0), next(next(0)), ... is resolved by segments: one lane per (segment, entry offset) walks the stored steps to the
//             segment's end and records where it leaves; a serial pass over the segments picks each one's true entry; one wave per
//             segment re-walks from it and ORs the intervals of the chain's windows with v > 20 into the bitmap.  A step is
//             32 + (32 - b) with b >= 2 at most, so 64 entry offsets cover every way into a segment.  Integers only.
//   apply     lane = byte, 64 aligned bytes of the packed text per step; ballots and popcounts give the counts and the bitmap words.
#include <hip/hip_runtime.h>
#include "vsx_fastx_mask_internal.h"

typedef unsigned int u32;
typedef unsigned long long u64;

#define DW 64
#define DH 32
#define DLEVEL 20
#define EVAL_PER_WAVE 8

namespace {

struct MaskLds {
  uint8_t cnt[4][64 * 64];                             // [wave][word * 64 + lane]
  uint8_t tri[4][DW];
  u32 hist[4][64];                                     // 3-mer counts of the whole window
  u32 magic[64];                                       // ceil(2^32 / j)
};

__device__ __forceinline__ void lds_setup(MaskLds & l)
{
  if (threadIdx.x < 64)
    {
      const u32 j = threadIdx.x < 2 ? 2u : threadIdx.x;
      l.magic[threadIdx.x] = (u32) (0x100000000ull / j) + ((j & (j - 1u)) ? 1u : 0u);
    }
  __syncthreads();
}

// map_2bit (utils/maps.cpp): A 0, C 1, G 2, T 3, U 3, either case; everything else 0
__device__ __forceinline__ u32 two_bit(u32 c)
{
  c |= 0x20u;
  return c == 'c' ? 1u : c == 'g' ? 2u : (c == 't' || c == 'u') ? 3u : 0u;
}

// the best interval of the window of n <= 64 symbols at s, by the whole wave (every lane calls it); v = 0: none
// Only a score ABOVE the level matters to the callers, and 10 * pairs / j > 20 needs pairs >= 2.1 j while no interval holds more pairs
// of equal 3-mers than the whole window does (the sum over the words of c (c - 1) / 2): end offsets from 10 * total / 21 + 1 on can
// neither be the answer nor change it (the bound of vsx_mask.cpp's window_best).  Ordinary text walks a fifth of the end offsets.
__device__ __forceinline__ void dust_window(const uint8_t * __restrict__ s, int n, uint8_t * cnt, uint8_t * tri, u32 * hist, const u32 * magic,
                                            int lane, int & v, int & a, int & b)
{
  v = 0; a = 0; b = 0;
  const int starts = n - 7;                            // the smallest region has 8 symbols
  if (starts <= 0) return;
  {
    u32 t = 0;
#pragma unroll
    for (int x = 2; x >= 0; --x)
      {
        const u32 c = (lane - x >= 0 && lane < n) ? two_bit((u32) s[lane - x]) : 0u;
        t = (t << 2) | c;
      }
    tri[lane] = (uint8_t) t;
    hist[lane] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane >= 2 && lane < n) atomicAdd(&hist[t], 1u);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  int jlim;
  {
    const u32 c = hist[lane];
    u32 total = c * (c - 1u) / 2u;                     // (c = 0 gives 0: the product wraps to 0 - 0)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) total += (u32) __shfl_xor((int) total, d, 64);
    jlim = (int) (10u * total / (u32) (DLEVEL + 1)) + 1;            // exclusive
  }
  if (jlim <= 2) return;
#pragma unroll 8
  for (int w = 0; w < 64; ++w) cnt[w * 64 + lane] = 0;
  // (each lane reads tri[] of the other lanes, written before the barriers above, and only its own counters)
  int best = 0, bj = 0;
  if (lane < starts)
    {
      int pairs = 0;
      const int jn = n - lane < jlim ? n - lane : jlim;
      for (int j = 2; j < jn; ++j)
        {
          const u32 w = tri[lane + j];
          uint8_t * c = cnt + w * 64 + lane;
          const u32 cv = *c;
          if (cv)
            {
              pairs += (int) cv;
              const int x = (int) __umulhi((u32) (10 * pairs), magic[j]);
              if (x > best) { best = x; bj = j; }
            }
          *c = (uint8_t) (cv + 1u);
        }
    }
  u32 key = ((u32) best << 6) | (u32) (63 - lane);     // maximum score, smallest start offset
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1)
    {
      const u32 o = (u32) __shfl_xor((int) key, d, 64);
      key = o > key ? o : key;
    }
  const int wi = 63 - (int) (key & 63u);
  const int wj = __shfl(bj, wi, 64);
  v = (int) (key >> 6); a = wi; b = wi + wj;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");          // the next window rewrites tri[] and the counters
  __builtin_amdgcn_wave_barrier();
}

__global__ void __launch_bounds__(256)
mask_short_kernel(const uint8_t * __restrict__ text, const u64 * __restrict__ off, const u32 * __restrict__ len, const u32 * __restrict__ list,
                  u32 n_list, u32 * __restrict__ dbits, u64 * __restrict__ counter)
{
  __shared__ MaskLds lds;
  lds_setup(lds);
  const int lane = (int) (threadIdx.x & 63), wave = (int) (threadIdx.x >> 6);
  const u32 item = blockIdx.x * 4 + wave;
  if (item >= n_list) return;
  const u32 seq = list[item];
  const u64 base = off[seq];
  const uint8_t * __restrict__ s = text + base;
  const long L = (long) len[seq];
  u32 visited = 0;
  for (long i0 = 0; i0 < L; i0 += DH)
    {
      const int n = (int) (L > i0 + DW ? DW : L - i0);
      int v, a, b;
      dust_window(s + i0, n, lds.cnt[wave], lds.tri[wave], lds.hist[wave], lds.magic, lane, v, a, b);
      ++visited;
      if (v > DLEVEL)
        {
          if (a + lane <= b)
            {
              const u64 bit = base + (u64) (i0 + a + lane);
              atomicOr(&dbits[bit >> 5], 1u << (u32) (bit & 31u));
            }
          if (b < DH) i0 += DH - b;
        }
    }
  if (lane == 0 && visited) atomicAdd(counter, (u64) visited);
}

__global__ void __launch_bounds__(256)
mask_eval_kernel(const uint8_t * __restrict__ s, u32 L, u32 c0, u32 npos, u32 * __restrict__ wout)
{
  __shared__ MaskLds lds;
  lds_setup(lds);
  const int lane = (int) (threadIdx.x & 63), wave = (int) (threadIdx.x >> 6);
  const u64 first = ((u64) blockIdx.x * 4 + (u64) wave) * EVAL_PER_WAVE;
  for (int k = 0; k < EVAL_PER_WAVE; ++k)
    {
      const u64 r = first + (u64) k;
      if (r >= (u64) npos) break;
      const u32 i = c0 + (u32) r;                      // < L
      const int n = (int) (L - i > (u32) DW ? (u32) DW : L - i);
      int v, a, b;
      dust_window(s + i, n, lds.cnt[wave], lds.tri[wave], lds.hist[wave], lds.magic, lane, v, a, b);
      const bool masked = v > DLEVEL;
      const u32 step = (u32) DH + ((masked && b < DH) ? (u32) (DH - b) : 0u);
      if (lane == 0) wout[r] = step | ((u32) a << 6) | ((u32) b << 12) | (masked ? 1u << 18 : 0u);
    }
}

// one lane per (segment, entry offset): where a chain that enters the segment at that offset leaves it, as an offset into the next one
__global__ void __launch_bounds__(256)
mask_segwalk_kernel(const u32 * __restrict__ w, u32 c0, u32 npos, u32 S, u32 nseg, uint8_t * __restrict__ exits)
{
  const u64 t = (u64) blockIdx.x * 256 + threadIdx.x;
  if (t >= (u64) nseg * VSX_MASK_ENTRIES) return;
  const u32 seg = (u32) (t / VSX_MASK_ENTRIES), e = (u32) (t % VSX_MASK_ENTRIES);
  const u64 start = (u64) seg * S;                                 // positions relative to c0
  const u64 end = start + S < (u64) npos ? start + S : (u64) npos;
  u64 p = start + e;
  while (p < end) p += VSX_MASK_W_STEP(w[p]);
  exits[t] = (uint8_t) (p - end);
}

// the true entry of every segment, in order; *entry: the chain's offset into this chunk on entry, into the next chunk on return
__global__ void mask_resolve_kernel(const uint8_t * __restrict__ exits, u32 nseg, uint8_t * __restrict__ true_entry, u32 * __restrict__ entry)
{
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  u32 e = *entry;
  for (u32 seg = 0; seg < nseg; ++seg)
    {
      true_entry[seg] = (uint8_t) e;
      e = exits[(u64) seg * VSX_MASK_ENTRIES + e];
    }
  *entry = e;
}

// one wave per segment: the chain from the true entry; the intervals of its windows with v > 20 go into the bitmap
__global__ void __launch_bounds__(256)
mask_mark_kernel(const u32 * __restrict__ w, u32 c0, u32 npos, u32 S, u32 nseg, const uint8_t * __restrict__ true_entry,
                 u32 * __restrict__ dbits, u64 bit0)
{
  const int lane = (int) (threadIdx.x & 63);
  const u32 seg = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (seg >= nseg) return;
  const u64 start = (u64) seg * S;
  const u64 end = start + S < (u64) npos ? start + S : (u64) npos;
  u64 p = start + true_entry[seg];
  while (p < end)
    {
      const u32 x = w[p];
      if (VSX_MASK_W_MASKED(x))
        {
          const u32 a = VSX_MASK_W_A(x), b = VSX_MASK_W_B(x);
          if (a + (u32) lane <= b)
            {
              const u64 bit = bit0 + (u64) c0 + p + a + (u64) lane;
              atomicOr(&dbits[bit >> 5], 1u << (u32) (bit & 31u));
            }
        }
      p += VSX_MASK_W_STEP(x);
    }
}

// packed positions [lo, hi) by one wave; returns the unmasked count (uniform)
__device__ __forceinline__ u32 apply_range(const uint8_t * __restrict__ text, u64 lo, u64 hi, int qmask, int hard, const u32 * __restrict__ dbits,
                                           uint8_t * __restrict__ out, u64 * __restrict__ obits, int lane)
{
  u32 count = 0;
  for (u64 blk = lo & ~(u64) 63; blk < hi; blk += 64)
    {
      const u64 p = blk + (u64) lane;
      const bool act = p >= lo && p < hi;
      const u32 c = act ? (u32) text[p] : 0u;
      u32 o = c;
      if (qmask == 2)
        {
          const bool in = act && ((dbits[p >> 5] >> (u32) (p & 31u)) & 1u);
          if (hard) o = in ? (u32) 'N' : c;
          else o = in ? (c | 0x20u) : ((c >= 'a' && c <= 'z') ? c - 32u : c);
        }
      else if (qmask == 1 && hard) o = (c & 0x20u) ? (u32) 'N' : c;
      const bool counts = qmask == 0 ? true : hard ? o != (u32) 'N' : (o >= 'A' && o <= 'Z');
      count += (u32) __popcll(__ballot(act && counts));
      const u64 m = __ballot(act && !counts);
      if (out && act) out[p] = (uint8_t) o;
      if (obits && lane == 0 && m) atomicOr(&obits[blk >> 6], m);      // a boundary word is shared with the neighbouring sequence
    }
  return count;
}

__global__ void __launch_bounds__(256)
mask_apply_kernel(const uint8_t * __restrict__ text, const u64 * __restrict__ off, const u32 * __restrict__ len, u32 n, int qmask, int hard,
                  const u32 * __restrict__ dbits, uint8_t * __restrict__ out, u64 * __restrict__ obits, u32 * __restrict__ unmasked)
{
  const int lane = (int) (threadIdx.x & 63);
  const u32 k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= n) return;
  const u32 L = len[k];
  if (L > VSX_MASK_APPLY_WHOLE) return;                // mask_apply_long_kernel adds this one up
  const u64 lo = off[k];
  const u32 count = apply_range(text, lo, lo + L, qmask, hard, dbits, out, obits, lane);
  if (lane == 0) unmasked[k] = count;
}

__global__ void __launch_bounds__(256)
mask_apply_long_kernel(const uint8_t * __restrict__ text, u64 off, u32 L, u32 k, int qmask, int hard, const u32 * __restrict__ dbits,
                       uint8_t * __restrict__ out, u64 * __restrict__ obits, u32 * __restrict__ unmasked)
{
  const int lane = (int) (threadIdx.x & 63);
  const u64 tile = (u64) blockIdx.x * 4 + (threadIdx.x >> 6);
  const u64 t0 = tile * VSX_MASK_APPLY_TILE;
  if (t0 >= (u64) L) return;
  const u64 t1 = t0 + VSX_MASK_APPLY_TILE < (u64) L ? t0 + VSX_MASK_APPLY_TILE : (u64) L;
  const u32 count = apply_range(text, off + t0, off + t1, qmask, hard, dbits, out, obits, lane);
  if (lane == 0 && count) atomicAdd(&unmasked[k], count);
}

}  // namespace

extern "C" {

hipError_t vsx_launch_mask_short(const uint8_t * d_text, const uint64_t * d_off, const uint32_t * d_len, const uint32_t * d_list, uint32_t n_list,
                                 uint32_t * d_dbits, unsigned long long * d_counter, hipStream_t st)
{
  if (n_list == 0) return hipSuccess;
  hipLaunchKernelGGL(mask_short_kernel, dim3((n_list + 3) / 4), dim3(256), 0, st, d_text, (const u64 *) d_off, d_len, d_list, n_list, d_dbits, d_counter);
  return hipGetLastError();
}

hipError_t vsx_launch_mask_eval(const uint8_t * d_seq, uint32_t L, uint32_t c0, uint32_t npos, uint32_t * d_w, hipStream_t st)
{
  if (npos == 0) return hipSuccess;
  const uint32_t per_block = 4 * EVAL_PER_WAVE;
  hipLaunchKernelGGL(mask_eval_kernel, dim3((npos + per_block - 1) / per_block), dim3(256), 0, st, d_seq, L, c0, npos, d_w);
  return hipGetLastError();
}

hipError_t vsx_launch_mask_chain(const uint32_t * d_w, uint32_t L, uint32_t c0, uint32_t npos, uint32_t S, uint8_t * d_exit, uint8_t * d_true,
                                 uint32_t * d_entry, uint32_t * d_dbits, uint64_t bit0, hipStream_t st)
{
  (void) L;
  if (npos == 0) return hipSuccess;
  const uint32_t nseg = (uint32_t) (((uint64_t) npos + S - 1) / S);
  const uint64_t lanes = (uint64_t) nseg * VSX_MASK_ENTRIES;
  hipLaunchKernelGGL(mask_segwalk_kernel, dim3((unsigned) ((lanes + 255) / 256)), dim3(256), 0, st, d_w, c0, npos, S, nseg, d_exit);
  hipLaunchKernelGGL(mask_resolve_kernel, dim3(1), dim3(64), 0, st, d_exit, nseg, d_true, d_entry);
  hipLaunchKernelGGL(mask_mark_kernel, dim3((nseg + 3) / 4), dim3(256), 0, st, d_w, c0, npos, S, nseg, d_true, d_dbits, (u64) bit0);
  return hipGetLastError();
}

hipError_t vsx_launch_mask_apply(const uint8_t * d_text, const uint64_t * d_off, const uint32_t * d_len, uint32_t n, int qmask, int hard,
                                 const uint32_t * d_dbits, uint8_t * d_out, unsigned long long * d_obits, uint32_t * d_unmasked, hipStream_t st)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(mask_apply_kernel, dim3((n + 3) / 4), dim3(256), 0, st, d_text, (const u64 *) d_off, d_len, n, qmask, hard, d_dbits, d_out,
                     (u64 *) d_obits, d_unmasked);
  return hipGetLastError();
}

hipError_t vsx_launch_mask_apply_long(const uint8_t * d_text, uint64_t off, uint32_t len, uint32_t k, int qmask, int hard,
                                      const uint32_t * d_dbits, uint8_t * d_out, unsigned long long * d_obits, uint32_t * d_unmasked, hipStream_t st)
{
  const uint64_t tiles = ((uint64_t) len + VSX_MASK_APPLY_TILE - 1) / VSX_MASK_APPLY_TILE;
  if (tiles == 0) return hipSuccess;
  hipLaunchKernelGGL(mask_apply_long_kernel, dim3((unsigned) ((tiles + 3) / 4)), dim3(256), 0, st, d_text, (u64) off, len, k, qmask, hard, d_dbits, d_out,
                     (u64 *) d_obits, d_unmasked);
  return hipGetLastError();
}

}  // extern "C"
