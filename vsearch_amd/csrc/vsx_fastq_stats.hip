// vsx_fastq_stats.hip -- read summary statistics on gfx950: the walks of --fastq_stats and --fastq_chars.
//
// Both kernels have the layout of the eestats walk (vsx_eestats.hip): one lane per read, 256 reads per workgroup, 64 positions
// at a time; each wave brings its reads' bytes into LDS with one coalesced 64-byte load per read, then every lane walks its own
// row with its state (running expected error, lowest score, current run) carried in registers from tile to tile.
//
//   stats walk  counts the quality character in a workgroup-private LDS histogram flushed once per tile, adds the tabulated error
//               to the running double `ee` and stores it into matrix[position][read] for the ordered-sum kernel of vsx_eestats.hip.
//               "lowest score so far > t" and "ee <= t" both hold on a prefix of a read and never come back (the minimum only
//               falls, ee only grows: every addend is >= 0), so a lane counts the positions at which each holds -- the length of
//               that prefix, found with the reference's comparisons in position order -- and adds one count to a histogram of
//               prefix lengths, equal lengths combined inside the wave.  The host forms the tables with a suffix sum.
//   chars       private counters for A C G T N, reduced per wave at the end; other letters and the quality characters through LDS
//               atomics, flushed per tile.  A run is recorded only when it ends with a count above zero; the tail is the run of
//               equal quality characters the read ends with.
//
// Only integer atomics, no flags, tickets or cooperative launches; stores are ordinary vector stores.  Built with
// -ffp-contract=off and without fast-math: ee += pe and the comparisons are the IEEE double operations of the reference.
#include <hip/hip_runtime.h>
#include "vsx_fastq_stats_internal.h"
#include "vsx_devutil.h"

namespace {

using vsxd::wave_sum;

constexpr int ROW_BYTES = VSX_FQS_ROW_WORDS * 4;

// each wave loads the tile rows of its own 64 reads: row r is the read of lane r
__device__ __forceinline__ void load_rows(uint8_t * wave_rows, const uint8_t * __restrict__ blob, uint32_t off, int full, int c, int lane)
{
  for (int r = 0; r < 64; ++r)
    {
      const uint32_t roff = (uint32_t) __builtin_amdgcn_readlane((int) off, r);
      const int rlen = __builtin_amdgcn_readlane(full, r);
      if (c >= rlen) continue;
      const int sym = c + lane < rlen ? (int) blob[(size_t) roff + c + lane] : 0;
      wave_rows[r * ROW_BYTES + lane] = (uint8_t) sym;
    }
}

__global__ __launch_bounds__(VSX_FQS_THREADS)
void vsx_fastq_stats_walk_kernel(const VsxEestatsItem * __restrict__ items, uint32_t n_items, const uint8_t * __restrict__ qual,
                                 VsxFastqStatsParams P, uint32_t * __restrict__ minmax)
{
  __shared__ double s_q2e[256];
  __shared__ uint32_t s_tile[VSX_FQS_THREADS * VSX_FQS_ROW_WORDS];
  __shared__ uint32_t s_sc[VSX_FQS_TILE * VSX_FQS_SYMS];
  __shared__ int s_maxlen;

  const int t = threadIdx.x, lane = t & 63;
  s_q2e[t] = P.q2e[t];
  if (t == 0) s_maxlen = 0;
  __syncthreads();

  const uint32_t read = blockIdx.x * VSX_FQS_THREADS + t;
  VsxEestatsItem it { 0, 0 };
  if (read < n_items) it = items[read];
  const int full = (int) it.len;
  atomicMax(&s_maxlen, full);
  __syncthreads();
  const int maxlen = __builtin_amdgcn_readfirstlane(s_maxlen);

  uint8_t * const tile = reinterpret_cast<uint8_t *>(s_tile);
  uint8_t * const wave_rows = tile + (size_t) (t - lane) * ROW_BYTES;
  const uint8_t * const my_row = tile + (size_t) t * ROW_BYTES;

  int low = 255, high = 0;                 // quality characters
  int lowest = 0x7fffffff;                 // score
  double ee = 0.0;
  uint32_t ee_prefix[4] = { 0, 0, 0, 0 }, q_prefix[4] = { 0, 0, 0, 0 };

  for (int c = 0; c < maxlen; c += VSX_FQS_TILE)
    {
      const int jn = maxlen - c < VSX_FQS_TILE ? maxlen - c : VSX_FQS_TILE;
      for (int k = t; k < jn * VSX_FQS_SYMS; k += VSX_FQS_THREADS) s_sc[k] = 0;
      load_rows(wave_rows, qual, it.off, full, c, lane);
      __syncthreads();

      const int mine = full - c < jn ? full - c : jn;
      for (int j = 0; j < mine; ++j)
        {
          const int sym = (int) my_row[j];
          low = sym < low ? sym : low;
          high = sym > high ? sym : high;
          const int column = sym - VSX_FQS_FIRST;
          // (a character outside 33 ... 126 fails the call on the host; it must not leave the histogram here)
          if ((unsigned) column < (unsigned) VSX_FQS_SYMS) atomicAdd(&s_sc[j * VSX_FQS_SYMS + column], 1u);
          const int score = sym < P.ascii ? 0 : sym - P.ascii;
          lowest = score < lowest ? score : lowest;
          q_prefix[0] += lowest > 5; q_prefix[1] += lowest > 10; q_prefix[2] += lowest > 15; q_prefix[3] += lowest > 20;
          ee += s_q2e[sym];
          P.matrix[(size_t) (c + j) * P.stride + read] = ee;
          ee_prefix[0] += ee <= 1.0; ee_prefix[1] += ee <= 0.5; ee_prefix[2] += ee <= 0.25; ee_prefix[3] += ee <= 0.1;
        }
      __syncthreads();
      // (c + j) * 94 + column == c * 94 + k
      uint32_t * const dst = P.symbol_counts + (size_t) c * VSX_FQS_SYMS;
      for (int k = t; k < jn * VSX_FQS_SYMS; k += VSX_FQS_THREADS)
        if (s_sc[k]) atomicAdd(&dst[k], s_sc[k]);
      __syncthreads();
    }

  // one count per read and threshold into the histogram of prefix lengths (each <= the read's length <= len_max)
  const bool have = read < n_items;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    {
      const uint32_t v = k < 4 ? ee_prefix[k] : q_prefix[k - 4];
      uint32_t * const row = P.prefix_hist + (size_t) k * (P.len_max + 1);
      unsigned long long todo = __ballot(have);
      while (todo)
        {
          const int leader = __ffsll(todo) - 1;
          const uint32_t x = (uint32_t) __builtin_amdgcn_readlane((int) v, leader);
          const unsigned long long same = __ballot(have && v == x);
          if (lane == leader) atomicAdd(&row[x], (uint32_t) __popcll(same));
          todo &= ~same;
        }
    }
  if (have) minmax[read] = full ? (uint32_t) low | (uint32_t) high << 8 : VSX_FQS_NO_SYMBOL;
}

__global__ __launch_bounds__(VSX_FQS_THREADS)
void vsx_fastq_chars_kernel(const VsxEestatsItem * __restrict__ items, uint32_t n_items, const uint8_t * __restrict__ seq,
                            const uint8_t * __restrict__ qual, uint32_t tail, VsxFastqCharsAcc * __restrict__ acc, uint32_t * __restrict__ err)
{
  __shared__ uint32_t s_seq_tile[VSX_FQS_THREADS * VSX_FQS_ROW_WORDS];
  __shared__ uint32_t s_qual_tile[VSX_FQS_THREADS * VSX_FQS_ROW_WORDS];
  __shared__ uint32_t s_qual[VSX_FQS_SYMS], s_tail[VSX_FQS_SYMS], s_other[26];
  __shared__ int s_maxrun[26];
  __shared__ uint32_t s_nmin, s_nmax;
  __shared__ int s_maxlen;

  const int t = threadIdx.x, lane = t & 63;
  if (t < VSX_FQS_SYMS) { s_qual[t] = 0; s_tail[t] = 0; }
  if (t < 26) { s_other[t] = 0; s_maxrun[t] = 0; }
  if (t == 0) { s_maxlen = 0; s_nmin = 255; s_nmax = 0; }
  __syncthreads();

  const uint32_t read = blockIdx.x * VSX_FQS_THREADS + t;
  VsxEestatsItem it { 0, 0 };
  if (read < n_items) it = items[read];
  const int full = (int) it.len;
  atomicMax(&s_maxlen, full);
  __syncthreads();
  const int maxlen = __builtin_amdgcn_readfirstlane(s_maxlen);

  uint8_t * const seq_tile = reinterpret_cast<uint8_t *>(s_seq_tile);
  uint8_t * const qual_tile = reinterpret_cast<uint8_t *>(s_qual_tile);
  const size_t wave_at = (size_t) (t - lane) * ROW_BYTES, my_at = (size_t) t * ROW_BYTES;

  uint32_t n_a = 0, n_c = 0, n_g = 0, n_t = 0, n_n = 0;
  int run_char = -1, run = 0;              // the reference's counter: the run's length minus one
  int tail_char = -1;                      // the run of equal quality characters that ends at the current position
  uint32_t tail_run = 0;
  uint32_t nmin = 255, nmax = 0, bad = 0;

  for (int c = 0; c < maxlen; c += VSX_FQS_TILE)
    {
      const int jn = maxlen - c < VSX_FQS_TILE ? maxlen - c : VSX_FQS_TILE;
      load_rows(seq_tile + wave_at, seq, it.off, full, c, lane);
      load_rows(qual_tile + wave_at, qual, it.off, full, c, lane);
      __syncthreads();

      const int mine = full - c < jn ? full - c : jn;
      for (int j = 0; j < mine; ++j)
        {
          const int raw = (int) seq_tile[my_at + j], q = (int) qual_tile[my_at + j];
          const int s = (unsigned) ((raw | 0x20) - 'a') < 26u ? (raw & 0xDF) : 'N';
          if (s == 'A') ++n_a;
          else if (s == 'C') ++n_c;
          else if (s == 'G') ++n_g;
          else if (s == 'T') ++n_t;
          else if (s == 'N') ++n_n;
          else atomicAdd(&s_other[s - 'A'], 1u);
          const int column = q - VSX_FQS_FIRST;
          if ((unsigned) column < (unsigned) VSX_FQS_SYMS) atomicAdd(&s_qual[column], 1u);
          else bad = 1;
          if (s == 'N')
            {
              nmin = (uint32_t) q < nmin ? (uint32_t) q : nmin;
              nmax = (uint32_t) q > nmax ? (uint32_t) q : nmax;
            }
          if (s == run_char) ++run;
          else
            {
              if (run > 0) atomicMax(&s_maxrun[run_char - 'A'], run);
              run_char = s;
              run = 0;
            }
          if (q == tail_char) ++tail_run;
          else { tail_char = q; tail_run = 1; }
        }
      __syncthreads();
      // per tile: a workgroup adds at most 256 x 64 to a counter between two flushes
      if (t < VSX_FQS_SYMS && s_qual[t]) { atomicAdd(&acc->qual[VSX_FQS_FIRST + t], (unsigned long long) s_qual[t]); s_qual[t] = 0; }
      if (t >= 128 && t < 128 + 26 && s_other[t - 128]) { atomicAdd(&acc->seq['A' + t - 128], (unsigned long long) s_other[t - 128]); s_other[t - 128] = 0; }
      __syncthreads();
    }

  if (run > 0) atomicMax(&s_maxrun[run_char - 'A'], run);
  if ((uint32_t) full >= tail && tail_run >= tail && (unsigned) (tail_char - VSX_FQS_FIRST) < (unsigned) VSX_FQS_SYMS)
    atomicAdd(&s_tail[tail_char - VSX_FQS_FIRST], 1u);
  typedef unsigned long long u64;                                 // (the sums are taken in 64 bits)
  const u64 w_a = wave_sum<u64>(n_a), w_c = wave_sum<u64>(n_c), w_g = wave_sum<u64>(n_g), w_t = wave_sum<u64>(n_t), w_n = wave_sum<u64>(n_n);
  if (lane == 0)
    {
      if (w_a) atomicAdd(&acc->seq['A'], w_a);
      if (w_c) atomicAdd(&acc->seq['C'], w_c);
      if (w_g) atomicAdd(&acc->seq['G'], w_g);
      if (w_t) atomicAdd(&acc->seq['T'], w_t);
      if (w_n) atomicAdd(&acc->seq['N'], w_n);
    }
  if (nmin <= nmax) { atomicMin(&s_nmin, nmin); atomicMax(&s_nmax, nmax); }
  __syncthreads();
  if (t < VSX_FQS_SYMS && s_tail[t]) atomicAdd(&acc->tail[VSX_FQS_FIRST + t], (unsigned long long) s_tail[t]);
  if (t >= 128 && t < 128 + 26 && s_maxrun[t - 128] > 0) atomicMax(&acc->maxrun['A' + t - 128], s_maxrun[t - 128]);
  if (t == 0 && s_nmin <= s_nmax) { atomicMin(&acc->qmin_n, s_nmin); atomicMax(&acc->qmax_n, s_nmax); }
  if (read < n_items) err[read] = bad;
}

}  // namespace

extern "C" hipError_t vsx_launch_fastq_stats_walk(const VsxEestatsItem * d_items, uint32_t n_items, const uint8_t * d_qual,
                                                  VsxFastqStatsParams P, uint32_t * d_minmax, hipStream_t st)
{
  if (n_items == 0) return hipSuccess;
  const uint32_t blocks = (n_items + VSX_FQS_THREADS - 1) / VSX_FQS_THREADS;
  hipLaunchKernelGGL(vsx_fastq_stats_walk_kernel, dim3(blocks), dim3(VSX_FQS_THREADS), 0, st, d_items, n_items, d_qual, P, d_minmax);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_fastq_chars(const VsxEestatsItem * d_items, uint32_t n_items, const uint8_t * d_seq, const uint8_t * d_qual,
                                             uint32_t tail, VsxFastqCharsAcc * d_acc, uint32_t * d_err, hipStream_t st)
{
  if (n_items == 0) return hipSuccess;
  const uint32_t blocks = (n_items + VSX_FQS_THREADS - 1) / VSX_FQS_THREADS;
  hipLaunchKernelGGL(vsx_fastq_chars_kernel, dim3(blocks), dim3(VSX_FQS_THREADS), 0, st, d_items, n_items, d_seq, d_qual, tail, d_acc, d_err);
  return hipGetLastError();
}
