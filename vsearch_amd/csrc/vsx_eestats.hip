// vsx_eestats.hip -- read quality statistics on gfx950: the tables of --fastq_eestats and --fastq_eestats2 in three kernels.
//
// The reference (commands/fastq_eestats.cpp, fastq_eestats2.cpp) walks every quality symbol of every read, adds the tabulated
// error 10^(-q/10) to a running double `ee` and, at every position, counts the quality, counts the bin (int)(1000.0 * ee) of a
// per-position histogram and adds ee to a per-position double; eestats2 compares ee with a list of cutoffs at a list of lengths.
//
//   walk      one lane per read, 256 reads per workgroup, 64 positions at a time: each wave brings its reads' quality bytes into
//             LDS with one coalesced 64-byte load per read, then every lane walks its own row, its ee carried from tile to tile.
//             All lanes of a wave are at the same position, so the cutoff positions of eestats2 are wave-uniform and a count is
//             one ballot.  Quality counts go to a workgroup-private LDS histogram flushed once per tile; histogram bins go to the
//             global histogram by integer atomics (equal bins combined inside the wave at early positions, where a position sees
//             a handful of distinct bins); the running ee goes into matrix[position][read], a coalesced store.
//   sum       sum_ee[i] is a chain of dependent double adds over the reads in input order: one lane per position, 16 positions
//             per workgroup.  All four waves fetch the next 16 x 256 block of the matrix (rows are contiguous in the reads) into
//             registers while 16 lanes of the first wave add the block already in LDS column by column -- the transpose between
//             "lane = read" and "lane = position" happens in LDS.  A read shorter than the position adds +0.0, which is exact
//             for these non-negative sums.  The chain is carried from window to window through d_sum; windows follow each other
//             by stream order and events only: no workgroup ever waits for another.
//   quantile  one wave per position scans that position's histogram row with a running integer prefix count and emits the five
//             bins the reference's scan finds (first / last non-zero bin, first bin with count >= 0.25, 0.50, 0.75 * reads).
//
// No floating-point atomics, no flags, tickets or cooperative launches; stores are ordinary vector stores.  The file is built
// with -ffp-contract=off and without fast-math: ee += pe and 1000.0 * ee are the IEEE double operations of the reference.
#include <hip/hip_runtime.h>
#include "vsx_eestats_internal.h"

namespace {

// where row i of the histogram starts (the reference's ee_start)
__device__ inline size_t ee_start(size_t i) { return i * (VSX_EESTATS_RESOLUTION * (i + 1) + 2) / 2; }

__global__ __launch_bounds__(VSX_EESTATS_THREADS)
void vsx_eestats_walk_kernel(const VsxEestatsItem * __restrict__ items, uint32_t n_items, const uint8_t * __restrict__ qual,
                             VsxEestatsParams P, uint32_t * __restrict__ err)
{
  __shared__ double s_q2e[128];
  __shared__ uint32_t s_tile[VSX_EESTATS_THREADS * VSX_EESTATS_ROW_WORDS];
  __shared__ uint32_t s_qc[VSX_EESTATS_TILE * VSX_EESTATS_MAX_COLS];
  __shared__ int s_maxlen;

  const int t = threadIdx.x, lane = t & 63;
  if (t < 128) s_q2e[t] = P.q2e[t];
  if (t == 0) s_maxlen = 0;
  __syncthreads();

  const uint32_t read = blockIdx.x * VSX_EESTATS_THREADS + t;
  VsxEestatsItem it { 0, 0 };
  if (read < n_items) it = items[read];
  const int full = (int) it.len;
  atomicMax(&s_maxlen, full);
  __syncthreads();
  const int maxlen = __builtin_amdgcn_readfirstlane(s_maxlen);

  uint8_t * const tile = reinterpret_cast<uint8_t *>(s_tile);
  uint8_t * const wave_rows = tile + (size_t) (t - lane) * (VSX_EESTATS_ROW_WORDS * 4);
  const uint8_t * const my_row = tile + (size_t) t * (VSX_EESTATS_ROW_WORDS * 4);
  const int cols = P.cols;

  int len = full;                          // shortened to the first out-of-range position, if there is one
  uint32_t bad = VSX_EESTATS_NO_ERROR;
  double ee = 0.0;
  // the next cutoff position of eestats2 (0-based) and its row; wave-uniform
  long long next_cut = (long long) P.shortest - 1;
  int cut_row = 0;

  for (int c = 0; c < maxlen; c += VSX_EESTATS_TILE)
    {
      const int jn = maxlen - c < VSX_EESTATS_TILE ? maxlen - c : VSX_EESTATS_TILE;
      if (P.want_tables)
        for (int k = t; k < jn * cols; k += VSX_EESTATS_THREADS) s_qc[k] = 0;
      // each wave loads the rows of its own 64 reads: row r is the read of lane r
      for (int r = 0; r < 64; ++r)
        {
          const uint32_t roff = (uint32_t) __builtin_amdgcn_readlane((int) it.off, r);
          const int rlen = __builtin_amdgcn_readlane(full, r);
          if (c >= rlen) continue;
          const int sym = c + lane < rlen ? (int) qual[(size_t) roff + c + lane] : 0;
          wave_rows[r * (VSX_EESTATS_ROW_WORDS * 4) + lane] = (uint8_t) sym;
        }
      __syncthreads();

      const bool combine = c < VSX_EESTATS_COMBINE_BELOW;
      for (int j = 0; j < jn; ++j)
        {
          const int i = c + j;
          bool active = i < len;
          const int sym = active ? (int) my_row[j] : 0;
          const int v = (int) (int8_t) sym - P.ascii;
          if (active && (v < P.qmin || v > P.qmax)) { bad = (uint32_t) i; len = i; active = false; }
          const int q = v > 0 ? v : 0;
          if (active) ee += s_q2e[sym & 127];

          if (P.want_tables)
            {
              const int limit = VSX_EESTATS_RESOLUTION * (i + 1);
              const int e_int = (int) ((double) VSX_EESTATS_RESOLUTION * ee);
              const int bin = e_int < limit ? e_int : limit;
              uint32_t * const row = P.hist + ee_start((size_t) i);
              if (active)
                {
                  atomicAdd(&s_qc[j * cols + q], 1u);
                  P.matrix[(size_t) i * P.stride + read] = ee;
                }
              if (combine)
                {
                  unsigned long long todo = __ballot(active);
                  while (todo)
                    {
                      const int leader = __ffsll(todo) - 1;
                      const int b = __builtin_amdgcn_readlane(bin, leader);
                      const unsigned long long same = __ballot(active && bin == b);
                      if (lane == leader) atomicAdd(&row[b], (uint32_t) __popcll(same));
                      todo &= ~same;
                    }
                }
              else if (active) atomicAdd(&row[bin], 1u);
            }

          if (P.want_cutoffs && i == next_cut && cut_row < P.len_steps)
            {
              for (int y = 0; y < P.n_cutoffs; ++y)
                {
                  const double cutoff = P.cutoffs[y];
                  const uint32_t count = (uint32_t) __popcll(__ballot(active && ee <= cutoff));
                  if (lane == 0 && count) atomicAdd(&P.cutoff_counts[(size_t) cut_row * P.n_cutoffs + y], count);
                }
              next_cut += P.increment;
              ++cut_row;
            }
        }
      __syncthreads();
      if (P.want_tables)
        {
          // (c + j) * cols + q == c * cols + k
          uint32_t * const dst = P.qual_counts + (size_t) c * cols;
          for (int k = t; k < jn * cols; k += VSX_EESTATS_THREADS)
            if (s_qc[k]) atomicAdd(&dst[k], s_qc[k]);
          __syncthreads();
        }
    }
  if (read < n_items) err[read] = bad;
}

// read r's column of the 16 matrix rows from p0 on, and its length
__device__ __forceinline__ void sum_fetch(const double * __restrict__ matrix, uint32_t stride, const VsxEestatsItem * __restrict__ items,
                                          uint32_t n_items, uint32_t len_max, uint32_t p0, uint32_t r,
                                          double (&reg)[VSX_EESTATS_SUM_POS], uint32_t & reg_len)
{
  const bool have = r < n_items;
  reg_len = have ? items[r].len : 0u;
#pragma unroll
  for (int k = 0; k < VSX_EESTATS_SUM_POS; ++k)
    reg[k] = have && p0 + k < len_max ? matrix[(size_t) (p0 + k) * stride + r] : 0.0;
}

__global__ __launch_bounds__(VSX_EESTATS_SUM_READS)
void vsx_eestats_sum_kernel(const double * __restrict__ matrix, uint32_t stride, const VsxEestatsItem * __restrict__ items,
                            uint32_t n_items, uint32_t len_max, double * __restrict__ sum)
{
  constexpr int ROW = VSX_EESTATS_SUM_READS + 1;          // doubles; lane p reads s_m[p * ROW + r]: 16 different bank pairs
  __shared__ double s_m[VSX_EESTATS_SUM_POS * ROW];
  __shared__ uint32_t s_len[VSX_EESTATS_SUM_READS];

  const int t = threadIdx.x;
  const uint32_t p0 = blockIdx.x * VSX_EESTATS_SUM_POS;
  const uint32_t p = p0 + t;
  const bool adder = t < VSX_EESTATS_SUM_POS && p < len_max;
  double acc = adder ? sum[p] : 0.0;

  double reg[VSX_EESTATS_SUM_POS];
  uint32_t reg_len;
  sum_fetch(matrix, stride, items, n_items, len_max, p0, (uint32_t) t, reg, reg_len);
  for (uint32_t r0 = 0; r0 < n_items; r0 += VSX_EESTATS_SUM_READS)
    {
#pragma unroll
      for (int k = 0; k < VSX_EESTATS_SUM_POS; ++k) s_m[k * ROW + t] = reg[k];
      s_len[t] = reg_len;
      __syncthreads();
      // in flight while the chain below runs
      if (r0 + VSX_EESTATS_SUM_READS < n_items)
        sum_fetch(matrix, stride, items, n_items, len_max, p0, r0 + VSX_EESTATS_SUM_READS + t, reg, reg_len);
      if (adder)
        {
          const int count = n_items - r0 < VSX_EESTATS_SUM_READS ? (int) (n_items - r0) : VSX_EESTATS_SUM_READS;
          const double * const mine = s_m + t * ROW;
#pragma unroll 8
          for (int r = 0; r < count; ++r)
            {
              // what lies in the matrix beyond a read's end was never written: select, do not multiply
              const double v = p < s_len[r] ? mine[r] : 0.0;
              acc += v;
            }
        }
      __syncthreads();
    }
  if (adder) sum[p] = acc;
}

__global__ __launch_bounds__(64)
void vsx_eestats_quantile_kernel(const uint32_t * __restrict__ hist, const uint64_t * __restrict__ reads_at, uint32_t len_max,
                                 int64_t * __restrict__ bins)
{
  const uint32_t i = blockIdx.x;
  if (i >= len_max) return;
  const int lane = threadIdx.x;
  const uint32_t * const row = hist + ee_start((size_t) i);
  const int nbins = VSX_EESTATS_RESOLUTION * ((int) i + 1) + 1;
  // the reference compares a running count held in a double with 0.25 * reads: both are exact below 2^53
  const double reads = (double) reads_at[i];
  const double t_low = 0.25 * reads, t_med = 0.50 * reads, t_hi = 0.75 * reads;
  long long b_min = -1, b_low = -1, b_med = -1, b_hi = -1, b_max = -1;
  unsigned long long carry = 0;
  for (int k0 = 0; k0 < nbins; k0 += 64)
    {
      const int k = k0 + lane;
      const uint32_t x = k < nbins ? row[k] : 0u;
      const unsigned long long nonzero = __ballot(x != 0);
      if (!nonzero) continue;
      unsigned long long n = x;
      for (int d = 1; d < 64; d <<= 1)
        {
          const unsigned long long up = __shfl_up(n, d);
          if (lane >= d) n += up;
        }
      n += carry;
      // the count only grows at non-zero bins, so the first lane at or above a threshold holds a non-zero bin
      if (b_min < 0) b_min = k0 + __ffsll(nonzero) - 1;
      b_max = k0 + 63 - __clzll(nonzero);
      unsigned long long at;
      if (b_low < 0 && (at = __ballot((double) n >= t_low))) b_low = k0 + __ffsll(at) - 1;
      if (b_med < 0 && (at = __ballot((double) n >= t_med))) b_med = k0 + __ffsll(at) - 1;
      if (b_hi < 0 && (at = __ballot((double) n >= t_hi))) b_hi = k0 + __ffsll(at) - 1;
      carry = __shfl(n, 63);
    }
  if (lane == 0)
    {
      int64_t * const o = bins + (size_t) i * 5;
      o[0] = b_min; o[1] = b_low; o[2] = b_med; o[3] = b_hi; o[4] = b_max;
    }
}

}  // namespace

extern "C" hipError_t vsx_launch_eestats_walk(const VsxEestatsItem * d_items, uint32_t n_items, const uint8_t * d_qual, VsxEestatsParams P,
                                              uint32_t * d_err, hipStream_t st)
{
  if (n_items == 0) return hipSuccess;
  const uint32_t blocks = (n_items + VSX_EESTATS_THREADS - 1) / VSX_EESTATS_THREADS;
  hipLaunchKernelGGL(vsx_eestats_walk_kernel, dim3(blocks), dim3(VSX_EESTATS_THREADS), 0, st, d_items, n_items, d_qual, P, d_err);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_eestats_sum(const double * d_matrix, uint32_t stride, const VsxEestatsItem * d_items, uint32_t n_items,
                                             uint32_t len_max, double * d_sum, hipStream_t st)
{
  if (n_items == 0 || len_max == 0) return hipSuccess;
  const uint32_t blocks = (len_max + VSX_EESTATS_SUM_POS - 1) / VSX_EESTATS_SUM_POS;
  hipLaunchKernelGGL(vsx_eestats_sum_kernel, dim3(blocks), dim3(VSX_EESTATS_SUM_READS), 0, st, d_matrix, stride, d_items, n_items, len_max, d_sum);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_eestats_quantile(const uint32_t * d_hist, const uint64_t * d_reads_at, uint32_t len_max, int64_t * d_bins,
                                                  hipStream_t st)
{
  if (len_max == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_eestats_quantile_kernel, dim3(len_max), dim3(64), 0, st, d_hist, d_reads_at, len_max, d_bins);
  return hipGetLastError();
}
