// vsx_filter.hip -- read quality filtering on gfx950: one wavefront per read, the quality walk in chunks of 64 positions.
//
// The reference (core/filter.cpp: analyse) strips and truncates a read by position, then walks its quality symbols: at each
// position it checks the range, adds the tabulated error 10^(-q/10) to a running double, and stops when the quality is at or
// below truncqual or the sum passes truncee / truncee_rate * positions; at a stop it subtracts the last error again.  The sum is
// order-dependent, so it is formed in position order on a value every lane holds identically: per chunk each lane loads one
// quality byte (one coalesced 64-byte load) and looks its error up in an LDS copy of the host-built table, the three
// per-position conditions (out of range, <= truncqual, < minqual) become 64-bit ballots, and the chunk's additions run over
// v_readlane broadcasts of lane j's error.  With truncee and truncee_rate unbounded (the default) the stop position follows
// from the ballots alone and the loop is additions only.  The add and the subtract at a stop stay two operations (the stored
// sum is (ee + e) - e, not the previous ee); the file is built with -ffp-contract=off and without fast-math, so ee / length is
// the IEEE double division.  No array is sized by the read length: any length the interface admits runs here.
// Output: one record per read, an ordinary vector store by lane 0.
#include <hip/hip_runtime.h>
#include <float.h>
#include "vsx_filter_internal.h"

namespace {

// lane j's value on every lane; j is wave-uniform
__device__ inline double lane_value(double v, int j)
{
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), j), hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
  return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(VSX_FILTER_THREADS)
void vsx_filter_kernel(const VsxFilterItem * __restrict__ items, uint32_t n_items, const uint8_t * __restrict__ seq,
                       const uint8_t * __restrict__ qual, VsxFilterParams P, VsxFilterDevRec * __restrict__ recs)
{
  __shared__ double s_q2e[128];
  for (int k = threadIdx.x; k < 128; k += VSX_FILTER_THREADS) s_q2e[k] = P.q2e[k];
  __syncthreads();

  // (threadIdx.x / 64 is not provably wave-uniform; everything below that steers a loop is)
  const uint32_t read = __builtin_amdgcn_readfirstlane(blockIdx.x * VSX_FILTER_WAVES + (threadIdx.x >> 6));
  if (read >= n_items) return;
  const int lane = threadIdx.x & 63;
  const VsxFilterItem it = items[read];
  const int full = (int) it.len;

  // ---- strip and truncate by position
  int start = 0, len = full;
  if (P.stripleft < (int64_t) len) { start += (int) P.stripleft; len -= (int) P.stripleft; } else { start = len; len = 0; }
  if (P.stripright < (int64_t) len) len -= (int) P.stripright; else len = 0;
  if (P.trunclen >= 0 && P.trunclen < (int64_t) len) len = (int) P.trunclen;
  if (P.trunclen_keep >= 0 && P.trunclen_keep < (int64_t) len) len = (int) P.trunclen_keep;

  VsxFilterDevRec rec;
  rec.qerr = 0; rec.pad = 0; rec.qerr_value = 0;
  bool discarded = false;
  double ee = -1.0;

  if (P.has_qual)
    {
      // ---- the quality walk
      ee = 0.0;
      const uint8_t * q = qual + it.off + start;
      const bool bounded = P.truncee < DBL_MAX || P.truncee_rate < DBL_MAX;
      const int walk = len;
      bool stopped = false;
      for (int c = 0; c < walk && !stopped; c += 64)
        {
          const int n = walk - c < 64 ? walk - c : 64;
          const bool valid = lane < n;
          const int sym = valid ? (int) q[c + lane] : 0;
          const int v = (int) (int8_t) sym - P.ascii;
          const bool oor = valid && (v < P.qmin || v > P.qmax);
          const double e = valid ? s_q2e[sym & 127] : 0.0;
          const unsigned long long b_oor = __ballot(oor), b_tq = __ballot(valid && (int64_t) v <= P.truncqual),
                                   b_mq = __ballot(valid && (int64_t) v < P.minqual);
          // positions before `first` are in range and above truncqual
          const unsigned long long b_first = b_oor | b_tq;
          const int first = b_first ? __ffsll(b_first) - 1 : n;
          int j = 0;
          if (bounded)
            for (; j < first; ++j)
              {
                const double ej = lane_value(e, j);
                ee += ej;
                if (ee > P.truncee || ee > P.truncee_rate * (double) (c + j + 1)) { ee -= ej; stopped = true; break; }
              }
          else
            for (; j < first; ++j) ee += lane_value(e, j);
          if (!stopped && first < n)
            {
              if ((b_oor >> first) & 1)
                {
                  // the range check comes before the stop test of the same position
                  const int bad = __builtin_amdgcn_readlane(v, first);
                  rec.start = start; rec.length = c + first; rec.ee = ee; rec.discarded = 0; rec.truncated = 0;
                  rec.qerr = bad < P.qmin ? 1 : 2; rec.qerr_value = bad;
                  if (lane == 0) recs[read] = rec;
                  return;
                }
              const double ej = lane_value(e, first);
              ee += ej;
              ee -= ej;
              stopped = true;
            }
          // j: the stop position of this chunk, or the positions it passed; a quality below minqual counts before the stop only
          const unsigned long long before = j >= 64 ? ~0ull : (1ull << j) - 1;
          if (b_mq & before) discarded = true;
          if (stopped) len = c + j;
        }

      // ---- expected-error filters
      if (ee > P.maxee) discarded = true;
      if (len > 0 && ee / (double) len > P.maxee_rate) discarded = true;
    }

  // ---- length and content filters (the abundance filter needs no device: the host applies it)
  if (P.trunclen >= 0 && (int64_t) len < P.trunclen) discarded = true;
  if ((int64_t) len < P.minlen || (int64_t) len > P.maxlen) discarded = true;
  const uint8_t * s = seq + it.off + start;
  int64_t ncount = 0;
  for (int c = 0; c < len; c += 64)
    {
      const uint8_t ch = c + lane < len ? s[c + lane] : 0;
      ncount += __popcll(__ballot(ch == 'N' || ch == 'n'));
    }
  if (ncount > P.maxns) discarded = true;

  rec.start = start; rec.length = len; rec.ee = ee;
  rec.discarded = discarded ? 1 : 0; rec.truncated = len < full ? 1 : 0;
  if (lane == 0) recs[read] = rec;
}

}  // namespace

extern "C" hipError_t vsx_launch_filter(const VsxFilterItem * d_items, uint32_t n_items, const uint8_t * d_seq, const uint8_t * d_qual,
                                        VsxFilterParams P, VsxFilterDevRec * d_recs, hipStream_t st)
{
  if (n_items == 0) return hipSuccess;
  const uint32_t blocks = (n_items + VSX_FILTER_WAVES - 1) / VSX_FILTER_WAVES;
  hipLaunchKernelGGL(vsx_filter_kernel, dim3(blocks), dim3(VSX_FILTER_THREADS), 0, st, d_items, n_items, d_seq, d_qual, P, d_recs);
  return hipGetLastError();
}
