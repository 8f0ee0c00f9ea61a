// vsx_chimera.hip -- parent selection and scoring of --uchime_ref on the device: find_best_parents + eval_parents
// (reference core/chimera.cpp:627-751, :1245-1700), one workgroup per query.  The host form of the same two functions is
// chimera_eval_host in vsx_chimera.cpp (long queries, sentinel pairs, VSX_CHIMERA=host, and the tests' checker).
//
// Inputs: the whole-query alignments of a query against its <= 16 candidate parents as the traceback left them in HBM (hit records
// + run words, the format of vsx_plan_export_hits / vsx_plan_export_runs) and the 4-bit codes of the query and the candidates.
//
//   find_matches (:367-413)      candidate c's match row = one bit per query position (a NONZERO 4-bit AND of the aligned symbols),
//                                16 rows of VSX_CHIMERA_MAX_QLEN bits in LDS; one wave walks one candidate's runs, lanes over a run
//   smooth / maxsmooth / wins     the 32-column window sum at qpos is popcount of the 32 bits ending there (two LDS words); one
//                                thread per position takes the max over the live candidates and counts the winners
//   wipe (:651-664)              position i is cleared for every candidate iff the first parent won a window ending in [i, i + 31]:
//                                a bit vector of winning window ends, OR-ed over 32 shifts per word
//   eval_parents                 only QUERY columns can survive `ignore` (an insertion column has qsym 0), so the three-row
//                                alignment is never built: per query position the two parents' codes (0 = 'D'), plus one bit
//                                "some parent inserts before this position" (maxi > 0) for the gap-neighbour rule.  left / right
//                                counts = a block-wide prefix scan of the A / B / abstain columns packed into one 64-bit word
//                                (21 bits each), h per column in both orientations, arg-max = largest h, then lowest column
//                                (= the reference's ascending visit with strict '>').
//
// Exact arithmetic: h, QA .. QM and the divergence are the reference's double expressions, separately rounded (no contraction,
// plain IEEE division), so the kernel's records equal the host restatement's and the x86 reference's bit for bit.
//
// LDS: 12.5 KiB shared by the two phases (selection: 16 x 4096 match bits + round-0 maxsmooth bytes + wipe bits; scoring: two
// parent code rows + one flag byte per position + insertion bits) and 5 KiB of per-thread arg-max slots: ~18 KiB per 256-thread
// workgroup, 8 workgroups (32 waves) per CU -- occupancy is not what limits this kernel, the serial run walks are.
#include "vsx_internal.h"
#include "../../include/vsx_search.h"

#include <hip/hip_runtime.h>
#include "vsx_devutil.h"
#include "vsx_symbols.h"

#pragma clang fp contract(off)

namespace {

constexpr int CH_THREADS = 256;
constexpr int CH_WAVES = CH_THREADS / 64;
constexpr int CH_LMAX = VSX_CHIMERA_MAX_QLEN;
constexpr int CH_W = CH_LMAX / 32;                  // match-bit words per candidate row
constexpr int CH_WIN = 32;                          // `window` (chimera.cpp:110)
constexpr unsigned long long M21 = (1ull << 21) - 1;

constexpr int P1_MBITS = VSX_CHIM_MAXCAND * CH_W * 4;
constexpr int P1_MS0 = CH_LMAX;
constexpr int P1_BYTES = P1_MBITS + P1_MS0 + (CH_W + 1) * 4;
constexpr int P2_BYTES = 3 * CH_LMAX + (CH_W + 1) * 4;
constexpr int LDS_BYTES = P1_BYTES > P2_BYTES ? P1_BYTES : P2_BYTES;
static_assert(CH_LMAX % 32 == 0 && CH_LMAX < (1 << 21), "layout");

using vsxsym::ambiguous4;

// the 32-column window sum ending at qpos (qpos >= 31)
__device__ __forceinline__ int smooth_at(const uint32_t * row, int qpos)
{
  const int s = qpos - (CH_WIN - 1);
  const int w = s >> 5, o = s & 31;
  uint32_t v = row[w];
  if (o) v = (v >> o) | (row[w + 1] << (32 - o));
  return __popc(v);
}

__device__ void write_unscored(vsx_chimera_result * r, int status, uint32_t pa, uint32_t pb)
{
  vsx_chimera_result z = {};
  z.parent_a = pa;
  z.parent_b = pb;
  z.closest = 0xFFFFFFFFu;
  z.status = status;
  z.flag = 'N';
  *r = z;
}

__global__ void __launch_bounds__(CH_THREADS)
vsx_chimera_eval_kernel(const VsxChimItem * __restrict__ items, const uint8_t * __restrict__ qcodes, const uint64_t * __restrict__ qoff,
                        const uint32_t * __restrict__ qlen, const uint8_t * __restrict__ tcodes, const uint64_t * __restrict__ toff,
                        const uint32_t * __restrict__ tlen, const VsxPairOut * __restrict__ hits, const uint32_t * __restrict__ runs,
                        uint64_t n_runs, VsxChimParams P, vsx_chimera_result * __restrict__ out)
{
  __shared__ __align__(16) uint8_t lds[LDS_BYTES];
  __shared__ int s_wins[VSX_CHIM_MAXCAND];
  __shared__ int s_cnt[5];
  __shared__ int s_best;
  __shared__ unsigned long long s_tot, s_wsum[CH_WAVES];
  __shared__ double s_h[CH_THREADS];
  __shared__ int s_i[CH_THREADS];
  __shared__ unsigned long long s_pk[CH_THREADS];

  const VsxChimItem & it = items[blockIdx.x];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int L = (int) qlen[it.q];
  const int nc = (int) (it.ncand < VSX_CHIM_MAXCAND ? it.ncand : VSX_CHIM_MAXCAND);
  const uint8_t * q = qcodes + qoff[it.q];
  vsx_chimera_result * res = out + it.out;
  if (L > CH_LMAX || L < CH_WIN || nc < 2)         // (the host sends no such item; < 32 columns or < 2 candidates: no parents)
    {
      if (tid == 0) write_unscored(res, VSX_CHIMERA_NO_PARENTS, 0xFFFFFFFFu, 0xFFFFFFFFu);
      return;
    }

  // ---- find_matches ----
  uint32_t * mb = reinterpret_cast<uint32_t *>(lds);
  uint8_t * ms0 = lds + P1_MBITS;
  uint32_t * flg = reinterpret_cast<uint32_t *>(lds + P1_MBITS + P1_MS0);
  const int W = (L + 31) >> 5;
  for (int k = tid; k < VSX_CHIM_MAXCAND * CH_W; k += CH_THREADS) mb[k] = 0u;
  for (int k = tid; k <= CH_W; k += CH_THREADS) flg[k] = 0u;
  if (tid < VSX_CHIM_MAXCAND) s_wins[tid] = 0;
  __syncthreads();
  for (int c = wave; c < nc; c += CH_WAVES)
    {
      const VsxPairOut h = hits[it.pair0 + c];
      const uint8_t * t = tcodes + toff[it.cand[c]];
      const int tl = (int) tlen[it.cand[c]];
      int qp = 0, tp = 0;
      for (int k = (int) h.nruns - 1; k >= 0; --k)          // run words are stored last column first
        {
          const uint64_t ri = h.run_off + (uint64_t) k;
          if (ri >= n_runs) break;
          const uint32_t word = runs[ri];
          const int len = (int) (word >> 2), op = (int) (word & 3u);
          if (op == 0)
            {
              for (int j = lane; j < len; j += 64)
                {
                  const int a = qp + j, b = tp + j;
                  if (a < L && b < tl && (q[a] & t[b]) != 0) atomicOr(&mb[c * CH_W + (a >> 5)], 1u << (a & 31));
                }
              qp += len;
              tp += len;
            }
          else if (op == 1) tp += len;
          else qp += len;
        }
    }
  __syncthreads();

  // ---- find_best_parents: two rounds ----
  int parent[2] = {-1, -1};
  for (int f = 0; f < 2; ++f)
    {
      if (f == 1)
        {
          const uint32_t * row0 = mb + parent[0] * CH_W;
          for (int qp = CH_WIN - 1 + tid; qp < L; qp += CH_THREADS)
            if (smooth_at(row0, qp) == (int) ms0[qp]) atomicOr(&flg[qp >> 5], 1u << (qp & 31));
          __syncthreads();
          for (int w = tid; w < W; w += CH_THREADS)
            {
              const unsigned long long F = (unsigned long long) flg[w] | ((unsigned long long) flg[w + 1] << 32);
              uint32_t wipe = 0u;
#pragma unroll
              for (int k = 0; k < CH_WIN; ++k) wipe |= (uint32_t) (F >> k);
              if (wipe)
                for (int c = 0; c < nc; ++c) mb[c * CH_W + w] &= ~wipe;
            }
          if (tid < VSX_CHIM_MAXCAND) s_wins[tid] = 0;
          __syncthreads();
        }
      int wl[VSX_CHIM_MAXCAND];
#pragma unroll
      for (int c = 0; c < VSX_CHIM_MAXCAND; ++c) wl[c] = 0;
      for (int qp = CH_WIN - 1 + tid; qp < L; qp += CH_THREADS)
        {
          int sm[VSX_CHIM_MAXCAND];
          int mx = 0;
#pragma unroll
          for (int c = 0; c < VSX_CHIM_MAXCAND; ++c)
            {
              sm[c] = (c < nc && c != parent[0]) ? smooth_at(mb + c * CH_W, qp) : -1;
              mx = sm[c] > mx ? sm[c] : mx;
            }
          if (f == 0) ms0[qp] = (uint8_t) mx;
          if (mx != 0)
            {
#pragma unroll
              for (int c = 0; c < VSX_CHIM_MAXCAND; ++c) wl[c] += sm[c] == mx ? 1 : 0;
            }
        }
#pragma unroll
      for (int c = 0; c < VSX_CHIM_MAXCAND; ++c)
        if (wl[c]) atomicAdd(&s_wins[c], wl[c]);
      __syncthreads();
      int best = -1, maxwins = 0;
      for (int c = 0; c < nc; ++c)
        if (s_wins[c] > maxwins) { maxwins = s_wins[c]; best = c; }
      parent[f] = best;
      __syncthreads();
      if (best < 0) break;
    }
  if (parent[0] < 0 || parent[1] < 0)
    {
      if (tid == 0) write_unscored(res, VSX_CHIMERA_NO_PARENTS, 0xFFFFFFFFu, 0xFFFFFFFFu);
      return;
    }

  // ---- eval_parents: the two parents' codes per query position ----
  uint8_t * ac = lds;
  uint8_t * bc = lds + CH_LMAX;
  uint8_t * cat = lds + 2 * CH_LMAX;
  uint32_t * ins = reinterpret_cast<uint32_t *>(lds + 3 * CH_LMAX);
  for (int k = tid; k < L; k += CH_THREADS) { ac[k] = 0; bc[k] = 0; }
  for (int k = tid; k <= CH_W; k += CH_THREADS) ins[k] = 0u;
  if (tid == 0) s_tot = 0ull;
  if (tid < 5) s_cnt[tid] = 0;
  __syncthreads();
  if (wave < 2)
    {
      const int c = parent[wave];
      uint8_t * dst = wave == 0 ? ac : bc;
      const VsxPairOut h = hits[it.pair0 + c];
      const uint8_t * t = tcodes + toff[it.cand[c]];
      const int tl = (int) tlen[it.cand[c]];
      int qp = 0, tp = 0;
      for (int k = (int) h.nruns - 1; k >= 0; --k)
        {
          const uint64_t ri = h.run_off + (uint64_t) k;
          if (ri >= n_runs) break;
          const uint32_t word = runs[ri];
          const int len = (int) (word >> 2), op = (int) (word & 3u);
          if (op == 0)
            {
              for (int j = lane; j < len; j += 64)
                {
                  const int a = qp + j, b = tp + j;
                  if (a < L && b < tl) dst[a] = t[b];
                }
              qp += len;
              tp += len;
            }
          else if (op == 1)
            {
              if (lane == 0 && qp <= L) atomicOr(&ins[qp >> 5], 1u << (qp & 31));      // maxi[qp] > 0
              tp += len;
            }
          else qp += len;                                                             // 'D': the parent has a gap (code 0)
        }
    }
  __syncthreads();

  // ignore + diffs per position: bits 0-1 class (0 none, 1 A, 2 B, 3 N / ?), 2 q == a, 3 q == b, 4 a == b, 5 ignored
  unsigned long long tot_local = 0ull;
  for (int i = tid; i < L; i += CH_THREADS)
    {
      const unsigned qv = q[i], av = ac[i], bv = bc[i];
      const bool zero = qv == 0u || av == 0u || bv == 0u;
      bool ign = zero || ambiguous4(qv) || ambiguous4(av) || ambiguous4(bv);
      if (((ins[i >> 5] >> (i & 31)) & 1u) || ((ins[(i + 1) >> 5] >> ((i + 1) & 31)) & 1u)) ign = true;   // insertion column beside
      if (i > 0 && (q[i - 1] == 0 || ac[i - 1] == 0 || bc[i - 1] == 0)) ign = true;
      if (i + 1 < L && (q[i + 1] == 0 || ac[i + 1] == 0 || bc[i + 1] == 0)) ign = true;
      unsigned c = 0u;
      if (!zero)
        {
          if (av == bv) c = qv == av ? 0u : 3u;
          else c = qv == av ? 1u : (qv == bv ? 2u : 3u);
        }
      cat[i] = (uint8_t) (c | ((qv == av) ? 4u : 0u) | ((qv == bv) ? 8u : 0u) | ((av == bv) ? 16u : 0u) | (ign ? 32u : 0u));
      if (!ign && c) tot_local += 1ull << (21 * (c - 1));
    }
  if (tot_local) atomicAdd(&s_tot, tot_local);
  __syncthreads();
  const unsigned long long tot = s_tot;
  const int sumA = (int) (tot & M21), sumB = (int) ((tot >> 21) & M21), sumN = (int) (tot >> 42);

  // left / right counts by prefix scan, h per column, the thread's best in ascending column order
  double bh = -1.0;
  int bi = -1;
  unsigned long long bpk = 0ull;
  unsigned long long carry = 0ull;
  for (int base = 0; base < L; base += CH_THREADS)
    {
      const int i = base + tid;
      unsigned long long v = 0ull;
      if (i < L)
        {
          const unsigned fl = cat[i];
          if (!(fl & 32u) && (fl & 3u)) v = 1ull << (21 * ((fl & 3u) - 1));
        }
      unsigned long long chunk = 0ull;
      const unsigned long long incl = vsxd::block_scan<CH_WAVES>(v, s_wsum, &chunk) + carry;
      carry += chunk;
      if (v)
        {
          const int left_y = (int) (incl & M21), left_n = (int) ((incl >> 21) & M21), left_a = (int) (incl >> 42);
          const int right_n = sumA - left_y, right_y = sumB - left_n, right_a = sumN - left_a;
          if ((left_y > left_n) && (right_y > right_n))
            {
              const double left_h = left_y / ((P.xn * (left_n + P.dn)) + left_a);
              const double right_h = right_y / ((P.xn * (right_n + P.dn)) + right_a);
              const double h = left_h * right_h;
              if (h > bh) { bh = h; bi = i; bpk = incl; }
            }
          else if ((left_n > left_y) && (right_n > right_y))
            {
              const double left_h = left_n / ((P.xn * (left_y + P.dn)) + left_a);
              const double right_h = right_n / ((P.xn * (right_y + P.dn)) + right_a);
              const double h = left_h * right_h;
              if (h > bh) { bh = h; bi = i; bpk = incl | (1ull << 63); }
            }
        }
    }
  s_h[tid] = bh;
  s_i[tid] = bi;
  s_pk[tid] = bpk;
  __syncthreads();
  if (tid == 0)
    {
      int bt = -1;
      for (int t = 0; t < CH_THREADS; ++t)
        if (s_i[t] >= 0 && (bt < 0 || s_h[t] > s_h[bt] || (s_h[t] == s_h[bt] && s_i[t] < s_i[bt]))) bt = t;
      s_best = bt;
    }
  __syncthreads();
  const int bt = s_best;
  const uint32_t seq0 = it.cand[parent[0]], seq1 = it.cand[parent[1]];
  if (bt < 0)
    {
      if (tid == 0) write_unscored(res, VSX_CHIMERA_NO_ALIGNMENT, seq0, seq1);
      return;
    }
  const int best_i = s_i[bt];
  const bool rev = (s_pk[bt] >> 63) != 0ull;

  // QA / QB / AB / QM over the columns not ignored (A and B swap when the reverse orientation won)
  int cols = 0, mqa = 0, mqb = 0, mab = 0, mqm = 0;
  for (int i = tid; i < L; i += CH_THREADS)
    {
      const unsigned fl = cat[i];
      if (fl & 32u) continue;
      const int qa0 = (int) ((fl >> 2) & 1u), qb0 = (int) ((fl >> 3) & 1u);
      const int qa = rev ? qb0 : qa0, qb = rev ? qa0 : qb0;
      ++cols;
      mqa += qa;
      mqb += qb;
      mab += (int) ((fl >> 4) & 1u);
      mqm += i <= best_i ? qa : qb;
    }
  if (cols) atomicAdd(&s_cnt[0], cols);
  if (mqa) atomicAdd(&s_cnt[1], mqa);
  if (mqb) atomicAdd(&s_cnt[2], mqb);
  if (mab) atomicAdd(&s_cnt[3], mab);
  if (mqm) atomicAdd(&s_cnt[4], mqm);
  __syncthreads();
  if (tid != 0) return;

  const unsigned long long pk = s_pk[bt] & ~(1ull << 63);
  const int left_y = (int) (pk & M21), left_n = (int) ((pk >> 21) & M21), left_a = (int) (pk >> 42);
  const int right_n = sumA - left_y, right_y = sumB - left_n, right_a = sumN - left_a;
  vsx_chimera_result r = {};
  r.score = s_h[bt];
  r.status = VSX_CHIMERA_SCORED;
  r.left_yes = rev ? left_n : left_y;
  r.left_no = rev ? left_y : left_n;
  r.left_abstain = left_a;
  r.right_yes = rev ? right_n : right_y;
  r.right_no = rev ? right_y : right_n;
  r.right_abstain = right_a;
  const int c0 = s_cnt[0];
  const double QA = 100.0 * s_cnt[1] / c0;
  const double QB = 100.0 * s_cnt[2] / c0;
  const double AB = 100.0 * s_cnt[3] / c0;
  const double QT = QA < QB ? QB : QA;                      // std::max(QA, QB)
  const double QM = 100.0 * s_cnt[4] / c0;
  const double divdiff = QM - QT;
  r.parent_a = rev ? seq1 : seq0;
  r.parent_b = rev ? seq0 : seq1;
  r.closest = QA >= QB ? r.parent_a : r.parent_b;
  r.id_query_model = QM;
  r.id_query_a = QA;
  r.id_query_b = QB;
  r.id_a_b = AB;
  r.id_query_top = QT;
  r.divergence = divdiff;
  const int sumL = r.left_no + r.left_abstain + r.left_yes, sumR = r.right_no + r.right_abstain + r.right_yes;
  r.flag = 'N';
  if (P.variant >= 2)
    {
      if (s_cnt[4] == c0 && QT < 100.0) r.flag = 'Y';          // uchime2 / uchime3 (chimera.cpp:1633-1640): a perfect model, no '?'
    }
  else if (r.score >= P.minh)
    {
      r.flag = '?';
      if ((divdiff >= P.mindiv) && (sumL >= P.mindiffs) && (sumR >= P.mindiffs)) r.flag = 'Y';
    }
  *res = r;
}

}  // namespace

extern "C" hipError_t vsx_launch_chimera_eval(const VsxChimItem * d_items, uint32_t nitems, const uint8_t * qcodes, const uint64_t * qoff,
                                              const uint32_t * qlen, const uint8_t * tcodes, const uint64_t * toff, const uint32_t * tlen,
                                              const VsxPairOut * d_hits, const uint32_t * d_runs, uint64_t n_runs, VsxChimParams P,
                                              void * d_out, hipStream_t st)
{
  if (nitems == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_chimera_eval_kernel, dim3(nitems), dim3(CH_THREADS), 0, st, d_items, qcodes, qoff, qlen, tcodes, toff, tlen,
                     d_hits, d_runs, n_runs, P, static_cast<vsx_chimera_result *>(d_out));
  return hipGetLastError();
}
