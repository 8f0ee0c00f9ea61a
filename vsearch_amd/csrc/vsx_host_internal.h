// vsx_host_internal.h -- the aligner's host types: what the files that implement include/vsx.h share (vsx_context.cpp, vsx_seqset.cpp,
// vsx_plan.cpp, vsx_fetch.cpp, vsx_align_pairs.cpp).  Host-only C++; no other file of the library sees inside a context, a sequence
// set or a plan (they use the hooks of vsx_private.h).
#ifndef VSX_HOST_INTERNAL_H
#define VSX_HOST_INTERNAL_H

#include "../../include/vsx.h"
#include "vsx_internal.h"
#include "vsx_private.h"

#include <hip/hip_runtime.h>
#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

// (hidden, like vsxp: nothing here is a dynamic symbol of the library)
namespace vsxh __attribute__((visibility("hidden"))) {

inline int sat16(int x) { return x > 32767 ? 32767 : (x < -32768 ? -32768 : x); }

inline bool fits(int64_t q, int64_t d)      // search16_fits, core/align_simd.cpp:130-134
{
  return (q + d <= VSX_MAX_SEQLEN_SUM) && (q * d <= VSX_MAX_SEQLEN_PRODUCT);
}

// Scratch pool: hipMalloc/hipFree of the multi-GB checkpoint, slab and run buffers cost seconds per plan (page-table
// set-up), far more than the kernels of a 500 k-pair stage.  A context keeps the blocks its finished plans give back and
// hands them to the next plan (best fit, but never a block more than 4x + 1 MB larger than the request: a retired multi-GB
// checkpoint block must not end up pinned under an 8-byte cursor).  vsx_destroy frees everything.
struct PoolBlock { void * p; size_t bytes; };
struct ScratchPool {
  std::vector<PoolBlock> free_blocks;
  std::mutex mu;
  bool retired = false;                 // the owning context is gone (sequence sets may outlive it): nothing is kept any more
  ~ScratchPool() { for (PoolBlock & b : free_blocks) (void) hipFree(b.p); }
  hipError_t get(size_t bytes, void ** out, size_t * got)
  {
    if (bytes == 0) bytes = 1;
    {
      std::lock_guard<std::mutex> lk(mu);
      size_t best = SIZE_MAX;
      const size_t limit = bytes > (SIZE_MAX >> 3) ? SIZE_MAX : 4 * bytes + (1u << 20);
      for (size_t k = 0; k < free_blocks.size(); ++k)
        if (free_blocks[k].bytes >= bytes && free_blocks[k].bytes <= limit &&
            (best == SIZE_MAX || free_blocks[k].bytes < free_blocks[best].bytes)) best = k;
      if (best != SIZE_MAX)
        {
          *out = free_blocks[best].p; *got = free_blocks[best].bytes;
          free_blocks.erase(free_blocks.begin() + (long) best);
          vsx_internal_poison(*out, std::min<size_t>(*got, (size_t) 256 << 20));
          return hipSuccess;
        }
    }
    if (bytes >= ((size_t) 16 << 20))
      {
        // (r05) never fill the device to the brim: the runtime needs room of its own (kernel scratch of every queue) and aborts the
        // process when it finds none -- profiles/r05/r05b_config5_share_abort.txt.  Below the reserve, idle blocks go first.
        // r06: only as much as restores the reserve -- this pool's largest idle blocks first, the other contexts of the device
        // only if that was not enough -- and said once: on a device that stays near full every plan would otherwise re-hipMalloc its
        // multi-GB blocks (seconds apiece) and the warm-call promise of the pools would vanish silently.
        size_t free_b = 0, total_b = 0;
        int dev = 0;
        const size_t need = bytes + VSX_DEVICE_RESERVE_BYTES;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b < need && hipGetDevice(&dev) == hipSuccess)
          {
            static std::atomic<bool> said {false};
            if (!said.exchange(true))
              std::fprintf(stderr, "vsx: device %d is nearly full (%.1f GB free, %.1f GB wanted + 6 GB reserve): idle scratch blocks are being "
                                   "returned; later plans re-allocate theirs (said once)\n", dev, free_b / 1e9, bytes / 1e9);
            if (!trim_until(need)) (void) vsx_internal_memory_pressure(dev);
          }
        (void) hipGetLastError();
      }
    // (an out-of-memory answer makes every context of the device, this pool's own included, free what is idle, and is asked again)
    const hipError_t e = vsxp::device_malloc(out, bytes);
    if (e == hipSuccess) { *got = bytes; vsx_internal_poison(*out, std::min<size_t>(bytes, (size_t) 256 << 20)); }
    return e;
  }
  void put(void * p, size_t bytes)
  {
    if (!p) return;
    std::lock_guard<std::mutex> lk(mu);
    if (retired) { (void) hipFree(p); return; }
    free_blocks.push_back(PoolBlock {p, bytes});
    while (free_blocks.size() > 64)                       // bound the number of idle blocks: drop the smallest
      {
        size_t m = 0;
        for (size_t k = 1; k < free_blocks.size(); ++k) if (free_blocks[k].bytes < free_blocks[m].bytes) m = k;
        (void) hipFree(free_blocks[m].p);
        free_blocks.erase(free_blocks.begin() + (long) m);
      }
  }
  size_t idle_bytes()
  {
    std::lock_guard<std::mutex> lk(mu);
    size_t t = 0;
    for (const PoolBlock & b : free_blocks) t += b.bytes;
    return t;
  }
  void trim()
  {
    std::lock_guard<std::mutex> lk(mu);
    for (PoolBlock & b : free_blocks) (void) hipFree(b.p);
    free_blocks.clear();
  }
  // free idle blocks, largest first, until the device reports `want_free` bytes free; false: the pool ran dry first
  bool trim_until(size_t want_free)
  {
    std::lock_guard<std::mutex> lk(mu);
    for (;;)
      {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b >= want_free) return true;
        if (free_blocks.empty()) return false;
        size_t m = 0;
        for (size_t k = 1; k < free_blocks.size(); ++k) if (free_blocks[k].bytes > free_blocks[m].bytes) m = k;
        (void) hipFree(free_blocks[m].p);
        free_blocks.erase(free_blocks.begin() + (long) m);
      }
  }
  void retire() { trim(); std::lock_guard<std::mutex> lk(mu); retired = true; }
};

template <typename T>
struct PoolBuf {
  T * p = nullptr;
  size_t n = 0, bytes = 0;
  ScratchPool * pool = nullptr;
  ~PoolBuf() { release(); }
  void release() { if (p && pool) pool->put(p, bytes); else if (p) (void) hipFree(p); p = nullptr; n = 0; bytes = 0; }
  hipError_t alloc(ScratchPool * pl, size_t count)       // pl == nullptr: plain hipMalloc / hipFree
  {
    release();
    pool = pl;
    if (count == 0) count = 1;
    void * q = nullptr;
    size_t got = count * sizeof(T);
    hipError_t e = pl ? pl->get(count * sizeof(T), &q, &got) : hipMalloc(&q, count * sizeof(T));
    if (e == hipSuccess) { p = static_cast<T *>(q); n = count; bytes = got; }
    return e;
  }
};

// Stream-ordered scratch shared by the plans of one context: checkpoints and the traceback slab are dead once a plan's
// kernels have finished, and the plans of a context execute in order on its streams, so they can all use ONE block (the
// next plan's kernels are queued behind the previous plan's traceback).  A plan holds a reference; a larger request
// replaces the context's current block, the old one goes back to the pool when its last plan dies.
struct SharedBlock {
  void * p = nullptr;
  size_t bytes = 0;
  ScratchPool * pool = nullptr;
  ~SharedBlock() { if (p) { if (pool) pool->put(p, bytes); else (void) hipFree(p); } }
};
struct SharedSlot;
extern thread_local const SharedSlot * tl_acquiring_slot;      // the slot whose lock THIS thread holds inside acquire() (try_reset); vsx_context.cpp
struct SharedSlot {
  std::mutex mu;
  std::shared_ptr<SharedBlock> cur;
  hipError_t acquire(ScratchPool * pool, size_t bytes, std::shared_ptr<SharedBlock> & out, bool headroom = true)
  {
    std::lock_guard<std::mutex> lk(mu);
    struct Mark { const SharedSlot * prev; explicit Mark(const SharedSlot * s) : prev(tl_acquiring_slot) { tl_acquiring_slot = s; } ~Mark() { tl_acquiring_slot = prev; } } mark(this);
    if (cur && cur->bytes >= bytes) { out = cur; return hipSuccess; }
    cur.reset();                       // (r05) too small: back to the pool as soon as no plan holds it, where memory pressure can free it
    auto b = std::make_shared<SharedBlock>();
    static const bool dbg = std::getenv("VSX_DEBUG_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    // a little headroom: the slices of a pipeline differ by a few per cent, and replacing a multi-GB block costs a hipMalloc
    hipError_t e = pool->get(headroom ? bytes + bytes / 8 : bytes, &b->p, &b->bytes);
    if (dbg) std::fprintf(stderr, "  shared block: %zu bytes wanted (had %zu), got %zu in %.2f ms\n", bytes, cur ? cur->bytes : (size_t) 0, b->bytes,
                          std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3);
    if (e == hipErrorOutOfMemory) { (void) hipGetLastError(); e = pool->get(bytes, &b->p, &b->bytes); }
    if (e != hipSuccess) { b->p = nullptr; return e; }
    b->pool = pool;
    cur = b;
    out = b;
    return hipSuccess;
  }
  void reset() { std::lock_guard<std::mutex> lk(mu); cur.reset(); }
  // (memory pressure may be raised from INSIDE an acquire of this very slot, whose lock is then held by the caller: skip it -- by the
  //  thread-local mark, not by try_lock on a mutex the caller owns, which is undefined; the try_lock that remains is for
  //  slots held by OTHER threads, which may themselves be waiting for a slot of ours)
  void try_reset() { if (tl_acquiring_slot == this) return; if (mu.try_lock()) { cur.reset(); mu.unlock(); } }
  size_t bytes() { std::lock_guard<std::mutex> lk(mu); return cur ? cur->bytes : 0; }
};
template <typename T>
struct SharedBuf {
  std::shared_ptr<SharedBlock> blk;
  T * p = nullptr;
  hipError_t alloc(SharedSlot & slot, ScratchPool * pool, size_t count)
  {
    hipError_t e = slot.acquire(pool, std::max<size_t>(count, 1) * sizeof(T), blk);
    p = (e == hipSuccess) ? static_cast<T *>(blk->p) : nullptr;
    return e;
  }
};

// The kernel class of a task: which instantiation of the DP kernel runs it.  The planner groups, merges, sorts and cuts launches by it.
struct KernelClass {
  int rows; int track; int tilt; int nq /* tasks per wave: 1, or 2 / 4 = a sparse-task class; 8 = pair profile, 16 = split profile */;
  bool operator==(const KernelClass & o) const { return rows == o.rows && track == o.track && tilt == o.tilt && nq == o.nq; }
  bool operator!=(const KernelClass & o) const { return !(*this == o); }
  // the order of the launches of a chunk: the nq variants of one (rows, track, tilt) are adjacent
  bool operator<(const KernelClass & o) const
  {
    if (rows != o.rows) return rows < o.rows;
    if (track != o.track) return track < o.track;
    if (tilt != o.tilt) return tilt < o.tilt;
    return nq < o.nq;
  }
  bool same_but_rows(const KernelClass & o) const { return track == o.track && tilt == o.tilt && nq == o.nq; }
  // the traceback does not know about nq: the nq variants of a class share one traceback launch
  bool same_traceback(const KernelClass & o) const { return rows == o.rows && track == o.track && tilt == o.tilt; }
  const KernelClass & cls() const { return *this; }
};

struct Launch : KernelClass {
  uint32_t first, count; uint32_t pair_first, pair_count;
  bool multi = false /* r06: some task of the launch spans several strips (Q > 16 rows): the general kernel; otherwise the ONE variants */;
};

struct Chunk {
  uint32_t task_first = 0, task_count = 0;
  uint32_t pair_first = 0, pair_count = 0;      // into the gpu-pair arrays
  std::vector<Launch> launches;
  // (a chunk's checkpoint block starts and ends with VSX_CK_SLACK_DW dwords nobody writes: the traceback reads the nine row-checkpoint
  //  pairs around a tile without clamping their addresses -- vsx_internal.h)
  uint64_t dir_dwords = VSX_CK_SLACK_DW, strip_elems = 0, slab_words = 0;
  hipEvent_t e0 = nullptr, e1 = nullptr, e1b = nullptr, e2 = nullptr;   // DP begin/end (stream), traceback begin/end (stream2)
};

// Where a plan's results go: arrays of the caller (already offset to the plan's first pair), a growing text blob.
struct FetchDest {
  int16_t * score; uint16_t * aligned, * matches, * mismatches, * gaps; uint64_t * cigar_off; uint8_t * verdict;
  char ** blob; uint64_t * blob_used;      // text is appended at *blob_used (the blob is realloc'ed); offsets are rebased by it
};

// Ranked fetch: only the pairs the plan's filter kept, in report order, appended to a sink.
struct RankedSink {
  std::vector<uint32_t> pair, undecided;
  std::vector<int16_t> score;
  std::vector<uint16_t> aligned, matches, mismatches, gaps;
  std::vector<uint8_t> verdict;
  std::vector<double> id;
  std::vector<uint64_t> cigar_off;
  char * blob = nullptr;
  uint64_t blob_used = 0;
  int keep_weak = 0;
  ~RankedSink() { std::free(blob); }
};

template <typename T>
T * dup_array(const std::vector<T> & v)
{
  T * p = (T *) std::malloc(std::max<size_t>(v.size(), 1) * sizeof(T));
  if (p && !v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}

// threads for a host pass over n items that is worth a thread per `grain` of them
inline int pass_threads(uint64_t n, uint64_t grain)
{
  return (int) std::max<uint64_t>(1, std::min<uint64_t>((uint64_t) vsx_internal_usable_cpus(), n / grain));
}
// threads for a memory-bound host pass over `bytes` bytes
inline int copy_threads(uint64_t bytes) { return pass_threads(bytes, (uint64_t) 1 << 21); }

// thread t's contiguous share [lo, hi) of n items among nth threads
struct Slice { uint64_t lo, hi; };
inline Slice slice_of(uint64_t n, int t, int nth)
{
  return Slice {n * (uint64_t) t / (uint64_t) nth, n * (uint64_t) (t + 1) / (uint64_t) nth};
}

// f(0) on the caller, f(1) ... f(nth - 1) on the host worker pool (the WorkerPool of vsx_context.cpp)
template <typename F>
void run_threads(int nth, F && f) { vsxp::run_pool(nth, f); }

// per device: 0 = not tested yet, 1 = v_pk_maximum3_f16 is the integer maximum on [0, 0x7BFF] (vsx_create's self-test), 2 = it is not
extern std::atomic<int> g_max3_state[64];      // vsx_context.cpp

int pick_rows(int Q);                                                                              // vsx_plan.cpp
int plan_set_ranked(vsx_plan * pl);
int ensure_impure(const vsx_seqset * s);                                                           // vsx_seqset.cpp
int fetch_core(vsx_plan * pl, const FetchDest & D);                                                // vsx_fetch.cpp
int fetch_ranked_core(vsx_plan * pl, uint64_t first, const uint32_t * qkey, RankedSink & S);
int results_alloc(vsx_results * out, uint64_t n, bool with_verdict);
FetchDest dest_at(vsx_results * out, uint64_t first);

}  // namespace vsxh

// the opaque types of include/vsx.h (global names); their members are vsxh types
using vsxp::DevBuf;
using vsxh::ScratchPool; using vsxh::PoolBuf; using vsxh::SharedSlot; using vsxh::SharedBuf; using vsxh::Chunk;

struct vsx_ctx {
  int device = 0;
  hipStream_t stream = nullptr;      // DP kernels, copies
  hipStream_t stream2 = nullptr;     // traceback kernels (overlap with the next chunk's DP)
  hipStream_t stream_b = nullptr;    // DP kernels of every other pipelined slice (vsx_align_pairs): the next launch fills this one's tail
  hipStream_t stream_up = nullptr;   // plan uploads (a plan may be created while another one runs: vsx_align_pairs pipeline)
  hipStream_t stream_dn = nullptr;   // result downloads (vsx_plan_fetch of slice i-1 while slice i's kernels occupy `stream`)
  vsx_scoring sc {};
  bool force_fallback = false;      // a score/penalty left the 16-bit range: every pair -> sentinel
  bool tb_packed = false;           // VSX_TB_ARITH=packed: plan every task into the TRACK = 1 class (saturating packed ops, capture layout)
  int pen[12] {};                   // clamped CELL penalties: go_q_l, go_t_l, go_q_i, go_t_i, go_q_r, go_t_r, ge_*
  VsxDevParams P {};
  DevBuf<int16_t> d_htop, d_hleft, d_matrix;
  VsxDevParams Pt {};               // the same scoring in TILTED coordinates (VsxDevParams::tilt, vsx_forward_kernel TILT); Pt.tilt == 0: unavailable
  DevBuf<int16_t> d_htop_t, d_hleft_t, d_matrix_t;
  std::shared_ptr<ScratchPool> pool_owner = std::make_shared<ScratchPool>();   // sequence sets hold a reference (they may outlive the context)
  ScratchPool & pool = *pool_owner;
  // Two checkpoint blocks, used alternately by the plans of the context: the DP kernels of plan i+1 run while the traceback of
  // plan i still reads its block, so the launch tails of one fill with the other's waves (a pipeline of small plans lost 15 %
  // to tails when every plan waited for its predecessor's traceback: r02 timeline in DESIGN 5).  ev_tb[s] = "the last traceback
  // that read block s has finished".
  // r04: THREE blocks.  In a pipeline of slices the DP kernel of slice i + 2 used to wait for the
  // traceback of slice i, which shares the device with the DP kernel of slice i + 1 on bad terms (rocprofv3 trace of one call,
  // profiles/r03/r03v_e2e_trace_*.csv); with a third block only slice i + 3 waits for it.  A block is sized by the largest plan that
  // used it (<= 0.4 of what is free when it is made), 20 GB for the 200 k-pair slices of the bench shape.
  SharedSlot shared_dir[3], shared_slab;   // declared after the pool: released first
  std::atomic<uint64_t> req_hwm[2] {{0}, {0}};      // largest checkpoint block / slab a plan of this context asked for since the last reset (bytes)
  hipEvent_t ev_tb[3] = {nullptr, nullptr, nullptr};
  bool ev_tb_used[3] = {false, false, false};
  std::atomic<unsigned> plan_seq {0};
  // r06: which block a new plan takes (vsx_plan_create).  slot_refs[s] = live plans on block s (a plan is destroyed after its traceback
  // has finished), slot_stamp[s] = plan_seq at the last acquisition.
  std::mutex slot_mu;
  int slot_refs[3] = {0, 0, 0};
  unsigned slot_stamp[3] = {0, 0, 0};
  // pinned host memory: results cross PCIe into it (vsx_plan_fetch), one fetch at a time; grow-only
  std::mutex stage_mu;
  uint8_t * stage = nullptr;
  size_t stage_bytes = 0;
  std::vector<unsigned long long *> cursor_slots;   // idle pinned {run cursor, text cursor} pairs of finished plans
  // what settle_runs() / settle() had to repeat: [0] plans run again for the run buffer, [1] text kernels run again (vsx_internal_settle_counts)
  std::atomic<uint64_t> settle_counts[2] {{0}, {0}};
  ~vsx_ctx()
  {
    for (hipEvent_t e : ev_tb) if (e) (void) hipEventDestroy(e);
    if (stage) (void) hipHostFree(stage);
    for (auto * c : cursor_slots) (void) hipHostFree(c);
  }
};

#define VSX_SEQSET_POOLED_BYTES (64ull << 20)
struct vsx_seqset {
  vsx_ctx * ctx = nullptr;
  int device = 0;
  uint64_t n = 0;
  uint64_t bytes = 0;
  std::vector<uint64_t> off;
  std::vector<uint32_t> len;
  // Device buffers of sets up to VSX_SEQSET_POOLED_BYTES come from the context's scratch pool and go back to it: a search creates
  // one query set per window, and hipMalloc / hipFree synchronise the WHOLE device -- with the k-mer counting kernel of the next
  // window running that was an 8-11 ms stall per window (r03 timeline); large sets (databases) use hipMalloc as before.
  std::shared_ptr<ScratchPool> pool_ref;   // keeps the pool alive; declared BEFORE the buffers, so it is destroyed after them
  PoolBuf<uint8_t> d_codes;         // VSX_CODE_SLACK bytes | codes | VSX_CODE_SLACK bytes: the traceback stages rows/columns with unaligned dword loads
  uint8_t * codes() const { return d_codes.p + VSX_CODE_SLACK; }
  PoolBuf<uint64_t> d_off;
  PoolBuf<uint32_t> d_len;
  // soft masking for the k-mer index only (vsx_internal_seqset_create_cased): one bit per blob byte, set where the symbol was
  // not an upper-case A C G T U.  The aligner never sees it: alignment is case-blind in the reference too (chrmap_4bit)
  PoolBuf<uint8_t> d_lower;
  uint64_t lower_bytes = 0;
  // pair-profile classes only: per-sequence "contains a non-ACGT symbol", computed on first use (vsx_purity_kernel) under the lock
  mutable std::mutex impure_mu;
  mutable std::vector<uint8_t> impure;
  mutable bool have_impure = false;
};

struct vsx_plan {
  vsx_ctx * ctx = nullptr;
  const vsx_seqset * Q = nullptr;
  const vsx_seqset * T = nullptr;
  uint64_t n_pairs = 0;
  VsxFilterDev filter {};                // accept filter evaluated by the traceback kernel (enabled == 0: none)
  std::vector<VsxPairOut> host_out;      // answers of the closed-form / sentinel pairs, parallel to host_pairs
  std::vector<std::string> host_cigar;   // only for the Q == 0 closed form
  std::vector<uint32_t> host_cigar_pair;
  std::vector<uint32_t> host_cigar_run;  // the same alignments as run words ((D << 2) | I), for the exported run buffer

  std::vector<VsxTask> tasks;
  std::vector<uint32_t> pair_slot, pair_ids;
  std::vector<uint64_t> slab_off;
  std::vector<Chunk> chunks;
  uint64_t cells = 0, dir_bytes_total = 0;

  // every device buffer comes from the context's pool (hipFree synchronises the device: it would stall a pipeline of plans)
  PoolBuf<VsxTask> d_tasks;
  PoolBuf<uint32_t> d_pair_slot, d_pair_ids;
  SharedBuf<uint32_t> d_dir[1], d_slab;         // stream-ordered scratch shared by the context's plans
  int dir_slot = 0;                             // which of the context's checkpoint blocks
  bool slot_held = false;                       // counted in ctx->slot_refs[dir_slot]
  bool alt_fwd = false;                         // DP kernels on the context's second DP stream (pipelined slices, see vsx_align_pairs)
  PoolBuf<uint32_t> d_runs;
  PoolBuf<uint64_t> d_slab_off;
  PoolBuf<uint2> d_strip;
  PoolBuf<VsxSlotOut> d_slot;
  PoolBuf<VsxPairOut> d_out;
  PoolBuf<unsigned long long> d_cursor;  // [0] run words used, [1] text bytes used, [2] DP steps skipped (vsx_forward_kernel EARLY)
  PoolBuf<uint8_t> d_text, d_soa;        // CIGAR text and the output arrays, written by the traceback epilogues (vsx_tbtext.h)
  // r06, ranked plans: the lists the traceback's epilogue fills (VsxFilterDev::rank_counts ...), see plan_set_ranked()
  PoolBuf<uint32_t> d_rank_counts, d_kept_pair, d_refused_pair;
  PoolBuf<double> d_kept_id;
  VsxSoaOut soa {};
  uint64_t soa_bytes = 0, soa_off[7] {};
  uint64_t text_capacity = 0;
  unsigned long long * h_cursor = nullptr;   // pinned copy of d_cursor, filled at the end of a run
  std::vector<uint32_t> host_pairs;      // pairs answered without DP (sentinels, empty query), ascending
  uint64_t runs_capacity = 0;
  hipEvent_t ev_begin = nullptr, ev_end = nullptr;
  bool ran = false;
  bool host_patched = false;

  ~vsx_plan()
  {
    for (auto & c : chunks)
      {
        if (c.e0) (void) hipEventDestroy(c.e0);
        if (c.e1) (void) hipEventDestroy(c.e1);
        if (c.e1b) (void) hipEventDestroy(c.e1b);
        if (c.e2) (void) hipEventDestroy(c.e2);
      }
    if (ev_begin) (void) hipEventDestroy(ev_begin);
    if (ev_end) (void) hipEventDestroy(ev_end);
    if (h_cursor) { std::lock_guard<std::mutex> lk(ctx->stage_mu); ctx->cursor_slots.push_back(h_cursor); }
    if (slot_held) { std::lock_guard<std::mutex> lk(ctx->slot_mu); --ctx->slot_refs[dir_slot]; }
  }
};

#endif
