// vsx_context.cpp -- host side of libvsx, the context: the C-ABI of include/vsx.h is implemented by this file (vsx_create, vsx_destroy,
// the scratch pool, the host worker pool, the vsx_internal_* hooks of vsx_private.h), vsx_seqset.cpp (sequence sets), vsx_plan.cpp
// (batch planning: pairs -> wavefront tasks -> direction-buffer chunks; run, sync, describe), vsx_fetch.cpp (result marshalling) and
// vsx_align_pairs.cpp (the pipelined one-call form).  Their shared types are in vsx_host_internal.h.
//
// Reference seams replaced here (see include/vsx.h for per-function citations):
//   search16_init/exit/qprep/search16            src/core/align_simd.cpp:1282-2060
//   the "<= 8 targets per call" batch shape      src/core/searchcore.cpp:757-778
// Everything that touches sequence data runs on the GPU; the host only groups indices, evaluates the
// reference's closed-form special cases (empty query / empty target / size guard / forced fallback)
// and turns run lists into CIGAR text.
#include "vsx_host_internal.h"

#include <cerrno>
#include <sched.h>
#include <condition_variable>
#include <deque>
#include <functional>
#include <thread>

using vsxp::fail;
using namespace vsxh;

static thread_local std::string g_err;
static std::mutex g_ctx_mu;                   // the live contexts of the process (vsx_internal_memory_pressure)
static std::vector<vsx_ctx *> g_ctxs;
thread_local const SharedSlot * vsxh::tl_acquiring_slot = nullptr;
std::atomic<int> vsxh::g_max3_state[64];

// Host worker pool: a plan is built in a dozen short parallel passes (validation, classification, grouping, task tables; the
// fetch spreads its copies); spawning std::threads for each cost more than the passes themselves on 200 k-pair slices.  Workers
// are created once per process; a parallel region pushes its tasks, runs task 0 itself, helps with the queue and waits for its
// own tasks only -- regions of different host threads (the planner of a pipeline, the fetching caller) interleave freely.
namespace {
class WorkerPool {
 public:
  static WorkerPool & get() { static WorkerPool p; return p; }
  template <typename F>
  void run(int nth, F && f)
  {
    if (nth <= 1) { f(0); return; }
    // `left` is only touched under `m`: a worker's last access to the region is its unlock, and the caller can see left == 0 only
    // after locking behind it -- the region lives on the caller's stack and must not be touched once run() returns
    struct Region { int left; std::mutex m; std::condition_variable cv; };
    Region rg;
    rg.left = nth - 1;
    {
      std::lock_guard<std::mutex> lk(mu_);
      for (int t = 1; t < nth; ++t)
        queue_.push_back([&f, &rg, t]() {
          f(t);
          std::lock_guard<std::mutex> lk2(rg.m);
          if (--rg.left == 0) rg.cv.notify_all();
        });
    }
    cv_.notify_all();
    f(0);
    // help: run queued tasks (ours or another region's) instead of sleeping while ours are pending
    for (;;)
      {
        { std::lock_guard<std::mutex> lk(rg.m); if (rg.left == 0) break; }
        std::function<void()> job;
        {
          std::lock_guard<std::mutex> lk(mu_);
          if (!queue_.empty()) { job = std::move(queue_.front()); queue_.pop_front(); }
        }
        if (job) { job(); continue; }
        std::unique_lock<std::mutex> lk(rg.m);
        if (rg.cv.wait_for(lk, std::chrono::microseconds(50), [&] { return rg.left == 0; })) break;
      }
  }
 private:
  WorkerPool()
  {
    const int n = std::max(1, vsx_internal_usable_cpus() - 1);
    for (int i = 0; i < n; ++i)
      workers_.emplace_back([this]() {
        for (;;)
          {
            std::function<void()> job;
            {
              std::unique_lock<std::mutex> lk(mu_);
              cv_.wait(lk, [&] { return stop_ || !queue_.empty(); });
              if (stop_ && queue_.empty()) return;
              job = std::move(queue_.front());
              queue_.pop_front();
            }
            job();
          }
      });
  }
  ~WorkerPool()
  {
    { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
    cv_.notify_all();
    for (auto & w : workers_) w.join();
  }
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::function<void()>> queue_;
  std::vector<std::thread> workers_;
  bool stop_ = false;
};
}  // namespace

extern "C" {

// VSX_POISON (vsx_private.h): -1 = off, else the fill byte.  The environment is read once per process.
int vsx_internal_poison_byte(void)
{
  static const int byte = [] {
    if (!std::getenv("VSX_POISON")) return -1;
    int b = 0xA5;
    if (const char * s = std::getenv("VSX_POISON_BYTE"))
      {
        char * end = nullptr;
        errno = 0;
        const bool hex = s[0] == '0' && (s[1] == 'x' || s[1] == 'X');
        const long v = std::strtol(s, &end, hex ? 16 : 10);
        if (end != s && *end == '\0' && errno == 0 && v >= 0 && v <= 255) b = (int) v;
        else std::fprintf(stderr, "vsx: VSX_POISON_BYTE=%s is not a byte (0 .. 255, decimal or 0x..): filling with 0x%02X\n", s, b);
      }
    return b;
  }();
  return byte;
}
void vsx_internal_poison(void * p, size_t bytes)
{
  const int byte = vsx_internal_poison_byte();
  if (byte >= 0 && p && bytes) { (void) hipMemset(p, byte, bytes); (void) hipDeviceSynchronize(); }
}
// the host worker pool of the dispatch layer, vsx_search.cpp and the commands on its searcher (fn(0) runs on the caller, which also helps with queued jobs while it waits)
void vsx_internal_run_threads(int nth, void (*fn)(int, void *), void * arg) { WorkerPool::get().run(nth, [&](int t) { fn(t, arg); }); }
// shared with vsx_search.cpp: one thread-local error slot for the whole library
void vsx_internal_set_error(const char * msg) { g_err = msg ? msg : ""; }
const vsx_scoring * vsx_internal_scoring(const vsx_ctx * ctx) { return &ctx->sc; }
uint64_t vsx_internal_symbols(uint8_t * code, uint8_t * ambiguous, uint8_t * complement, uint8_t * upcase, uint64_t word)
{
  for (uint32_t c = 0; c < 256; ++c)
    {
      code[c] = (uint8_t) vsxsym::map4(c);
      ambiguous[c] = vsxsym::ambiguous4(c) ? 1 : 0;
      complement[c] = (uint8_t) vsxsym::complement(c);
      upcase[c] = (uint8_t) vsxsym::upcase(c);
    }
  return vsxsym::mix64(word);
}
int vsx_internal_usable_cpus(void)
{
  // CPUs this process may really use: affinity mask, capped by a cgroup v2 CPU quota
  int n = (int) std::thread::hardware_concurrency();
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof set, &set) == 0) n = CPU_COUNT(&set);
  if (FILE * f = std::fopen("/sys/fs/cgroup/cpu.max", "r"))
    {
      char q[32]; long long period = 0;
      if (std::fscanf(f, "%31s %lld", q, &period) == 2 && std::strcmp(q, "max") != 0 && period > 0)
        n = std::min<int>(n, (int) std::max<long long>(1, std::atoll(q) / period));
      std::fclose(f);
    }
  return std::max(1, n);
}
// Self-test of the host worker pool (no device): `regions` short parallel regions of `width` tasks each, issued from TWO
// host threads at once (as the planner of a pipeline and the fetching caller do); every task adds its index into a per-region
// slot on the issuing thread's stack.  Returns 0 if every region saw exactly the sum of its task indices.
int vsx_internal_pool_selftest(int regions, int width)
{
  std::atomic<int> bad {0};
  auto driver = [&](int salt) {
    for (int r = 0; r < regions; ++r)
      {
        const int w = 1 + (r * 7 + salt) % std::max(1, width);
        std::vector<long long> part((size_t) w, 0);
        volatile long long guard_before = 0x1122334455667788ll;
        run_threads(w, [&](int t) { part[(size_t) t] += (long long) t + 1; });
        volatile long long guard_after = 0x1122334455667788ll;
        long long sum = 0;
        for (long long v : part) sum += v;
        if (sum != (long long) w * (w + 1) / 2 || guard_before != guard_after) bad.fetch_add(1);
      }
  };
  std::thread other(driver, 3);
  driver(0);
  other.join();
  return bad.load();
}
int vsx_internal_device(const vsx_ctx * ctx) { return ctx->device; }
// r05: device memory under pressure.  A context keeps its big stream-ordered blocks (three checkpoint blocks, the slab) and a pool of
// idle scratch between plans, so that a warm call never meets a multi-GB hipMalloc; after ONE very large plan (BASELINE config 5's
// per-GPU share: 3 x 62 GB of checkpoints) those blocks starved every other allocator of the device -- the k-mer scratch of a search on
// the same GPU failed with "out of memory" (profiles/r05/r05a_config5_share_oom.json).  Whoever meets hipErrorOutOfMemory calls this
// once and retries: every live context of the device drops the blocks no plan holds and frees its idle pool.  Returns the bytes released.
uint64_t vsx_internal_memory_pressure(int device)
{
  std::lock_guard<std::mutex> lk(g_ctx_mu);
  uint64_t freed = 0;
  for (vsx_ctx * c : g_ctxs)
    if (c->device == device)
      {
        SharedSlot * slot[4] = {&c->shared_dir[0], &c->shared_dir[1], &c->shared_dir[2], &c->shared_slab};
        for (SharedSlot * sl : slot) sl->try_reset();      // a block a plan still references lives until that plan dies
        freed += c->pool.idle_bytes();
        c->pool.trim();
      }
  return freed;
}
// The big stream-ordered scratch blocks of a context (three checkpoint blocks, the traceback slab): their sizes, and a reservation
// of at least those sizes.  A search runs its windows on several contexts of one device; a context that meets its first full
// window in the middle of a warm search would pay the multi-GB hipMalloc there (0.5-1 s in a 0.15 s call), so the searcher levels
// the contexts after a call (vsx_search.cpp).
// what the plans of a context asked for since the last reset: {checkpoint block, slab} bytes.  The searcher levels its contexts to
// THESE (r04: it used to level to the blocks the contexts hold, and a context that had also run somebody else's 80 GB plan -- the
// bench's aligner context is the searcher's first -- made every search call try, and fail, to give all contexts 88 GB blocks:
// 13 ms of refused hipMallocs per call)
void vsx_internal_scratch_requests(vsx_ctx * ctx, uint64_t out[2], int reset)
{
  for (int k = 0; k < 2; ++k) out[k] = reset ? ctx->req_hwm[k].exchange(0) : ctx->req_hwm[k].load();
}
void vsx_internal_scratch_sizes(vsx_ctx * ctx, uint64_t out[4])
{
  out[0] = ctx->shared_dir[0].bytes(); out[1] = ctx->shared_dir[1].bytes(); out[2] = ctx->shared_dir[2].bytes(); out[3] = ctx->shared_slab.bytes();
}
int vsx_internal_scratch_reserve(vsx_ctx * ctx, const uint64_t want[4])
{
  if (hipSetDevice(ctx->device) != hipSuccess) { (void) hipGetLastError(); return VSX_EHIP; }
  SharedSlot * slot[4] = {&ctx->shared_dir[0], &ctx->shared_dir[1], &ctx->shared_dir[2], &ctx->shared_slab};
  for (int k = 0; k < 4; ++k)
    if (want[k] > slot[k]->bytes())
      {
        std::shared_ptr<SharedBlock> hold;
        const hipError_t e = slot[k]->acquire(&ctx->pool, (size_t) want[k], hold, true);
        if (e != hipSuccess) { (void) hipGetLastError(); return e == hipErrorOutOfMemory ? VSX_ENOMEM : VSX_EHIP; }
      }
  return VSX_OK;
}
// r06: what the checkpoint block of ONE plan of `ntasks` whole-wave tasks (a query of qlen rows against up to eight targets of tlen columns)
// will ask for -- a caller that knows the largest plan it is going to submit (vsx_cluster_fast: a round of queries, eight candidates each)
// reserves the block once instead of letting it grow over its first rounds
uint64_t vsx_internal_ckpt_bytes_estimate(const vsx_ctx * ctx, uint64_t ntasks, uint32_t qlen, uint32_t tlen)
{
  if (qlen == 0 || tlen == 0) return 0;
  const int rows = pick_rows((int) qlen);
  const uint64_t total_lanes = ((uint64_t) qlen + (uint64_t) rows - 1) / (uint64_t) rows, nstrips = (total_lanes + 15) / 16;
  const uint64_t steps = (((uint64_t) tlen + 3) & ~3ull) + 16;
  const int tilt = ((!ctx || ctx->Pt.tilt != 0) && rows >= 4) ? 1 : 0;      // no context (tests without a device): the compressed layout, the smaller one
  return (ntasks * vsx_ckpt_dwords(nstrips, steps, (uint64_t) rows, tilt) + 2 * VSX_CK_SLACK_DW) * 4;
}
hipStream_t vsx_internal_stream(const vsx_ctx * ctx) { return ctx->stream; }
// a block of the context's scratch pool for a call that is no plan (vsx_otutab): `got` is what goes back with it
hipError_t vsx_internal_scratch_get(vsx_ctx * ctx, size_t bytes, void ** out, size_t * got) { return ctx->pool.get(bytes, out, got); }
void vsx_internal_scratch_put(vsx_ctx * ctx, void * p, size_t got) { ctx->pool.put(p, got); }
// host copies of the set's lengths (the k-mer index build of long words lays its key slots out by their running sum)
const uint32_t * vsx_internal_seqset_host_lengths(const vsx_seqset * s) { return s ? s->len.data() : nullptr; }
void vsx_internal_seqset_device(const vsx_seqset * s, const uint8_t ** codes, const uint64_t ** off, const uint32_t ** len, uint64_t * n)
{
  *codes = s->codes(); *off = s->d_off.p; *len = s->d_len.p; *n = s->n;
}

const char * vsx_version_string(void) { return "libvsx 0.1.0 (gfx950)"; }

const char * vsx_last_error(void) { return g_err.c_str(); }

int vsx_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void) hipGetLastError(); return 0; }
  int usable = 0;
  for (int d = 0; d < n; ++d)
    {
      hipDeviceProp_t p;
      if (hipGetDeviceProperties(&p, d) == hipSuccess && std::strncmp(p.gcnArchName, "gfx950", 6) == 0) ++usable;
    }
  return usable;
}

// ---- vsx_create: one function per step; a step that fails has set the error and the driver gives the context back ----

namespace {
// what the steps hand on: the clamped scores, the host copies of the border chains and the score matrix
struct CtxDraft {
  int match = 0, mism = 0;
  std::vector<int16_t> htop, hleft, matrix;
};
// the clamped CELL penalties by name (vsx_ctx::pen)
struct Pen { int goql, gotl, goqi, goti, goqr, gotr, geql, getl, geqi, geti, geqr, getr; };
}  // namespace
static Pen pen_of(const vsx_ctx * c)
{
  const int * p = c->pen;
  return Pen {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11]};
}
static uint32_t pk(int v) { uint32_t x = (uint32_t) v & 0xffffu; return x | (x << 16); }

static void scoring_params(vsx_ctx * c, const vsx_scoring * s, CtxDraft & d)
{
  // search16_init, align_simd.cpp:1282-1376: scores must fit a CELL, each penalty SHRT_MAX/(1+CDEPTH)
  auto clamp = [&](int64_t v, int64_t lim) -> int {
    if (v > lim) { c->force_fallback = true; return (int) lim; }
    if (v < -lim) { c->force_fallback = true; return (int) -lim; }
    return (int) v;
  };
  const int match = d.match = clamp(s->match, 32767);
  const int mism = d.mism = clamp(s->mismatch, 32767);
  const int64_t raw[12] = {s->gap_open_query_left, s->gap_open_target_left, s->gap_open_query_interior,
                           s->gap_open_target_interior, s->gap_open_query_right, s->gap_open_target_right,
                           s->gap_ext_query_left, s->gap_ext_target_left, s->gap_ext_query_interior,
                           s->gap_ext_target_interior, s->gap_ext_query_right, s->gap_ext_target_right};
  for (int k = 0; k < 12; ++k) c->pen[k] = clamp(raw[k], 6553);
  const auto [goql, gotl, goqi, goti, goqr, gotr, geql, getl, geqi, geti, geqr, getr] = pen_of(c);

  VsxDevParams & P = c->P;
  P.match_pk = pk(match);
  P.qrq_i_pk = pk(goqi + geqi); P.rq_i_pk = pk(geqi);
  P.qrq_r_pk = pk(goqr + geqr); P.rq_r_pk = pk(geqr);
  P.qrt_i = goti + geti; P.rt_i = geti;
  P.qrt_r = gotr + getr; P.rt_r = getr;
  P.match = match; P.mismatch = mism;
  P.n_mismatch = s->n_mismatch ? 1 : 0;
  P.top_open = goql; P.top_step = geql;
  P.share_sub = (goqi + geqi == goti + geti && !std::getenv("VSX_NO_SHARE_SUB")) ? 1 : 0;
  int pmax = 0;
  for (int v : {goql + geql, goqi + geqi, goqr + geqr, gotl + getl, goti + geti, gotr + getr}) pmax = std::max(pmax, v);
  P.smin = -32768 + pmax;                                       // compute_score_min :1432-1444
}

static void border_tables_and_matrix(const vsx_ctx * c, CtxDraft & d)
{
  const auto [goql, gotl, goqi, goti, goqr, gotr, geql, getl, geqi, geti, geqr, getr] = pen_of(c);
  // border chains, evaluated with the reference's saturating steps
  d.htop.resize(VSX_TABLE_LEN); d.hleft.resize(VSX_TABLE_LEN); d.matrix.resize(256);
  {
    int h = -goql - geql;                                       // :1895-1910 (plain casts, in range by the 6553 limit)
    for (int j = 0; j < VSX_TABLE_LEN; ++j) { d.htop[j] = (int16_t) h; h = sat16(h - geql); }   // :2043-2051
    int m = gotl + getl;                                        // M_QR_target_left
    for (int i = 0; i < VSX_TABLE_LEN; ++i) { d.hleft[i] = (int16_t) sat16(0 - m); m = sat16(m + getl); }  // :844-859
  }
  auto amb = [](unsigned x) { return !(x == 1 || x == 2 || x == 4 || x == 8); };
  for (unsigned x = 0; x < 16; ++x)                              // :1319-1342
    for (unsigned y = 0; y < 16; ++y)
      {
        int v;
        if (c->P.n_mismatch && (x == 15 || y == 15)) v = d.mism;
        else if (amb(x) || amb(y)) v = 0;
        else v = (x == y) ? d.match : d.mism;
        d.matrix[x * 16 + y] = (int16_t) v;
      }
}

static int create_streams_and_tables(vsx_ctx * c, const CtxDraft & d)
{
  hipError_t e;
  // the aligner's streams get the HIGHEST priority the device offers: in a search its short plans share the GPU with the k-mer
  // counting kernel of the next window (lowest priority, vsx_kmer_host.cpp), whose millions of 15-us blocks would otherwise keep
  // every CU busy and hold each alignment stage back until the counting is over (r03 timeline: windows aligned 100 ms late)
  // Between them the TRACEBACK stream ranks above the DP streams where the device has a level to spare: the DP kernel of slice
  // i+2 waits for the traceback of slice i (two checkpoint blocks).  Same-box A/B of vsx_align_pairs (800 k pairs): 36.7-37.3 ms
  // against 37.5-39.0 with equal priorities.  It does not cure the starvation itself: a traceback wave needs 168 VGPRs, a retiring
  // DP wave frees 128, so while a DP launch still has workgroups to dispatch the traceback only gets whole-SIMD gaps (rocprofv3
  // traces of one call: profiles/r03/r03v_e2e_trace*.csv).
  int prio_low = 0, prio_high = 0;
  (void) hipDeviceGetStreamPriorityRange(&prio_low, &prio_high);            // numerically: high < low
  const int prio_dp = (prio_low - prio_high >= 2) ? prio_high + 1 : prio_high;
  // (r04 measured CU-masked streams -- a fixed share of the CUs for the traceback -- and rejected them: the DP kernel ran 2 x slower,
  //  profiles/r04/r04p_e2e_cumask_ab.txt; the VSX_TB_CUS switch is gone: masked streams also lose hipStreamNonBlocking and the priorities)
  if ((e = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio_dp)) != hipSuccess ||
      (e = hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, prio_high)) != hipSuccess ||
      (e = hipStreamCreateWithPriority(&c->stream_b, hipStreamNonBlocking, prio_dp)) != hipSuccess ||
      (e = hipStreamCreateWithPriority(&c->stream_up, hipStreamNonBlocking, prio_high)) != hipSuccess ||
      (e = hipStreamCreateWithPriority(&c->stream_dn, hipStreamNonBlocking, prio_high)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&c->ev_tb[0], hipEventDisableTiming)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&c->ev_tb[1], hipEventDisableTiming)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&c->ev_tb[2], hipEventDisableTiming)) != hipSuccess ||
      (e = c->d_htop.alloc(VSX_TABLE_LEN)) != hipSuccess || (e = c->d_hleft.alloc(VSX_TABLE_LEN)) != hipSuccess ||
      (e = c->d_matrix.alloc(256)) != hipSuccess ||
      (e = hipMemcpy(c->d_htop.p, d.htop.data(), VSX_TABLE_LEN * 2, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(c->d_hleft.p, d.hleft.data(), VSX_TABLE_LEN * 2, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(c->d_matrix.p, d.matrix.data(), 512, hipMemcpyHostToDevice)) != hipSuccess)
    return fail(VSX_EHIP, "vsx_create: %s", hipGetErrorString(e));
  c->P.htop = c->d_htop.p;
  c->P.hleft = c->d_hleft.p;
  c->P.matrix = c->d_matrix.p;
  c->P.tilt = 0;
  return VSX_OK;
}

// once per device, check on the hardware what the MAX3 class assumes (v_pk_maximum3_f16 == integer maximum on
// the patterns 0 .. 0x7BFF, denormals included); a device that fails keeps the 16-bit TILT class (tilt_possible())
static void max3_selftest_once(vsx_ctx * c)
{
  const int device = c->device;
  if (device < 64 && g_max3_state[device].load() == 0)
    {
      DevBuf<uint32_t> d_bad;
      uint32_t bad2[2] = {1, 1};
      if (d_bad.alloc(2) == hipSuccess && hipMemsetAsync(d_bad.p, 0, 8, c->stream) == hipSuccess &&
          vsx_launch_max3_selftest(d_bad.p, c->stream) == hipSuccess &&
          hipMemcpyAsync(bad2, d_bad.p, 8, hipMemcpyDeviceToHost, c->stream) == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess)
        {
          const uint32_t bad = bad2[0];
          if (bad) std::fprintf(stderr, "libvsx: device %d: v_pk_maximum3_f16 disagrees with the integer maximum on %u probes -- MAX3 class disabled\n", device, bad);
          g_max3_state[device].store(bad ? 2 : 1);
          // the second traceback kernel reads sign bits with v_perm_b32 selectors 8 .. 11: same one-off check, same kind of fallback
          if (bad2[1])
            {
              std::fprintf(stderr, "libvsx: device %d: v_perm_b32 sign selectors disagree on %u probes -- the first traceback kernel is used\n", device, bad2[1]);
              vsx_internal_set_tb_v2(device, 0);
            }
        }
      else
        {
          //  a self-test that could not RUN proves nothing: fail closed -- the 16-bit TILT class and the first traceback
          // kernel, which rest on no hardware assumption -- and say so
          (void) hipGetLastError();
          std::fprintf(stderr, "libvsx: device %d: the MAX3 / v_perm_b32 self-test could not run -- MAX3 class and second traceback kernel disabled\n", device);
          g_max3_state[device].store(2);
          vsx_internal_set_tb_v2(device, 0);
        }
    }
  else if (device >= 64) vsx_internal_set_tb_v2(device, 0);      // (no per-device state beyond 64 devices: the conservative kernels)
}

// Tilted coordinates X* = X + (i + j) g, g = the interior extension (VsxDevParams::tilt): available when both interior
// extensions are g > 0 and the interior QR coincide (the DP kernel's shared H - QR); per task the planner still has to
// prove the shifted range (tilt_possible()).  VSX_TILT=0 switches the class off (A/B measurements, tests).
// The tilted kernel adds the primed scores with a 32-bit add over both int16 halves: they must be non-negative
// (mismatch + 2g >= 0, the dummy rows' -ge(query left) + 2g >= 0).
static int tilted_params(vsx_ctx * c, const CtxDraft & d)
{
  const auto [goql, gotl, goqi, goti, goqr, gotr, geql, getl, geqi, geti, geqr, getr] = pen_of(c);
  const int match = d.match, mism = d.mism;
  const VsxDevParams & P = c->P;
  if (!(geqi == geti && geti > 0 && P.share_sub && !c->tb_packed && !c->force_fallback &&
        std::min(match, mism) + 2 * geti >= 0 && 2 * geti - geql >= 0 &&
        std::max(match, mism) + 2 * geti <= 255 && 2 * geti - geql <= 255 &&       // the LDS query profile of the class holds bytes
        // compressed checkpoints: H - F(next row) and H - E(next column) lie in [-g, max QR'] (plus the dummy rows' seed
        // go_ql + ge_ql + QR'): they must fit a signed byte
        geti <= 127 && std::max({goqi, goti, goqr + geqr - geti, gotr + getr - geti, goql + geql + goqi}) <= 127 &&
        !(std::getenv("VSX_TILT") && std::strcmp(std::getenv("VSX_TILT"), "0") == 0)))
    return VSX_OK;
  hipError_t e;
  const int g = geti;
  VsxDevParams & T = c->Pt;
  T = P;
  T.tilt = g;
  T.qrq_i_pk = pk(goqi + geqi - g); T.rq_i_pk = pk(geqi - g);
  T.qrq_r_pk = pk(goqr + geqr - g); T.rq_r_pk = pk(geqr - g);
  T.qrt_i = goti + geti - g; T.rt_i = geti - g;
  T.qrt_r = gotr + getr - g; T.rt_r = getr - g;
  std::vector<int16_t> htop_t(VSX_TABLE_LEN), hleft_t(VSX_TABLE_LEN), matrix_t(256);
  for (int j = 0; j < VSX_TABLE_LEN; ++j)              // entries beyond the range tilt_possible() admits are never read
    {
      htop_t[j] = (int16_t) sat16((int) d.htop[j] + (j - 1) * g);
      hleft_t[j] = (int16_t) sat16((int) d.hleft[j] + (j - 1) * g);
    }
  for (int x = 0; x < 256; ++x) matrix_t[x] = (int16_t) sat16(d.matrix[x] + 2 * g);
  if ((e = c->d_htop_t.alloc(VSX_TABLE_LEN)) != hipSuccess || (e = c->d_hleft_t.alloc(VSX_TABLE_LEN)) != hipSuccess ||
      (e = c->d_matrix_t.alloc(256)) != hipSuccess ||
      (e = hipMemcpy(c->d_htop_t.p, htop_t.data(), VSX_TABLE_LEN * 2, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(c->d_hleft_t.p, hleft_t.data(), VSX_TABLE_LEN * 2, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(c->d_matrix_t.p, matrix_t.data(), 512, hipMemcpyHostToDevice)) != hipSuccess)
    return fail(VSX_EHIP, "vsx_create: %s", hipGetErrorString(e));
  T.htop = c->d_htop_t.p; T.hleft = c->d_hleft_t.p; T.matrix = c->d_matrix_t.p;
  // EARLY (vsx_forward_kernel): the whole-wave single-strip MAX3 kernels end a task once the rest is a proven right-terminal gap.
  // The proof prices every move of an unseen path at M = the largest matrix entry (the ambiguous symbols' 0 included) per diagonal and
  // e = the smallest of the six extensions per gap column or row, charging no open: all twelve gap penalties must be >= 0.  The
  // kernel's 16-bit sums add at most (M + e + g) (R - 1) <= 31 (M + e + g), (M + e + g) rows of position 0 <= 32 (M + e + g) or
  // g + M + e to a value <= 0x7BFF: they stay inside a half when 32 (M + e + g) <= 0xFFFF - 0x7BFF.
  bool ok = true;
  for (int k = 0; k < 12; ++k) ok = ok && c->pen[k] >= 0;
  const int e_min = std::min({geql, getl, geqi, geti, geqr, getr});
  const int w0 = std::max({match, mism, 0}) + e_min;
  if (ok && 32 * (w0 + g) <= 0xFFFF - 0x7BFF)
    {
      T.es_on = 1; T.es_w0 = w0; T.es_e = e_min; T.es_rr = geqr;
      T.es_rate = std::max(1, w0 + geql);
    }
  return VSX_OK;
}

// a context vsx_create could not finish (the destructor gives back the events and the tables)
static void discard_ctx(vsx_ctx * c)
{
  for (hipStream_t st : {c->stream, c->stream2, c->stream_b, c->stream_up, c->stream_dn})
    if (st) (void) hipStreamDestroy(st);
  delete c;
}

int vsx_create(vsx_ctx ** out, const vsx_scoring * s, int device)
{
  if (!out || !s) return fail(VSX_EINVAL, "vsx_create: null argument");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    {
      (void) hipGetLastError();
      return fail(VSX_ENODEVICE, "vsx_create: no HIP device visible (libvsx has no CPU fallback)");
    }
  if (device < 0 || device >= ndev) return fail(VSX_EINVAL, "vsx_create: device %d out of range (0..%d)", device, ndev - 1);
  hipDeviceProp_t prop;
  VSX_HIP(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(VSX_ENODEVICE, "vsx_create: device %d is %s, libvsx is built for gfx950 only", device, prop.gcnArchName);
  VSX_HIP(hipSetDevice(device));

  auto * c = new vsx_ctx;
  c->device = device;
  c->sc = *s;
  if (const char * mode = std::getenv("VSX_TB_ARITH")) c->tb_packed = std::strcmp(mode, "packed") == 0;
  CtxDraft d;
  scoring_params(c, s, d);
  border_tables_and_matrix(c, d);
  int rc = create_streams_and_tables(c, d);
  if (rc == VSX_OK)
    {
      max3_selftest_once(c);
      rc = tilted_params(c, d);
    }
  if (rc != VSX_OK) { discard_ctx(c); return rc; }
  { std::lock_guard<std::mutex> lk(g_ctx_mu); g_ctxs.push_back(c); }
  *out = c;
  return VSX_OK;
}

void vsx_destroy(vsx_ctx * c)
{
  if (!c) return;
  { std::lock_guard<std::mutex> lk(g_ctx_mu); g_ctxs.erase(std::remove(g_ctxs.begin(), g_ctxs.end(), c), g_ctxs.end()); }
  (void) hipSetDevice(c->device);
  if (c->stream) { (void) hipStreamSynchronize(c->stream); (void) hipStreamDestroy(c->stream); }
  if (c->stream2) { (void) hipStreamSynchronize(c->stream2); (void) hipStreamDestroy(c->stream2); }
  if (c->stream_b) { (void) hipStreamSynchronize(c->stream_b); (void) hipStreamDestroy(c->stream_b); }
  if (c->stream_up) { (void) hipStreamSynchronize(c->stream_up); (void) hipStreamDestroy(c->stream_up); }
  if (c->stream_dn) { (void) hipStreamSynchronize(c->stream_dn); (void) hipStreamDestroy(c->stream_dn); }
  c->shared_dir[0].reset();
  c->shared_dir[1].reset();
  c->shared_dir[2].reset();
  c->shared_slab.reset();
  c->pool.retire();
  delete c;
}

}  // extern "C"
