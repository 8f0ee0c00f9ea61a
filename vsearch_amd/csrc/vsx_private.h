// vsx_private.h -- the private interface of libvsx's host layer: every function one file of this directory defines and another
// calls (and that neither include/*.h, vsx_internal.h nor vsx_kmer.h declares), and the host helpers the files share.  Host-only
// C++; the file that defines a function includes this header too, so a declaration that drifts from its definition does not compile.
#ifndef VSX_PRIVATE_H
#define VSX_PRIVATE_H

#include "../../include/vsx_search.h"
#include "vsx_symbols.h"

#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

extern "C" {

// ---- vsx_context.cpp, vsx_seqset.cpp -----------------------------------------------------------------------------------------
// one thread-local error slot for the whole library (vsx_last_error)
void vsx_internal_set_error(const char * msg);
const vsx_scoring * vsx_internal_scoring(const vsx_ctx * ctx);
int vsx_internal_device(const vsx_ctx * ctx);
hipStream_t vsx_internal_stream(const vsx_ctx * ctx);
// a block of the context's scratch pool (reused from call to call, poisoned under VSX_POISON) and its way back; `got` is the block's
// real size, which put() wants again
hipError_t vsx_internal_scratch_get(vsx_ctx * ctx, size_t bytes, void ** out, size_t * got);
void vsx_internal_scratch_put(vsx_ctx * ctx, void * p, size_t got);
// vsx_symbols.h as the host compiles it (tests/test_symbols_host.py): four 256-entry tables by byte value -- map4, ambiguous4 (of the
// byte taken as a code), complement, upcase -- and the return value mix64(word)
uint64_t vsx_internal_symbols(uint8_t * code, uint8_t * ambiguous, uint8_t * complement, uint8_t * upcase, uint64_t word);
// CPUs this process may really use: affinity mask, capped by a cgroup v2 CPU quota
int vsx_internal_usable_cpus(void);
// the library's host worker pool: fn(0) runs on the caller, which also helps with queued jobs while it waits
void vsx_internal_run_threads(int nth, void (*fn)(int, void *), void * arg);
// VSX_POISON=1 (debugging aid, tests/test_gpu_poison.py): every device block this library hands out (scratch pool, DevBuf::alloc) is
// filled with 0xA5 first, so a read of memory nobody has written gives the same junk in every run instead of whatever an earlier
// plan, index or process left there.  VSX_POISON_BYTE (0 .. 255, decimal or 0x..) chooses another byte; anything else is refused
// with a line on stderr and the default stays.  The blocks the plans of a context SHARE (checkpoints, traceback slab) and a plan's
// strip buffer are handed out untouched when they are large enough, so vsx_plan_run fills the part each chunk is about to use,
// stream-ordered, before that chunk's first kernel.  A grow-only DevBuf is not filled again on reuse (some are built once and kept).
// Unset: nothing is filled and nothing is issued.  The environment is read once per process.
int vsx_internal_poison_byte(void);      // -1: off, else the byte
void vsx_internal_poison(void * p, size_t bytes);
// device memory under pressure: every live context of the device drops the stream-ordered blocks no plan holds and frees its idle
// pool.  Whoever meets hipErrorOutOfMemory calls this once and retries (vsxp::device_malloc does).  Returns the bytes released.
uint64_t vsx_internal_memory_pressure(int device);
// The big stream-ordered scratch blocks of a context (three checkpoint blocks, the traceback slab): their sizes, and a reservation
// of at least those sizes.  A search runs its windows on several contexts of one device; a context that meets its first full
// window in the middle of a warm search would pay the multi-GB hipMalloc there, so the searcher levels the contexts after a call.
void vsx_internal_scratch_sizes(vsx_ctx * ctx, uint64_t out[4]);
int vsx_internal_scratch_reserve(vsx_ctx * ctx, const uint64_t want[4]);
// what the plans of a context asked for since the last reset: {checkpoint block, slab} bytes
void vsx_internal_scratch_requests(vsx_ctx * ctx, uint64_t out[2], int reset);
// what the checkpoint block of ONE plan of `ntasks` whole-wave tasks (a query of qlen rows against up to eight targets of tlen
// columns) will ask for; ctx == NULL: as under a scoring that can be tilted (the compressed layout, a lower bound)
uint64_t vsx_internal_ckpt_bytes_estimate(const vsx_ctx * ctx, uint64_t ntasks, uint32_t qlen, uint32_t tlen);
void vsx_internal_seqset_device(const vsx_seqset * s, const uint8_t ** codes, const uint64_t ** off, const uint32_t ** len, uint64_t * n);
// host copies of the set's lengths (the k-mer index build of long words lays its key slots out by their running sum)
const uint32_t * vsx_internal_seqset_host_lengths(const vsx_seqset * s);
// soft_mask: the set also keeps the case bitmap its k-mer index honours
// (mode 1: the bitmap is the input's case; mode 2: the input is upper-cased and DUST-masked on the device, vsx_mask.hip)
int vsx_internal_seqset_create_cased(vsx_ctx * ctx, vsx_seqset ** out, uint64_t n, const char * blob, uint64_t blob_bytes,
                                     const uint64_t * offsets, const uint32_t * lengths, int mode);
// the set's case bitmap (soft masking) or NULL: an index over a set that has one leaves out every word over a lower-case symbol
const uint8_t * vsx_internal_seqset_lower(const vsx_seqset * s);
// the bitmap on the host: bit i of byte i / 8 = blob byte i is masked
int vsx_internal_seqset_lower_download(const vsx_seqset * s, uint8_t * dst, uint64_t nbytes);

// ---- vsx_search.cpp ----------------------------------------------------------------------------------------------------------
// what vsx_chimera.cpp reads of a searcher: its context, options (weak_id clamped), unclamped scoring, database set and masked text
vsx_ctx * vsx_internal_searcher_ctx(const vsx_searcher * S);
const vsx_search_opts * vsx_internal_searcher_opts(const vsx_searcher * S);
const vsx_scoring * vsx_internal_searcher_scoring(const vsx_searcher * S);
const vsx_seqset * vsx_internal_searcher_dbset(const vsx_searcher * S);
void vsx_internal_searcher_text(const vsx_searcher * S, const char ** blob, const uint64_t ** off, const uint32_t ** len);
// chimera detection's part search: the parts searched as given with candidate heaps of `tophits` entries; the searcher's own heap
// size is restored before returning
int vsx_internal_search_parts(vsx_searcher * S, int64_t tophits, uint64_t nq, const char * qblob, uint64_t qbytes,
                              const uint64_t * qoff, const uint32_t * qlen, vsx_hits * out);

}  // extern "C"

bool vsx_internal_searcher_has_abundances(const vsx_searcher * S);

// ---- vsx_denovo_search.cpp ---------------------------------------------------------------------------------------------------
// the de novo part search of vsx_uchime_denovo (vsx_chimera.cpp drives it; what needs the searcher's internals lives there)
struct VsxDenovo;
int vsx_internal_denovo_create(vsx_searcher * S, VsxDenovo ** out);
void vsx_internal_denovo_destroy(VsxDenovo * D);
int vsx_internal_denovo_window(VsxDenovo * D, uint64_t s0, uint64_t wn, const std::vector<uint64_t> & poff, const std::vector<uint32_t> & plen,
                               const std::vector<uint32_t> & pmember, double * t_rank, double * t_members);
void vsx_internal_denovo_merge(VsxDenovo * D, uint64_t p, const uint8_t * present, std::vector<uint32_t> & targets);
int vsx_internal_denovo_search(VsxDenovo * D, const std::vector<uint32_t> & parts, std::vector<std::vector<uint32_t>> & accepted,
                               uint64_t * pairs, uint64_t * sentinels);
void vsx_internal_denovo_commit(VsxDenovo * D, const std::vector<uint32_t> & seqnos);

// ---- vsx_chimera.cpp ---------------------------------------------------------------------------------------------------------
// what vsx_chimalns.cpp needs of the detection: (qidx[p] in qset, tidx[p] in the searcher's database) pairs through the detection's
// own align_pairs, with device buffers that live as long as the handle.  The view: the hit records on the host, the exported run
// words on the device (stored last column first) and their number.
struct VsxRealigned;
struct VsxPairOut;
int vsx_internal_chimera_realign(vsx_searcher * S, const vsx_seqset * qset, const std::vector<uint32_t> & qidx, const std::vector<uint32_t> & tidx,
                                 const char * who, VsxRealigned ** out);
void vsx_internal_chimera_realigned_view(const VsxRealigned * R, const VsxPairOut ** hits, const uint32_t ** d_runs, uint64_t * nruns);
void vsx_internal_chimera_realigned_free(VsxRealigned * R);

// ---- vsx_exact.cpp -----------------------------------------------------------------------------------------------------------
// the exact-match index of a searcher (device table + code words, host map), built by the first vsx_search_exact
struct VsxExactIndex;
void vsx_internal_exact_index_destroy(VsxExactIndex * X);

// ---- vsx_sintax.cpp ----------------------------------------------------------------------------------------------------------
// what a searcher keeps for vsx_sintax: the per-rank name ids of its labels (dropped when the labels change) and window buffers
struct VsxSintaxIndex;
void vsx_internal_sintax_index_destroy(VsxSintaxIndex * X);

// ---- vsx_orient.cpp ----------------------------------------------------------------------------------------------------------
// what a searcher keeps for vsx_orient: the match-count table of its database (device and host) and window buffers
struct VsxOrientIndex;
void vsx_internal_orient_index_destroy(VsxOrientIndex * X);

// ---- vsx_hitout.cpp ----------------------------------------------------------------------------------------------------------
// what a searcher keeps for vsx_hits_render: its database text on the device and the window buffers
struct VsxHitoutIndex;
void vsx_internal_hitout_index_destroy(VsxHitoutIndex * X);

// ---- vsx_msa.hip -------------------------------------------------------------------------------------------------------------
// rows of one tile of the device MSA's profile kernel: a cluster of n members takes ceil(n / this) row tiles per 64 columns (tests)
extern "C" uint32_t vsx_internal_msa_row_tile(void);

// ---- vsx_mask.cpp ------------------------------------------------------------------------------------------------------------
// DUST of one sequence, for the dispatch layer's per-query masking (the caller owns the scratch copy; hard: --hardmask)
void vsx_internal_dust_one(char * seq, int64_t len, std::vector<char> & scratch, bool hard = false);
// one sequence of vsx_fastx_mask on the host (vsx_fastx_mask.cpp: the host routes and what the device is compared to); qmask 0 none /
// 1 soft / 2 dust.  text and bits may be null; the bits are OR-ed atomically from bit0 on; *windows counts the DUST windows visited
uint32_t vsx_internal_fastx_mask_one(const char * in, int64_t len, int qmask, int hard, char * text, uint8_t * bits, uint64_t bit0,
                                     std::vector<char> & work, std::vector<char> & scratch, uint64_t * windows);

// ---- host helpers ------------------------------------------------------------------------------------------------------------
#ifndef VSX_DEVICE_RESERVE_BYTES
#define VSX_DEVICE_RESERVE_BYTES ((size_t) 6 << 30)      // what stays free for the runtime itself (kernel scratch of every queue, code objects)
#endif

// (hidden: the helpers add nothing to the library's dynamic symbols)
namespace vsxp __attribute__((visibility("hidden"))) {

// set the thread-local error text, return the code
__attribute__((format(printf, 2, 3))) inline int fail(int code, const char * fmt, ...)
{
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  const int n = vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (n < (int) sizeof buf) { vsx_internal_set_error(buf); return code; }
  std::string big((size_t) n + 1, '\0');
  va_start(ap, fmt);
  vsnprintf(&big[0], big.size(), fmt, ap);
  va_end(ap);
  vsx_internal_set_error(big.c_str());
  return code;
}

inline int hip_fail(const char * who, const char * call, hipError_t e, const char * file, int line)
{
  return fail(e == hipErrorOutOfMemory ? VSX_ENOMEM : VSX_EHIP, "%s%s%s failed: %s (%s:%d)", who ? who : "", who ? ": " : "", call,
              hipGetErrorString(e), file, line);
}

// return from the calling function when a HIP call fails: VSX_ENOMEM for hipErrorOutOfMemory, VSX_EHIP otherwise.
// VSX_HIP_AS puts the name of the API function the caller serves in front of the text.
#define VSX_HIP_AS(who, call) \
  do { const hipError_t e_ = (call); if (e_ != hipSuccess) return vsxp::hip_fail(who, #call, e_, __FILE__, __LINE__); } while (0)
#define VSX_HIP(call) VSX_HIP_AS(nullptr, call)

// hipMalloc that never fills the device to the brim and asks the contexts of the device for their idle blocks before it gives up.
// A device filled to the brim fails LATER and worse than a refused hipMalloc: the runtime cannot allocate a queue's kernel scratch
// and aborts the process (HSA_STATUS_ERROR_OUT_OF_RESOURCES, profiles/r05/r05b_config5_share_abort.txt).  Keep a reserve.
inline hipError_t device_malloc(void ** out, size_t bytes)
{
  if (bytes >= ((size_t) 16 << 20))
    {
      size_t free_b = 0, total_b = 0;
      int dev = 0;
      if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b < bytes + VSX_DEVICE_RESERVE_BYTES && hipGetDevice(&dev) == hipSuccess)
        (void) vsx_internal_memory_pressure(dev);
      (void) hipGetLastError();
    }
  hipError_t e = hipMalloc(out, bytes);
  if (e == hipErrorOutOfMemory)
    {
      // the aligner contexts of this device may sit on idle checkpoint blocks of an earlier, much larger plan: ask for them
      int dev = 0;
      (void) hipGetLastError();
      if (hipGetDevice(&dev) == hipSuccess && vsx_internal_memory_pressure(dev) > 0) e = hipMalloc(out, bytes);
    }
  return e;
}

// owning device buffer of `n` elements (a request for none still allocates one); every fresh block is poisoned
template <typename T>
struct DevBuf {
  T * p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf & operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  void release() { if (p) { (void) hipFree(p); p = nullptr; n = 0; } }
  hipError_t alloc(size_t count)
  {
    release();
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    const hipError_t e = device_malloc(reinterpret_cast<void **>(&p), bytes);
    if (e == hipSuccess) { n = count; vsx_internal_poison(p, bytes); } else p = nullptr;
    return e;
  }
  // grow-only: the block is replaced (old one freed first) only when it is too small
  hipError_t ensure(size_t count) { return (p && count <= n) ? hipSuccess : alloc(count); }
};

// its pinned host counterpart
template <typename T>
struct PinnedBuf {
  T * p = nullptr;
  size_t n = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf &) = delete;
  PinnedBuf & operator=(const PinnedBuf &) = delete;
  ~PinnedBuf() { release(); }
  void release() { if (p) { (void) hipHostFree(p); p = nullptr; n = 0; } }
  hipError_t alloc(size_t count)
  {
    release();
    const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p), std::max<size_t>(count, 1) * sizeof(T), hipHostMallocDefault);
    if (e == hipSuccess) n = count; else p = nullptr;
    return e;
  }
};

// grow-only, with a quarter of headroom: a staging buffer that is filled again window after window
template <typename T>
hipError_t ensure_pinned(PinnedBuf<T> & b, size_t count) { return (b.p && count <= b.n) ? hipSuccess : b.alloc(count + count / 4); }

// a fresh DevBuf of `count` elements filled from the host, and a device array into a host vector; both on `st`, neither waits
template <typename T>
hipError_t upload(DevBuf<T> & d, const T * h, size_t count, hipStream_t st)
{
  const hipError_t e = d.alloc(count);
  if (e != hipSuccess || count == 0) return e;
  return hipMemcpyAsync(d.p, h, count * sizeof(T), hipMemcpyHostToDevice, st);
}

template <typename T>
hipError_t download(std::vector<T> & h, const T * d, size_t count, hipStream_t st)
{
  h.resize(count);
  return count ? hipMemcpyAsync(h.data(), d, count * sizeof(T), hipMemcpyDeviceToHost, st) : hipSuccess;
}

// a fresh DevBuf of `count` zeroes (null stream)
template <typename T>
int zeroed(const char * who, DevBuf<T> & b, size_t count)
{
  VSX_HIP_AS(who, b.alloc(count));
  VSX_HIP_AS(who, hipMemset(b.p, 0, std::max<size_t>(count, 1) * sizeof(T)));
  return VSX_OK;
}

// a lease on a block of the context's scratch pool (vsx_internal_scratch_get): it goes back when the lease ends or is renewed
template <typename T>
struct Scratch {
  vsx_ctx * ctx = nullptr;
  T * p = nullptr;
  size_t got = 0;
  Scratch() = default;
  Scratch(const Scratch &) = delete;
  Scratch & operator=(const Scratch &) = delete;
  ~Scratch() { if (p) vsx_internal_scratch_put(ctx, p, got); }
  hipError_t alloc(vsx_ctx * c, size_t count)
  {
    if (p) { vsx_internal_scratch_put(ctx, p, got); p = nullptr; }
    ctx = c;
    void * q = nullptr;
    const hipError_t e = vsx_internal_scratch_get(c, std::max<size_t>(count, 1) * sizeof(T), &q, &got);
    if (e == hipSuccess) p = static_cast<T *>(q);
    return e;
  }
  hipError_t upload(vsx_ctx * c, const T * h, size_t count, hipStream_t st)
  {
    const hipError_t e = alloc(c, count);
    if (e != hipSuccess || count == 0) return e;
    return hipMemcpyAsync(p, h, count * sizeof(T), hipMemcpyHostToDevice, st);
  }
};

// the arrays of a result the caller frees with free(): n elements (one for none), null when the host is out of memory.
// array_of zeroes them; host_array leaves them as malloc gives them, for results of which every element is written
// (tests/test_gpu_poison.py would show one that is not: keep each caller on the kind it has).
template <typename T>
T * array_of(uint64_t n) { return static_cast<T *>(std::calloc(std::max<uint64_t>(n, 1), sizeof(T))); }
template <typename T>
T * host_array(uint64_t n) { return static_cast<T *>(std::malloc(std::max<uint64_t>(n, 1) * sizeof(T))); }

inline uint64_t align64(uint64_t v) { return (v + 63) & ~(uint64_t) 63; }

// a decimal number from the environment; `otherwise` when the variable is unset.  An empty value counts as unset -- except under
// empty_is_zero, for the variables that were always read with a bare strtoull (which makes 0 of it).
inline uint64_t env_u64(const char * name, uint64_t otherwise, bool empty_is_zero = false)
{
  const char * e = std::getenv(name);
  return (e && (*e || empty_is_zero)) ? std::strtoull(e, nullptr, 10) : otherwise;
}

// VSX_<COMMAND>=host: the call takes the command's host route
inline bool env_is_host(const char * name)
{
  const char * env = std::getenv(name);
  return env && std::strcmp(env, "host") == 0;
}

// Does a call that needs `need` bytes of device memory fit beside the reserve?  Sets the context's device and reads its free
// memory (hipMemGetInfo answers for the current device, so the two belong together).  pretend_env, where not null, names the
// testing aid that replaces `need`.  The answer goes to *fits; the return value is VSX_OK unless either call fails.
inline int device_fits(const vsx_ctx * ctx, const char * who, uint64_t need, const char * pretend_env, bool * fits)
{
  size_t free_b = 0, total_b = 0;
  if (hipSetDevice(vsx_internal_device(ctx)) != hipSuccess || hipMemGetInfo(&free_b, &total_b) != hipSuccess)
    return fail(VSX_EHIP, "%s: the device does not answer", who);
  if (pretend_env) need = env_u64(pretend_env, need, true);
  *fits = need + VSX_DEVICE_RESERVE_BYTES <= free_b;
  return VSX_OK;
}

// the error probability of a Phred quality value, as the reference tabulates it (the device never evaluates it: tables are host-built)
inline double phred_error_probability(int value) { return std::pow(10.0, -value / 10.0); }

// the reference's fatal error for a quality value outside [qmin, qmax]; kind 1: below qmin, 2: above qmax
inline int quality_failure(const char * who, int kind, int value, long long qmin, long long qmax)
{
  if (kind == 1) return fail(VSX_EINVAL, "%s: FASTQ quality value (%d) below qmin (%lld)", who, value, qmin);
  return fail(VSX_EINVAL, "%s: FASTQ quality value (%d) above qmax (%lld)", who, value, qmax);
}

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// adds the host time of its scope to a field of a command's stats
struct Stopwatch {
  double & seconds;
  const double t0 = now_s();
  explicit Stopwatch(double & field) : seconds(field) {}
  ~Stopwatch() { seconds += now_s() - t0; }
};

inline int usable_cpus() { return vsx_internal_usable_cpus(); }

// f(0) on the caller, f(1) ... f(nth - 1) on the library's persistent worker pool (every parallel pass of a search window or a
// clustering round used to create and join its own std::threads -- a dozen passes of 16 threads per round, ~3 ms of a 45 ms round)
template <typename F>
void run_pool(int nth, F && f)
{
  if (nth <= 1) { f(0); return; }
  using Fn = typename std::remove_reference<F>::type;
  vsx_internal_run_threads(nth, [](int t, void * a) { (*static_cast<Fn *>(a))(t); }, (void *) &f);
}

// chrmap_4bit (the codes the device encoder writes into a sequence set) and chrmap_ambiguous_4bit, as vsx_symbols.h states them
inline uint8_t map4(unsigned char c) { return (uint8_t) vsxsym::map4(c); }
using vsxsym::ambiguous4;

// do the n spans (offsets[k], lengths[k]) lie inside a blob of blob_bytes?  (offset + length may wrap: never added.)  `what` names
// a span in the error text: "query", "a sequence", ...
inline int check_spans(const char * who, const char * what, uint64_t n, const uint64_t * offsets, const uint32_t * lengths, uint64_t blob_bytes)
{
  for (uint64_t k = 0; k < n; ++k)
    if (offsets[k] > blob_bytes || lengths[k] > blob_bytes - offsets[k]) return fail(VSX_EINVAL, "%s: %s exceeds the blob", who, what);
  return VSX_OK;
}

}  // namespace vsxp

#endif
