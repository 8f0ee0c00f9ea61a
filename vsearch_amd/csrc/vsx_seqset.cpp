// vsx_seqset.cpp -- host side of libvsx, sequence sets: encoding, both strands, the case bitmap of the k-mer index, and the purity
// pass the planner asks for (ensure_impure).  See vsx_context.cpp for the layout of the host layer.
#include "vsx_host_internal.h"

#include <cinttypes>

using vsxp::fail;
using namespace vsxh;

extern "C" {

static int seqset_common(vsx_ctx * ctx, vsx_seqset ** out, uint64_t n, const void * blob, bool blob_on_device,
                         uint64_t blob_bytes, const uint64_t * offsets, const uint32_t * lengths, bool both_strands = false,
                         int case_bits = 0 /* 1: soft masking, 2: DUST */)
{
  if (!ctx || !out || (n && (!offsets || !lengths)) || (blob_bytes && !blob))
    return fail(VSX_EINVAL, "vsx_seqset_create: null argument");
  *out = nullptr;
  for (uint64_t i = 0; i < n; ++i)
    if (offsets[i] > blob_bytes || lengths[i] > blob_bytes - offsets[i])
      return fail(VSX_EINVAL, "vsx_seqset_create: sequence %" PRIu64 " exceeds the blob", i);
  VSX_HIP(hipSetDevice(ctx->device));
  auto * s = new vsx_seqset;
  s->ctx = ctx;
  s->device = ctx->device;
  s->n = n;
  s->bytes = blob_bytes;
  s->off.assign(offsets, offsets + n);
  s->len.assign(lengths, lengths + n);
  uint64_t code_bytes = blob_bytes;
  if (both_strands)
    {
      // the minus strands follow the plus strands' codes, packed in sequence order
      s->n = 2 * n;
      s->off.resize(2 * n);
      s->len.resize(2 * n);
      for (uint64_t k = 0; k < n; ++k) { s->off[n + k] = code_bytes; s->len[n + k] = lengths[k]; code_bytes += lengths[k]; }
      s->bytes = code_bytes;
    }
  hipError_t e = hipSuccess;
  ScratchPool * pl = (code_bytes <= VSX_SEQSET_POOLED_BYTES) ? &ctx->pool : nullptr;
  if (pl) s->pool_ref = ctx->pool_owner;
  PoolBuf<uint8_t> staging;
  const uint8_t * d_ascii = static_cast<const uint8_t *>(blob);
  do {
    if ((e = s->d_codes.alloc(pl, code_bytes + 2 * VSX_CODE_SLACK)) != hipSuccess) break;
    if ((e = s->d_off.alloc(pl, s->n)) != hipSuccess) break;
    if ((e = s->d_len.alloc(pl, s->n)) != hipSuccess) break;
    if (n)
      {
        if ((e = hipMemcpyAsync(s->d_off.p, s->off.data(), s->n * 8, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess) break;
        if ((e = hipMemcpyAsync(s->d_len.p, s->len.data(), s->n * 4, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess) break;
      }
    if (!blob_on_device && blob_bytes)
      {
        if ((e = staging.alloc(pl, blob_bytes + 16)) != hipSuccess) break;
        if ((e = hipMemcpyAsync(staging.p, blob, blob_bytes, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess) break;
        d_ascii = staging.p;
      }
    if ((e = vsx_launch_encode(d_ascii, s->codes(), blob_bytes, ctx->stream)) != hipSuccess) break;
    if (case_bits)
      {
        const uint64_t nb = (blob_bytes + 7) / 8 + 16;             // the sweep reads a dword at any byte of the map
        if ((e = s->d_lower.alloc(pl, nb)) != hipSuccess) break;
        if ((e = hipMemsetAsync(s->d_lower.p, 0, nb, ctx->stream)) != hipSuccess) break;
        if ((e = vsx_kmer_launch_case_bits(d_ascii, blob_bytes, s->d_lower.p, case_bits == 2, ctx->stream)) != hipSuccess) break;
        if (case_bits == 2 && (e = vsx_launch_dust(s->codes(), s->d_off.p, s->d_len.p, n, s->d_lower.p, ctx->stream)) != hipSuccess) break;
        s->lower_bytes = (blob_bytes + 7) / 8;
      }
    if (both_strands && (e = vsx_launch_revcomp(s->codes(), s->d_off.p, s->d_off.p + n, s->d_len.p, n, ctx->stream)) != hipSuccess) break;
    e = hipStreamSynchronize(ctx->stream);
  } while (false);
  if (e != hipSuccess)
    {
      delete s;
      return fail(e == hipErrorOutOfMemory ? VSX_ENOMEM : VSX_EHIP, "vsx_seqset_create: %s", hipGetErrorString(e));
    }
  *out = s;
  return VSX_OK;
}

int vsx_seqset_create(vsx_ctx * ctx, vsx_seqset ** out, uint64_t n, const char * blob, uint64_t blob_bytes,
                      const uint64_t * offsets, const uint32_t * lengths)
{
  return seqset_common(ctx, out, n, blob, false, blob_bytes, offsets, lengths);
}

int vsx_seqset_create_both_strands(vsx_ctx * ctx, vsx_seqset ** out, uint64_t n, const char * blob, uint64_t blob_bytes,
                                   const uint64_t * offsets, const uint32_t * lengths)
{
  return seqset_common(ctx, out, n, blob, false, blob_bytes, offsets, lengths, true);
}

// internal (vsx_search.cpp, soft_mask): the set also keeps the case bitmap its k-mer index honours
// (mode 1: the bitmap is the input's case; mode 2: the input is upper-cased and DUST-masked on the device, vsx_mask.hip)
int vsx_internal_seqset_create_cased(vsx_ctx * ctx, vsx_seqset ** out, uint64_t n, const char * blob, uint64_t blob_bytes,
                                     const uint64_t * offsets, const uint32_t * lengths, int mode)
{
  if (mode != 1 && mode != 2) return fail(VSX_EINVAL, "vsx_internal_seqset_create_cased: mode must be 1 (soft) or 2 (dust)");
  return seqset_common(ctx, out, n, blob, false, blob_bytes, offsets, lengths, false, mode);
}
const uint8_t * vsx_internal_seqset_lower(const vsx_seqset * s) { return s ? s->d_lower.p : nullptr; }
// the bitmap on the host: bit i of byte i / 8 = blob byte i is masked
int vsx_internal_seqset_lower_download(const vsx_seqset * s, uint8_t * dst, uint64_t nbytes)
{
  if (!s || !s->d_lower.p || nbytes > s->lower_bytes) return fail(VSX_EINVAL, "vsx_internal_seqset_lower_download: no case bitmap of that size");
  VSX_HIP(hipSetDevice(s->device));
  if (nbytes) VSX_HIP(hipMemcpy(dst, s->d_lower.p, nbytes, hipMemcpyDeviceToHost));
  return VSX_OK;
}

// test hook (tests/test_gpu_mask.py): the case bitmap a mode-1 / mode-2 set ends up with, (blob_bytes + 7) / 8 bytes
int vsx_internal_mask_bits(vsx_ctx * ctx, uint64_t n, const char * blob, uint64_t blob_bytes, const uint64_t * offsets,
                           const uint32_t * lengths, int mode, uint8_t * bits_out)
{
  vsx_seqset * s = nullptr;
  int rc = vsx_internal_seqset_create_cased(ctx, &s, n, blob, blob_bytes, offsets, lengths, mode);
  if (rc != VSX_OK) return rc;
  rc = vsx_internal_seqset_lower_download(s, bits_out, (blob_bytes + 7) / 8);
  vsx_seqset_destroy(s);
  return rc;
}

// test observable (tests/test_gpu_marshal.py): how often this context ran a plan again for its run buffer (out[0]) and a text
// kernel again for its text buffer (out[1]) since it was created
int vsx_internal_settle_counts(const vsx_ctx * ctx, uint64_t out[2])
{
  if (!ctx || !out) return fail(VSX_EINVAL, "vsx_internal_settle_counts: null argument");
  out[0] = ctx->settle_counts[0].load();
  out[1] = ctx->settle_counts[1].load();
  return VSX_OK;
}

int vsx_seqset_create_from_device(vsx_ctx * ctx, vsx_seqset ** out, uint64_t n, const void * d_blob,
                                  uint64_t blob_bytes, const uint64_t * offsets, const uint32_t * lengths)
{
  return seqset_common(ctx, out, n, d_blob, true, blob_bytes, offsets, lengths);
}

void vsx_seqset_destroy(vsx_seqset * s)
{
  if (!s) return;
  (void) hipSetDevice(s->device);       // the owning context may already be gone
  delete s;
}

uint64_t vsx_seqset_count(const vsx_seqset * s) { return s ? s->n : 0; }

}  // extern "C"

// per-sequence "contains a non-ACGT symbol" of a set, computed once (vsx_purity_kernel)
int vsxh::ensure_impure(const vsx_seqset * s)
{
  std::lock_guard<std::mutex> lk(s->impure_mu);
  if (s->have_impure) return VSX_OK;
  vsx_ctx * ctx = s->ctx;
  VSX_HIP(hipSetDevice(ctx->device));
  // (r06, ADVICE r05: the flags come from the scratch pool -- hipMalloc / hipFree synchronise the WHOLE device, and a search's plans are
  //  made while the counting kernel of the next window runs: 15-42 ms per window, profiles/r06/r06a_search_timeline.txt)
  PoolBuf<uint8_t> d_flags;
  VSX_HIP(d_flags.alloc(s->pool_ref ? s->pool_ref.get() : nullptr, s->n));
  VSX_HIP(vsx_launch_purity(s->codes(), s->d_off.p, s->d_len.p, s->n, d_flags.p, ctx->stream));
  s->impure.assign(s->n, 0);
  if (s->n) VSX_HIP(hipMemcpyAsync(s->impure.data(), d_flags.p, s->n, hipMemcpyDeviceToHost, ctx->stream));
  VSX_HIP(hipStreamSynchronize(ctx->stream));
  s->have_impure = true;
  return VSX_OK;
}
