// vsx_otutab_internal.h -- shared between the OTU-table kernels (vsx_otutab.hip) and their host side (vsx_otutab.cpp).
// An ITEM is a label the device works on: query k is item k; of the targets only those that take part in an add are items, named by
// the host's ascending list of their numbers.
#ifndef VSX_OTUTAB_INTERNAL_H
#define VSX_OTUTAB_INTERNAL_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>

#define VSX_OTUTAB_NO 0xFFFFFFFFu            // no target, no taxonomy, no sample (the low half of a key that is no cell)

// what a scan launch reads and writes
struct VsxOtutabScan {
  uint32_t         n;            // items
  const uint32_t * list;         // n label numbers, ascending; NULL: item i is label i
  const uint8_t *  blob;
  const uint64_t * off;          // per label
  const uint32_t * len;          // per label
  uint64_t         hash_mask;
  uint64_t *       name_off;     // per item: where the name begins in the blob
  uint32_t *       name_len;     // per item
  uint64_t *       hash;         // per item, cut to hash_mask
  uint64_t *       tax_off;      // targets, per LABEL: the value of tax=
  uint32_t *       tax_len;      // targets, per LABEL: VSX_OTUTAB_NO without tax=
};

// what the key and gather launches read: element e < nq is query e, element nq + u the u-th target of the unmatched pass
struct VsxOtutabAdds {
  uint32_t         nq, nu;
  uint32_t         n_otus;
  const uint32_t * q_target;     // nq
  const uint64_t * q_ab;         // nq or NULL (1 each)
  const uint32_t * q_sample;     // nq: sample ranks
  const uint32_t * unmatched;    // nu target numbers, ascending
  const uint32_t * t_otu;        // per target: OTU rank (written for the targets that take part)
  const uint32_t * t_tax_len;    // per target (written for the targets that take part)
};

#ifdef __cplusplus
extern "C" {
#endif
// one wavefront per item: name span, name hash; for targets (tax_len given) the taxonomy span too
hipError_t vsx_launch_otutab_scan(VsxOtutabScan P, int targets, hipStream_t st);
// d_idx[i] = i
hipError_t vsx_launch_otutab_iota(uint32_t n, uint32_t * d_idx, hipStream_t st);
// stable radix sort of (key, value) on the key's bits [0, end_bit); temp NULL: the temporary bytes only
hipError_t vsx_launch_otutab_sort(void * temp, size_t * temp_bytes, const uint64_t * d_keys_in, uint64_t * d_keys_out, const uint32_t * d_vals_in,
                                  uint32_t * d_vals_out, uint32_t n, uint32_t end_bit, hipStream_t st);
// one wavefront per sorted position: d_flag[i] = 0 iff item d_idx[i] has the hash, the length and the bytes of item d_idx[i - 1]
hipError_t vsx_launch_otutab_heads(uint32_t n, const uint64_t * d_sorted_hash, const uint32_t * d_idx, const uint8_t * d_blob,
                                   const uint64_t * d_name_off, const uint32_t * d_name_len, uint32_t * d_flag, hipStream_t st);
// inclusive sum of the flags; temp NULL: the temporary bytes only
hipError_t vsx_launch_otutab_flagsum(void * temp, size_t * temp_bytes, const uint32_t * d_flag, uint32_t * d_incl, uint32_t n, hipStream_t st);
// group g = d_incl[i] - 1: d_group[item] for every item, and per group its first item with that item's name span
hipError_t vsx_launch_otutab_groups(uint32_t n, const uint32_t * d_flag, const uint32_t * d_incl, const uint32_t * d_idx, const uint64_t * d_name_off,
                                    const uint32_t * d_name_len, uint32_t * d_group, uint32_t * d_rep_item, uint64_t * d_rep_off,
                                    uint32_t * d_rep_len, hipStream_t st);
// d_item_rank[item] = d_rank[d_group[item]]; with a list also d_label_rank[list[item]] (the other labels keep what a memset left)
hipError_t vsx_launch_otutab_assign(uint32_t n, const uint32_t * d_group, const uint32_t * d_rank, const uint32_t * d_list, uint32_t * d_item_rank,
                                    uint32_t * d_label_rank, hipStream_t st);
// key[e] = OTU rank << 32 | sample rank; the low half is VSX_OTUTAB_NO for what is no cell (abundance 0, unmatched pass) and the key
// n_otus << 32 | VSX_OTUTAB_NO for a query without a hit; value[e] = e
hipError_t vsx_launch_otutab_keys(VsxOtutabAdds A, uint64_t * d_keys, uint32_t * d_vals, hipStream_t st);
// in sorted order: the abundance, the key's OTU half, and e + 1 where the add's target carries tax= (else 0)
hipError_t vsx_launch_otutab_gather(VsxOtutabAdds A, const uint64_t * d_sorted_keys, const uint32_t * d_sorted_vals, uint64_t * d_count,
                                    uint32_t * d_otu, uint32_t * d_taxseq, hipStream_t st);
// sums per key; temp NULL: the temporary bytes only
hipError_t vsx_launch_otutab_reduce_cells(void * temp, size_t * temp_bytes, const uint64_t * d_keys, const uint64_t * d_count, uint32_t n,
                                          uint64_t * d_unique, uint64_t * d_sum, uint32_t * d_n_unique, hipStream_t st);
// maxima per OTU; temp NULL: the temporary bytes only
hipError_t vsx_launch_otutab_reduce_tax(void * temp, size_t * temp_bytes, const uint32_t * d_otu, const uint32_t * d_taxseq, uint32_t n,
                                        uint32_t * d_unique, uint32_t * d_max, uint32_t * d_n_unique, hipStream_t st);
#ifdef __cplusplus
}
#endif

#endif
