// nb_tree_prims.h — the two device-wide primitives of the Barnes-Hut build (nb_tree.hip.h), compiled in a translation unit of
// their own (nb_tree_prims.hip) so that rocPRIM's headers never meet the library's other kernels.
// Both follow rocPRIM's convention: tmp == nullptr only returns the temporary storage needed in `bytes`.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// stable radix sort of (64-bit key, 32-bit value) pairs, ascending
hipError_t nb_tree_sort_pairs(void *tmp, size_t &bytes, const uint64_t *keys_in, uint64_t *keys_out, const uint32_t *vals_in,
                              uint32_t *vals_out, size_t n, hipStream_t stream);
// exclusive prefix sum of 32-bit counts, accumulated and stored in 64 bits
hipError_t nb_tree_scan(void *tmp, size_t &bytes, const uint32_t *in, uint64_t *out, size_t n, hipStream_t stream);
