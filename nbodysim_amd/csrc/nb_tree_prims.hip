// nb_tree_prims.hip — rocPRIM's device radix sort and scan behind two plain functions (nb_tree_prims.h).
#include "nb_tree_prims.h"

#include <cstring>
#include <rocprim/rocprim.hpp>

hipError_t nb_tree_sort_pairs(void *tmp, size_t &bytes, const uint64_t *keys_in, uint64_t *keys_out, const uint32_t *vals_in,
                              uint32_t *vals_out, size_t n, hipStream_t stream)
{
    return rocprim::radix_sort_pairs(tmp, bytes, keys_in, keys_out, vals_in, vals_out, n, 0, 64, stream);
}

hipError_t nb_tree_scan(void *tmp, size_t &bytes, const uint32_t *in, uint64_t *out, size_t n, hipStream_t stream)
{
    return rocprim::exclusive_scan(tmp, bytes, in, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), stream);
}
