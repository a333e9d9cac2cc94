// ndt_prims.hpp -- the device-wide primitives this library takes from hipCUB (rocPRIM underneath): a stable LSD radix sort of
// (key, value) pairs over the key bits [0, end_bit) and an exclusive prefix sum.  ndt_prims.hip is the ONE unit that includes
// hipCUB: its sort and scan kernels are instantiated once, and replacing them is a one-file job.
// Every call is queued on `stream` and allocates nothing: the caller hands over `temp`, at least *_temp_bytes(n) bytes (what
// hipCUB asks for, plus 256), which one sort or scan after another may share in stream order.
#pragma once
#include <hip/hip_runtime.h>

namespace ndt {

size_t sort_pairs_temp_bytes(int n, size_t key_bytes);  // key_bytes: 4 (unsigned) or 8 (unsigned long long)
size_t exclusive_sum_temp_bytes(int n);
hipError_t sort_pairs(const unsigned* keys_in, unsigned* keys_out, const int* vals_in, int* vals_out, int n, int end_bit, void* temp,
                      size_t temp_bytes, hipStream_t stream);
hipError_t sort_pairs(const unsigned long long* keys_in, unsigned long long* keys_out, const int* vals_in, int* vals_out, int n, int end_bit,
                      void* temp, size_t temp_bytes, hipStream_t stream);
// out[i] = in[0] + ... + in[i - 1]; in == out is allowed
hipError_t exclusive_sum(const unsigned* in, unsigned* out, int n, void* temp, size_t temp_bytes, hipStream_t stream);

}  // namespace ndt
