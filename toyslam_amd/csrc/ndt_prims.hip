// ndt_prims.hip -- the one unit that includes hipCUB (ndt_prims.hpp has the contract)
#include "ndt_prims.hpp"

#include <hipcub/hipcub.hpp>

namespace ndt {

namespace {
template <class Key>
size_t sort_query(int n) {
  size_t tb = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, tb, static_cast<const Key*>(nullptr), static_cast<Key*>(nullptr),
                                           static_cast<const int*>(nullptr), static_cast<int*>(nullptr), n, 0, static_cast<int>(sizeof(Key) * 8));
  return tb;
}
}  // namespace

size_t sort_pairs_temp_bytes(int n, size_t key_bytes) {
  return (key_bytes == sizeof(unsigned long long) ? sort_query<unsigned long long>(n) : sort_query<unsigned>(n)) + 256;
}
size_t exclusive_sum_temp_bytes(int n) {
  size_t tb = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tb, static_cast<const unsigned*>(nullptr), static_cast<unsigned*>(nullptr), n);
  return tb + 256;
}
hipError_t sort_pairs(const unsigned* keys_in, unsigned* keys_out, const int* vals_in, int* vals_out, int n, int end_bit, void* temp,
                      size_t temp_bytes, hipStream_t stream) {
  return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, n, 0, end_bit, stream);
}
hipError_t sort_pairs(const unsigned long long* keys_in, unsigned long long* keys_out, const int* vals_in, int* vals_out, int n, int end_bit,
                      void* temp, size_t temp_bytes, hipStream_t stream) {
  return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, n, 0, end_bit, stream);
}
hipError_t exclusive_sum(const unsigned* in, unsigned* out, int n, void* temp, size_t temp_bytes, hipStream_t stream) {
  return hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, in, out, n, stream);
}

}  // namespace ndt
