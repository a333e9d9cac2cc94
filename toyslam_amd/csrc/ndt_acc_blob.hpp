// ndt_acc_blob.hpp -- the exported form of an accumulated target (include/ndt_mi355.h, "the blob"): header parser and
// checksum.  Host only, no HIP header: a CPU harness builds ndt_acc_blob.cpp alone.
#pragma once
#include <cstddef>
#include <cstdint>

namespace ndtc {

constexpr size_t kAccBlobHeaderBytes = 64, kAccBlobRowBytes = 104;
constexpr uint64_t kAccBlobHashSeed = 0xcbf29ce484222325ull;
constexpr long long kAccBlobCellLimit = 1ll << 20;  // cells of [-2^20, 2^20) on every axis

struct AccBlobHeader {
  float resolution = 0;
  uint64_t n_voxels = 0;
  int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  uint64_t checksum = 0;
};

// h continued over the 8-byte little-endian words of data: per word h = (h ^ w) * 0x100000001b3 mod 2^64.  bytes % 8 == 0
uint64_t acc_blob_hash(uint64_t h, const void* data, size_t bytes);
// the checksum of a blob: over bytes [0, 56) of the header followed by the payload
uint64_t acc_blob_checksum(const void* header, const void* payload, size_t payload_bytes);
// header of n_voxels rows in [lo, hi] at `out` (64 bytes), the checksum over it and the payload included
void acc_blob_write_header(void* out, float resolution, uint64_t n_voxels, const int lo[3], const int hi[3], const void* payload);
// nullptr = a well-formed blob (its header in *out); else what is wrong with it.  Looks at the header and the checksum,
// not into the rows
const char* acc_blob_parse(const void* blob, size_t bytes, AccBlobHeader* out);

}  // namespace ndtc
