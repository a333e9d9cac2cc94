// ndt_acc_blob.cpp -- header parser and checksum of an exported accumulated target (layout: include/ndt_mi355.h).
// Little-endian on disk and in memory: the fields are read and written with memcpy on a little-endian host.
#include "ndt_acc_blob.hpp"

#include <cmath>
#include <cstring>

namespace ndtc {
namespace {

const char kMagic[8] = {'N', 'D', 'T', 'A', 'C', 'C', '1', '\0'};

template <class T>
T get(const unsigned char* p, size_t off) {
  T v;
  std::memcpy(&v, p + off, sizeof(v));
  return v;
}
template <class T>
void put(unsigned char* p, size_t off, T v) {
  std::memcpy(p + off, &v, sizeof(v));
}

}  // namespace

uint64_t acc_blob_hash(uint64_t h, const void* data, size_t bytes) {
  const unsigned char* p = static_cast<const unsigned char*>(data);
  for (size_t o = 0; o + 8 <= bytes; o += 8) {
    uint64_t w;
    std::memcpy(&w, p + o, 8);
    h = (h ^ w) * 0x100000001b3ull;
  }
  return h;
}

uint64_t acc_blob_checksum(const void* header, const void* payload, size_t payload_bytes) {
  return acc_blob_hash(acc_blob_hash(kAccBlobHashSeed, header, 56), payload, payload_bytes);
}

void acc_blob_write_header(void* out, float resolution, uint64_t n_voxels, const int lo[3], const int hi[3], const void* payload) {
  unsigned char* p = static_cast<unsigned char*>(out);
  std::memset(p, 0, kAccBlobHeaderBytes);
  std::memcpy(p, kMagic, 8);
  put<uint32_t>(p, 8, 1u);
  put<uint32_t>(p, 12, static_cast<uint32_t>(kAccBlobRowBytes));
  put<float>(p, 16, resolution);
  put<uint64_t>(p, 24, n_voxels);
  for (int k = 0; k < 3; k++) {
    put<int32_t>(p, 32 + 4 * k, n_voxels ? lo[k] : 0);
    put<int32_t>(p, 44 + 4 * k, n_voxels ? hi[k] : 0);
  }
  put<uint64_t>(p, 56, acc_blob_checksum(p, payload, static_cast<size_t>(n_voxels) * kAccBlobRowBytes));
}

const char* acc_blob_parse(const void* blob, size_t bytes, AccBlobHeader* out) {
  if (!blob) return "null blob";
  if (bytes < kAccBlobHeaderBytes) return "the blob is shorter than its 64-byte header";
  const unsigned char* p = static_cast<const unsigned char*>(blob);
  if (std::memcmp(p, kMagic, 8) != 0) return "the blob does not start with the magic \"NDTACC1\"";
  if (get<uint32_t>(p, 8) != 1u) return "unknown blob version (this library reads version 1)";
  if (get<uint32_t>(p, 12) != kAccBlobRowBytes) return "the blob's row_bytes is not 104";
  AccBlobHeader hd;
  hd.resolution = get<float>(p, 16);
  hd.n_voxels = get<uint64_t>(p, 24);
  for (int k = 0; k < 3; k++) {
    hd.lo[k] = get<int32_t>(p, 32 + 4 * k);
    hd.hi[k] = get<int32_t>(p, 44 + 4 * k);
  }
  hd.checksum = get<uint64_t>(p, 56);
  const size_t payload = bytes - kAccBlobHeaderBytes;
  if (payload % kAccBlobRowBytes != 0 || hd.n_voxels != payload / kAccBlobRowBytes)
    return "the blob's size is not 64 + 104 * n_voxels bytes";
  if (acc_blob_checksum(p, p + kAccBlobHeaderBytes, payload) != hd.checksum) return "the blob's checksum does not match its contents";
  if (!std::isfinite(hd.resolution) || !(hd.resolution > 0.0f)) return "the blob's resolution is not finite and positive";
  for (int k = 0; k < 3; k++) {
    if (hd.lo[k] > hd.hi[k]) return "the blob's cell box has lo > hi on an axis";
    if (hd.lo[k] < -kAccBlobCellLimit || hd.hi[k] >= kAccBlobCellLimit) return "the blob's cell box lies outside [-2^20, 2^20)";
  }
  if (out) *out = hd;
  return nullptr;
}

}  // namespace ndtc
