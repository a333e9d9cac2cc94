// tests/acc_blob_fuzz.cpp -- mutation fuzzer of the accumulated target's blob parser and checksum (ndt_acc_blob.cpp), built
// with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_target_persist_host.py: truncated, spliced and bit-flipped
// blobs, half of them with the checksum mended so that the checks behind it are reached, must be accepted or refused, never
// crash or read outside the buffer (every case lives in a heap block of exactly its size).   acc_blob_fuzz [iterations]
#include "ndt_acc_blob.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

int main(int argc, char** argv) {
  std::mt19937 rng(11);
  // base blobs of 0, 1 and 9 rows with random payloads
  std::vector<std::vector<unsigned char>> bases;
  for (int rows : {0, 1, 9}) {
    std::vector<unsigned char> b(ndtc::kAccBlobHeaderBytes + rows * ndtc::kAccBlobRowBytes);
    for (size_t k = ndtc::kAccBlobHeaderBytes; k < b.size(); k++) b[k] = static_cast<unsigned char>(rng());
    const int lo[3] = {-3, 0, 1 - (1 << 20)}, hi[3] = {5, 0, (1 << 20) - 1};
    ndtc::acc_blob_write_header(b.data(), 0.5f, static_cast<uint64_t>(rows), lo, hi, b.data() + ndtc::kAccBlobHeaderBytes);
    ndtc::AccBlobHeader hd;
    if (ndtc::acc_blob_parse(b.data(), b.size(), &hd) != nullptr || hd.n_voxels != static_cast<uint64_t>(rows)) {
      std::printf("a blob written by acc_blob_write_header does not parse\n");
      return 1;
    }
    bases.push_back(b);
  }
  int ok = 0, bad = 0;
  const int iters = argc > 1 ? std::atoi(argv[1]) : 5000;
  for (int it = 0; it < iters; it++) {
    std::vector<unsigned char> f = bases[it % bases.size()];
    const int nm = 1 + rng() % 4;
    for (int k = 0; k < nm && !f.empty(); k++) {
      const int op = rng() % 5;
      const size_t pos = (rng() % 3 == 0) ? rng() % f.size() : rng() % (f.size() < 64 ? f.size() : 64);  // mostly the header
      if (op == 0) f[pos] = static_cast<unsigned char>(rng());
      else if (op == 1) f[pos] ^= static_cast<unsigned char>(1u << (rng() % 8));
      else if (op == 2) f.erase(f.begin() + pos, f.begin() + pos + (rng() % (f.size() - pos)) % 120);
      else if (op == 3) f.insert(f.begin() + pos, 1 + rng() % 120, static_cast<unsigned char>(rng()));
      else f.resize(pos);
    }
    if (it % 2 && f.size() >= ndtc::kAccBlobHeaderBytes) {  // mend the checksum over whole words of what is there
      const size_t payload = (f.size() - ndtc::kAccBlobHeaderBytes) / 8 * 8;
      const uint64_t sum = ndtc::acc_blob_checksum(f.data(), f.data() + ndtc::kAccBlobHeaderBytes, payload);
      std::memcpy(f.data() + 56, &sum, 8);
    }
    std::vector<unsigned char> exact(f);  // capacity == size: one byte past the end is out of bounds
    exact.shrink_to_fit();
    ndtc::AccBlobHeader hd;
    const char* why = ndtc::acc_blob_parse(exact.empty() ? nullptr : exact.data(), exact.size(), &hd);
    if (why == nullptr) {
      if (exact.size() != ndtc::kAccBlobHeaderBytes + hd.n_voxels * ndtc::kAccBlobRowBytes) {
        std::printf("accepted a blob whose size disagrees with its header\n");
        return 1;
      }
      ok++;
    } else {
      bad++;
    }
    (void)ndtc::acc_blob_hash(ndtc::kAccBlobHashSeed, exact.data(), exact.size() / 8 * 8);
  }
  std::printf("fuzz: %d accepted, %d refused, no crash\n", ok, bad);
  return 0;
}
