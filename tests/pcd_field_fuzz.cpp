// tests/pcd_field_fuzz.cpp -- mutation fuzzer of the PCD field reader (ndt::pcd_read_field, ndt_pcd.cpp), built with
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_deskew_host.py: truncated, spliced and bit-flipped files must be
// parsed or rejected, never crash, and every call ends.   pcd_field_fuzz [iterations] [scratch dir]
#include "ndt_pcd.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
int main(int argc, char** argv) {
  std::mt19937 rng(11);
  // base files: binary with mixed types, ascii, compressed-literal -- each with a time field
  std::vector<std::string> bases;
  {
    std::string h = "# .PCD v0.7\nVERSION 0.7\nFIELDS x y z ring t\nSIZE 4 4 4 2 8\nTYPE F F F U F\nCOUNT 1 1 1 1 1\nWIDTH 50\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS 50\nDATA binary\n";
    std::string b(50 * 22, '\0');
    for (auto& c : b) c = static_cast<char>(rng());
    bases.push_back(h + b);
    std::string a = "VERSION 0.7\nFIELDS x y z t\nSIZE 4 4 4 4\nTYPE F F F I\nCOUNT 1 1 1 1\nWIDTH 5\nHEIGHT 1\nPOINTS 5\nDATA ascii\n1 2 3 10\n4 5 6 -20\nnan 1 2 30\n7 8 9 40\n1e3 -2 0.5 50\n";
    bases.push_back(a);
    std::string ch = "VERSION 0.7\nFIELDS x y z t\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\nWIDTH 8\nHEIGHT 1\nPOINTS 8\nDATA binary_compressed\n";
    std::string raw(128, 'a');
    std::string comp;
    for (size_t i = 0; i < raw.size(); i += 32) { comp.push_back(31); comp.append(raw, i, 32); }
    unsigned sz[2] = {static_cast<unsigned>(comp.size()), 128};
    bases.push_back(ch + std::string(reinterpret_cast<char*>(sz), 8) + comp);
  }
  const std::string path_s = std::string(argc > 2 ? argv[2] : "/tmp") + "/field_fuzz_case.pcd";
  const char* path = path_s.c_str();
  const char* names[] = {"t", "x", "ring", "absent"};
  int ok = 0, bad = 0;
  const int iters = argc > 1 ? std::atoi(argv[1]) : 4000;
  for (int it = 0; it < iters; it++) {
    std::string f = bases[it % bases.size()];
    const int nm = rng() % 5;  // (now and then the file as it is)
    for (int k = 0; k < nm; k++) {
      const int op = rng() % 4;
      if (f.empty()) break;
      const size_t pos = rng() % f.size();
      if (op == 0) f[pos] = static_cast<char>(rng());
      else if (op == 1) f.erase(pos, 1 + rng() % 40);
      else if (op == 2) f.insert(pos, std::string(1 + rng() % 8, static_cast<char>('0' + rng() % 10)));
      else f.resize(pos);
    }
    FILE* fp = std::fopen(path, "wb");
    if (!fp) return 2;
    std::fwrite(f.data(), 1, f.size(), fp);
    std::fclose(fp);
    size_t n = 0; int nf = 0, kind = 0; std::string err;
    if (ndt::pcd_read_header(path, &n, &nf, &kind, err) != 0) { bad++; continue; }
    if (n > 1000000) { bad++; continue; }  // the caller sizes the buffer from the header
    std::vector<double> out(n ? n : 1);
    size_t got = 0;
    if (ndt::pcd_read_field(path, names[(it / 3) % 4], out.data(), n, &got, err) == 0) ok++; else bad++;
    if (n > 1 && ndt::pcd_read_field(path, "t", out.data(), n - 1, &got, err) == 0) return 3;  // (a buffer one too small is never filled)
  }
  std::printf("fuzz: %d parsed, %d rejected, no crash\n", ok, bad);
  return 0;
}
