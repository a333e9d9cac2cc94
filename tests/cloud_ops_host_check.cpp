// tests/cloud_ops_host_check.cpp -- the host pieces the cloud operations share (toyslam_amd/csrc/ndt_cloud_ops.hip, declared in
// ndt_internal.hpp) on the CPU, built with -fsanitize=address,undefined by tests/test_cloud_ops_cases.py: the range plan, the
// fold of box rows, the member table's host side, the list preamble's output nulling and the environment cap.  No device call
// is made: a table of fewer than two entries is never copied up.
#include <cassert>
#include <cstdio>

#include "ndt_internal.hpp"
#include "ndt_select.hpp"

namespace ndtc {  // what ndt_handle.hip defines for the library
thread_local std::string g_last_error;
thread_local hipStream_t tls_pool_stream = nullptr;
}  // namespace ndtc

int main() {
  // range_plan: the blocks tile [0, n), per is `least` until the cap binds
  for (size_t n : {size_t(0), size_t(1), size_t(255), size_t(256), size_t(257), size_t(4096), size_t(4097), size_t(262144), size_t(262145),
                   size_t(2147483647)})
    for (int cap : {1, 7, 64, 1024}) {
      int blocks = -1, per = -1;
      ndt::range_plan(n, 256, cap, &blocks, &per);
      assert(per >= 256 && blocks <= cap);
      assert(static_cast<size_t>(blocks) * per >= n && (blocks == 0 ? n == 0 : (static_cast<size_t>(blocks) - 1) * per < n));
      int b2 = 0, p2 = 0;
      if (cap == 1024) {
        ndt::select_plan(n, &b2, &p2);
        assert(b2 == blocks && p2 == per);
      }
    }
  // fold_box_rows: blocks [1, 3) of rows with a stride of 16 floats, into a cloud's empty boxes
  {
    std::vector<float> rows(4 * 16, 1e30f);
    for (int b = 0; b < 4; b++)
      for (int v = 0; v < 2; v++)
        for (int a = 0; a < 3; a++) {
          rows[b * 16 + v * 6 + a] = static_cast<float>(-b - a);
          rows[b * 16 + v * 6 + 3 + a] = static_cast<float>(b + a);
        }
    DeviceCloud c;
    fold_box_rows(&c, rows.data(), 16, 1, 2, NDT_BOX_ROUTE_DESKEW);
    for (int v = 0; v < 2; v++)
      for (int a = 0; a < 3; a++) assert(c.bb_min[v][a] == static_cast<float>(-2 - a) && c.bb_max[v][a] == static_cast<float>(2 + a));
    assert(c.box_route == NDT_BOX_ROUTE_DESKEW);
    fold_box_rows(&c, rows.data(), 16, 0, 0, NDT_BOX_ROUTE_SELECT);  // no block: the boxes stay, the route is set
    assert(c.bb_min[0][0] == -2.0f && c.box_route == NDT_BOX_ROUTE_SELECT);
  }
  // MemberTable: one entry is handed over as it is, nothing is copied up
  {
    struct M { int first, n; };
    MemberTable<M> t;
    t.host.push_back(M{0, 5});
    assert(t.n() == 1 && t.bytes() == sizeof(M) && t.one().n == 5 && t.table() == nullptr);
    assert(t.upload(nullptr) == NDT_OK && t.table() == nullptr);
  }
  // clouds_begin: both output arrays nulled, 65536 clouds refused before anything is written
  {
    ndt_cloud a[3], b[3];
    for (int k = 0; k < 3; k++) a[k] = b[k] = reinterpret_cast<ndt_cloud>(&a);
    assert(clouds_begin(65536, a, b) == NDT_ERR_INVALID && a[0] != nullptr && g_last_error == "at most 65535 clouds per call");
    assert(clouds_begin(3, a, b) == NDT_OK);
    for (int k = 0; k < 3; k++) assert(a[k] == nullptr && b[k] == nullptr);
    assert(clouds_begin(3, nullptr, nullptr) == NDT_OK);
  }
  // spec_checks and env_block_cap
  {
    ndt_select_spec s{};
    assert(spec_checks(&s, ndt::select_spec_error) == NDT_OK);
    s.flags = NDT_SELECT_BOX_NEGATE;
    assert(spec_checks(&s, ndt::select_spec_error) == NDT_ERR_INVALID && g_last_error == "BOX_NEGATE without BOX");
    assert(spec_checks(static_cast<const ndt_select_spec*>(nullptr), ndt::select_spec_error, "null motion") == NDT_ERR_INVALID &&
           g_last_error == "null motion");
    setenv("NDT_CLOUD_OPS_CHECK_CAP", "7", 1);
    assert(env_block_cap("NDT_CLOUD_OPS_CHECK_CAP", 1024) == 7 && env_block_cap("NDT_CLOUD_OPS_CHECK_CAP", 4) == 4);
    setenv("NDT_CLOUD_OPS_CHECK_CAP", "-3", 1);
    assert(env_block_cap("NDT_CLOUD_OPS_CHECK_CAP", 1024) == 1024 && env_block_cap("NDT_CLOUD_OPS_CHECK_UNSET", 9) == 9);
  }
  std::puts("cloud_ops_host_check: ok");
  return 0;
}
