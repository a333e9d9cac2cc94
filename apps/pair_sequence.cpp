// apps/pair_sequence.cpp -- the loop of the reference's scan-to-scan node (lidar_subscriber/src/ndt_omp_node.cpp) written
// against the C-ABI alone (no ROS, no PCL): every numbered cloud_N.pcd of a directory is read in order and voxel-filtered
// at 0.5 m into an ndt_cloud, then ALL consecutive pairs (k-1, k) are registered in one ndt_align_pairs_clouds call with
// the node's settings (resolution 1.0, step 0.1, epsilon 0.01, 64 iterations, DIRECT7) -- the registrations do not depend
// on each other once the clouds are known.  A pair that did not converge counts as identity (:120-123); the poses are
// chained with ndt_host_chain_pose.  Printed per pair: "Transform k-1 to k" and "TransformSum", then one timing line.
// --fitness: also the getFitnessScore of every pair at its final transformation, all from one ndt_pairs_fitness_scores
// call right after the pairs call ("fitness k-1 to k: <value>", 17 significant digits), and that call's time.
// --covariance: also the standard deviations of every pair's registered pose ("pair k sigma: sx sy sz sroll spitch syaw": the
// square roots of the diagonal of the sandwich covariance, "nan" where the pose is not determined), all pairs from one
// ndt_pairs_pose_covariances call right after the pairs call, and that call's time.  Not with --gicp.
// --batch-filter: every scan is read first, then all of them are prefiltered in ONE ndt_cloud_voxel_filter_batch call; the
// output is the plain run's, timing lines aside.
// --gicp: the same consecutive pairs through gicp_align_pairs_clouds (pclomp::GeneralizedIterativeClosestPoint with its
// constructor's settings, as apps/align.cpp runs it) in place of the NDT pairs call: every filtered scan indexed once, the
// k-NN covariances of all scans from one launch; poses chained as for NDT.  With --fitness the scores come from the same call.
// --gicp --lockstep: the same through gicp_align_pairs_lockstep (the registrations advanced together: one correspondence
// launch and one objective launch per step for all pairs in flight); it prints the lines --gicp prints.
// --map <out.pcd>: after the pose chain, all filtered scans at their chained poses (scan 0 at the identity) go into the map
// in ONE ndt_map_update_clouds call at the node's 0.5 m; "map: <n> points", and the map written as a binary PCD.
//
//   pair_sequence <pcd_directory> [--fitness] [--covariance] [--batch-filter] [--gicp [--lockstep]] [--map <out.pcd>]
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gicp_mi355.h"
#include "ndt_mi355.h"

#define CHECK(call)                                                     \
  do {                                                                  \
    if ((call) != NDT_OK) {                                             \
      std::fprintf(stderr, "%s failed: %s\n", #call, ndt_last_error()); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

static void print_matrix(const char* title, const float* T) {
  std::printf("%s\n", title);
  for (int r = 0; r < 4; r++) std::printf("  %.9g %.9g %.9g %.9g\n", T[r], T[4 + r], T[8 + r], T[12 + r]);
}

using clock_type = std::chrono::steady_clock;
static double since(clock_type::time_point a) { return std::chrono::duration<double, std::milli>(clock_type::now() - a).count(); }

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: pair_sequence <pcd_directory> [--fitness] [--covariance] [--batch-filter] [--gicp [--lockstep]] [--map <out.pcd>]\n");
    return 0;
  }
  bool want_fitness = false, want_covariance = false, batch_filter = false, use_gicp = false, lockstep = false;
  const char* map_path = nullptr;
  for (int a = 2; a < argc; a++) {
    if (std::strcmp(argv[a], "--fitness") == 0) want_fitness = true;
    if (std::strcmp(argv[a], "--covariance") == 0) want_covariance = true;
    if (std::strcmp(argv[a], "--batch-filter") == 0) batch_filter = true;
    if (std::strcmp(argv[a], "--gicp") == 0) use_gicp = true;
    if (std::strcmp(argv[a], "--lockstep") == 0) lockstep = true;
    if (std::strcmp(argv[a], "--map") == 0) {
      if (a + 1 >= argc) {
        std::fprintf(stderr, "--map needs a file name\nusage: pair_sequence <pcd_directory> [--fitness] [--covariance] [--batch-filter] [--gicp [--lockstep]] [--map <out.pcd>]\n");
        return 2;
      }
      map_path = argv[++a];
    }
  }
  if (want_covariance && use_gicp) {
    std::fprintf(stderr, "--covariance is the NDT pairs call's: not with --gicp\n");
    return 2;
  }
  const float kLeaf = 0.5f;
  ndt_handle h = nullptr;
  CHECK(ndt_create(0, &h));
  CHECK(ndt_set_resolution(h, 1.0f));
  CHECK(ndt_set_step_size(h, 0.1));
  CHECK(ndt_set_transformation_epsilon(h, 0.01));
  CHECK(ndt_set_maximum_iterations(h, 64));
  CHECK(ndt_set_neighborhood_search_method(h, NDT_DIRECT7));
  CHECK(ndt_warm_up(h, 65536));

  // ---- every cloud of the directory, filtered, resident in HBM
  ndt_pcd_sequence_handle seq = nullptr;
  CHECK(ndt_pcd_sequence_open(argv[1], &seq));
  size_t fresh = 0;
  CHECK(ndt_pcd_sequence_poll(seq, 0, &fresh));
  std::vector<ndt_cloud> clouds;
  const auto t_load = clock_type::now();
  if (batch_filter) {
    // every scan's records (16 bytes each) one after the other, then one prefilter call over all of them
    std::vector<float> raw_all;
    std::vector<size_t> offsets(1, 0);
    std::vector<int> dense_all, numbers;
    for (;;) {
      const void* raw = nullptr;
      size_t n = 0;
      int dense = 1, number = -1;
      if (ndt_pcd_sequence_next(seq, &raw, &n, &dense, &number) != NDT_OK) {  // unreadable file: skipped, as the node does
        std::fprintf(stderr, "skipped: %s\n", ndt_last_error());
        continue;
      }
      if (!raw) break;
      const float* p = static_cast<const float*>(raw);
      raw_all.insert(raw_all.end(), p, p + 4 * n);
      offsets.push_back(offsets.back() + n);
      dense_all.push_back(dense);
      numbers.push_back(number);
    }
    std::vector<ndt_cloud> filtered(numbers.size());
    CHECK(ndt_cloud_voxel_filter_batch(h, raw_all.data(), offsets.data(), numbers.size(), 16, dense_all.data(), kLeaf, 0, filtered.data(),
                                       nullptr));
    for (size_t k = 0; k < filtered.size(); k++) {
      size_t m = 0;
      CHECK(ndt_cloud_size(filtered[k], &m));
      if (m == 0) {  // empty clouds are not kept
        ndt_cloud_release(filtered[k]);
        continue;
      }
      std::printf("Loaded cloud_%d.pcd (%zu points)\n", numbers[k], m);
      clouds.push_back(filtered[k]);
    }
  }
  while (!batch_filter) {  // (the plain run: read and prefilter scan by scan)
    const void* raw = nullptr;
    size_t n = 0;
    int dense = 1, number = -1;
    if (ndt_pcd_sequence_next(seq, &raw, &n, &dense, &number) != NDT_OK) {  // unreadable file: skipped, as the node does
      std::fprintf(stderr, "skipped: %s\n", ndt_last_error());
      continue;
    }
    if (!raw) break;
    ndt_cloud c = nullptr;
    int overflowed = 0;
    CHECK(ndt_cloud_voxel_filter(h, raw, n, 16, dense, kLeaf, 0, &c, &overflowed));
    size_t m = 0;
    CHECK(ndt_cloud_size(c, &m));
    if (m == 0) {  // empty clouds are not kept
      ndt_cloud_release(c);
      continue;
    }
    std::printf("Loaded cloud_%d.pcd (%zu points)\n", number, m);
    clouds.push_back(c);
  }
  ndt_pcd_sequence_close(seq);
  const double load_ms = since(t_load);

  // ---- all consecutive pairs in one call
  const size_t n_pairs = clouds.size() > 1 ? clouds.size() - 1 : 0;
  std::vector<int> pairs(2 * n_pairs);
  for (size_t k = 0; k < n_pairs; k++) {
    pairs[2 * k] = static_cast<int>(k);
    pairs[2 * k + 1] = static_cast<int>(k + 1);
  }
  std::vector<float> T(16 * n_pairs);
  std::vector<int> conv(n_pairs), iters(n_pairs);
  std::vector<double> fitness(n_pairs);
  gicp_handle gh = nullptr;
  if (use_gicp) CHECK(gicp_create(0, &gh));
  const auto t_align = clock_type::now();
  if (use_gicp && lockstep)
    CHECK(gicp_align_pairs_lockstep(gh, clouds.data(), clouds.size(), pairs.data(), n_pairs, nullptr, DBL_MAX /* PCL's default */, T.data(),
                                    conv.data(), iters.data(), nullptr, want_fitness ? fitness.data() : nullptr));
  else if (use_gicp)
    CHECK(gicp_align_pairs_clouds(gh, clouds.data(), clouds.size(), pairs.data(), n_pairs, nullptr, DBL_MAX /* PCL's default */, T.data(),
                                  conv.data(), iters.data(), nullptr, want_fitness ? fitness.data() : nullptr));
  else
    CHECK(ndt_align_pairs_clouds(h, clouds.data(), clouds.size(), 1, pairs.data(), n_pairs, nullptr, T.data(), conv.data(), iters.data(), nullptr));
  const double align_ms = since(t_align);
  double fitness_ms = 0;
  if (want_fitness && n_pairs && !use_gicp) {
    const auto t_fit = clock_type::now();
    CHECK(ndt_pairs_fitness_scores(h, nullptr, DBL_MAX /* PCL's default */, fitness.data()));
    fitness_ms = since(t_fit);
  }
  double covariance_ms = 0;
  std::vector<double> cov(36 * n_pairs);
  if (want_covariance && n_pairs) {  // (at the final transformations the pairs call kept, converged or not)
    const auto t_cov = clock_type::now();
    CHECK(ndt_pairs_pose_covariances(h, nullptr, NDT_COV_SANDWICH, 1.0, cov.data(), nullptr));
    covariance_ms = since(t_cov);
  }

  // ---- pose chain
  static const float kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  std::vector<float> sum(kIdentity, kIdentity + 16);
  std::vector<float> poses(kIdentity, kIdentity + 16);  // scan k's pose in the frame of scan 0 (--map)
  size_t not_converged = 0;
  for (size_t k = 0; k < n_pairs; k++) {
    float* Tk = T.data() + 16 * k;
    if (!conv[k]) {
      not_converged++;
      for (int i = 0; i < 16; i++) Tk[i] = kIdentity[i];
    }
    ndt_host_chain_pose(sum.data(), Tk, sum.data());
    char title[96];
    std::snprintf(title, sizeof(title), "Transform %zu to %zu: (%d iterations%s)", k, k + 1, iters[k], conv[k] ? "" : ", not converged");
    print_matrix(title, Tk);
    print_matrix("TransformSum:", sum.data());
    poses.insert(poses.end(), sum.begin(), sum.end());
  }
  if (want_fitness)
    for (size_t k = 0; k < n_pairs; k++) std::printf("fitness %zu to %zu: %.17g\n", k, k + 1, fitness[k]);
  if (want_covariance)
    for (size_t k = 0; k < n_pairs; k++) {
      std::printf("pair %zu sigma:", k);
      for (int d = 0; d < 6; d++) std::printf(" %.9g", std::sqrt(cov[36 * k + 7 * d]));
      std::printf("\n");
    }
  std::printf("\nclouds %zu  pairs %zu (not converged %zu)\n", clouds.size(), n_pairs, not_converged);
  std::printf("time: read + prefilter %.2f ms, pairs call %.2f ms (%.1f pairs/s)\n", load_ms, align_ms,
              align_ms > 0 ? 1e3 * static_cast<double>(n_pairs) / align_ms : 0.0);
  if (want_fitness && !use_gicp) std::printf("time: fitness call %.3f ms\n", fitness_ms);
  if (want_covariance) std::printf("time: covariance call %.3f ms\n", covariance_ms);
  if (map_path) {  // ---- every scan at its pose into the map: one call
    const auto t_map = clock_type::now();
    std::vector<int> dense(clouds.size(), 1);
    int overflowed = 0;
    size_t n_map = 0;
    CHECK(ndt_map_update_clouds(h, clouds.data(), clouds.size(), dense.data(), poses.data(), kLeaf, &overflowed));
    CHECK(ndt_map_size(h, &n_map));
    const double map_ms = since(t_map);
    std::vector<float> map(4 * (n_map ? n_map : 1));
    CHECK(ndt_map_get(h, map.data(), 16));
    CHECK(ndt_pcd_write_xyz(map_path, map.data(), n_map, 16, 1));
    std::printf("map: %zu points\n", n_map);
    std::printf("time: map call %.3f ms%s\n", map_ms, overflowed ? " (leaf size too small: unfiltered)" : "");
  }
  for (ndt_cloud c : clouds) ndt_cloud_release(c);
  gicp_destroy(gh);
  ndt_destroy(h);
  return 0;
}
