// apps/map_sequence.cpp -- the processing loop of the reference's mapping node
// (lidar_subscriber/src/ndt_omp_mapping_node.cpp) written against the C-ABI alone (no ROS, no PCL): read the
// numbered cloud_N.pcd scans of a directory in order (process_new_clouds :110-136), voxel-filter each
// (load_and_filter_cloud :138-149), register every scan against its predecessor with the node's NDT settings
// (initialize_ndt :55-62, align_consecutive_clouds :151-169), chain the pose (process_available_clouds :70-100) and
// accumulate the global map (update_global_map :195-211).  What the node publishes as ROS messages is printed.
//
// With a fourth argument "rosbag" the loop is the other mapping node's (lidar_subscriber/src/ndt_rosbag_mapping_node.cpp:46-75,
// with the scans of the directory standing in for the bag's messages): leaf 0.3 (:87), every registration starts from
// the previous one's result (pres_transform, :63,127), its fitness score is printed (:130), a registration that did not
// converge counts as identity (:137-140), and pose, trajectory and global map are updated after every scan (:64-68).
//
// The node does everything for a scan one step after the other, and so does this program by default (files are read and
// parsed ahead in the background).  With a fifth argument "pipeline" the steps of CONSECUTIVE scans overlap (the results are
// the same, bit for bit -- every step runs the same kernels on the same data):
//   prep thread      voxel filter of scan k+1, its upload as the next source, its voxel grid as the target after that, on a
//                    prep handle of its own (NDT_PIPELINE_PARTITION=1: on the side partition of the CUs, ndt_set_cu_partition)
//   this thread      registration of scan k (inputs taken over with ndt_share_input_target / ndt_share_input_source: no
//                    copy, no rebuild), pose chain, printing
//   map thread       global map update of scan k-1 (the map is not an input of any registration)
// Measured at the nodes' size (40 scans of 60 k raw points, tools/time_map_sequence.py, round 3): 1.9 ms per scan one step
// after the other, 2.7 ms overlapped, 3.7 ms overlapped on CU partitions -- the steps are short host-paced sequences of
// pageable copies and small launches, and two threads driving them get in each other's way; hence not the default.
//
//   map_sequence [--scan-to-map [--window <metres>] [--map-fitness] [--nvtl] [--covariance] [--deskew <field>] [--range <min> <max>] [--outliers-radius <r> <min_neighbors>] [--outliers-stat <mean_k> <stddev_mul>] [--ground <threshold> <hypotheses> <eps_deg> [--ground-remove]] [--clusters <tolerance> <min_size> [<max_size>]] [--flat <k> <curvature_max>] [--reject-unexplained <L>] [--clear-rays <min_rays> <margin>] [--save-target <file>] [--load-target <file> [--localize]]] <pcd_directory> [voxel_leaf_size (0.5 | 0.3)] [global_map_out.pcd | -] [rosbag | node] [serial | pipeline] [host]
// ("host": the serial loop with every cloud passing through host buffers, as in rounds 1-3; the default keeps them in HBM)
//
// --scan-to-map (anywhere on the line; the node's loop with clouds resident in HBM): every scan after the first is registered
// against the ACCUMULATED target -- all scans so far, each merged into the voxel grid at its registered pose
// (ndt_target_accumulate_cloud) -- instead of against its predecessor alone.  The registration starts from the previous scan's
// pose (the rosbag node's guess rule) and its result IS the scan's pose in the map: nothing is chained, so the trajectory
// does not add up the errors of the pairs.  The printed lines keep their form.
// --window <metres> (with --scan-to-map): after a scan has been accumulated at its pose the target is cropped to the
// axis-aligned cube of that half-side around the pose's translation (ndt_target_accumulate_crop): the map the registrations see
// stays bounded on a trajectory of any length.  The largest voxel count the target reached is printed at the end.
// --save-target <file> (with --scan-to-map): after the run the whole accumulated target is saved (ndt_target_accumulate_save).
// --load-target <file> (with --scan-to-map): the file is imported before the first scan (ndt_target_accumulate_load), and the
// first scan is then registered against it from the identity guess -- like every later scan from the previous pose --
// instead of being placed at the identity.  --localize (with --load-target): scans are registered against the loaded map but
// neither accumulated into it nor is it cropped.
// --map-fitness (with --scan-to-map): after each registration "map fitness: <value>" is printed -- getFitnessScore of the scan at
// its registered pose against the centroid cloud of the target it was registered to (ndt_get_centroid_fitness_score), before
// the scan is accumulated: the quality number an accumulated target, which keeps no points, can give.  Without the switch
// every line of output is as it was.
// --gicp [--gicp-gate <m>] (with --scan-to-map): every scan after the first is registered by GICP against the accumulated target
// (gicp_set_input_target_grid: the scan's k-NN covariances matched to the voxel distributions of the map, found through the map's
// own voxel table -- nothing is built over the map) instead of by NDT; the guess is the previous pose as before and the same
// per-scan lines are printed.  --gicp-gate: the correspondence distance in metres (default 5; a few leaves).  --map-fitness moves
// the scan by the GICP result.  Not with --nvtl, --covariance or --reject-unexplained, which read the NDT registration's result.
// --nvtl (with --scan-to-map): after each registration "nvtl: <value> found <n_found>/<n>" is printed -- the nearest-voxel
// transformation likelihood of the scan at its registered pose against the target it was registered to (ndt_get_nvtl), before
// the scan is accumulated: the number a localisation stack thresholds to accept or reject the pose.
// --covariance (with --scan-to-map): after each registration "pose sigma: sx sy sz sroll spitch syaw" is printed -- the square
// roots of the diagonal of the sandwich covariance of the registered pose (ndt_pose_covariance) against the target the scan
// was registered to, before the scan is accumulated; "nan" six times when the pose is not determined (NDT_COV_INDEFINITE).
// --deskew <field> (with --scan-to-map): every raw scan is motion-compensated first of all (ndt_cloud_deskew), before --range,
// --outliers-* and the prefilter.  The points' times are the named scalar field of the scan's file, the *_<number>.pcd of the directory
// (ndt_pcd_read_field); t_begin / t_end are the smallest and the largest finite time of the file and t_ref = t_begin.  The motion
// over the sweep is the increment between the two previous registered poses (constant velocity; the first scan's pose is the
// identity), so the first two scans -- and a file whose times are all one value -- go through as they are.  "deskewed:
// <n - untimed>/<n>" is printed per compensated scan; the points without a finite time become NaN and are dropped downstream.
// --range <min> <max> (with --scan-to-map): every raw scan goes through ndt_cloud_select (RANGE | FINITE about the sensor, centre
// 0) before its prefilter -- the ego vehicle's own returns and everything beyond the useful range are dropped on the device --
// and "range kept: <k>/<n>" is printed per scan.
// --outliers-radius <r> <min_neighbors> / --outliers-stat <mean_k> <stddev_mul> (with --scan-to-map): every raw scan goes through
// ndt_cloud_remove_outliers on the device, after --range and before its prefilter -- stray returns do not become one-point
// voxels -- and "outliers removed: <n - k>/<n>" is printed per scan (with both: the radius filter first).
// --ground <threshold> <hypotheses> <eps_deg> [--ground-remove] (with --scan-to-map): after --deskew, --range and --outliers-* and
// before its prefilter, the ground plane of every raw scan is found on the device (ndt_cloud_segment_plane: RANSAC over
// <hypotheses> hypotheses with the distance threshold <threshold>, seed 0, only planes whose normal lies within <eps_deg> degrees
// of (0, 0, 1) in the sensor frame, no refinement) and "ground: <inliers>/<n> normal <a> <b> <c> d <d>" is printed per scan; with
// --ground-remove the scan goes on without its inliers (and without the rows that are not finite).
// --flat <k> <curvature_max> (with --scan-to-map): last before its prefilter, every raw scan goes through
// ndt_cloud_select_by_normals on the device -- normals over the k nearest neighbours, the viewpoint the origin, and only the
// points of curvature <= curvature_max go on -- and "flat kept: <kept>/<n>" is printed per scan.
// --clusters <tolerance> <min_size> [<max_size>] (with --scan-to-map): after --ground and before its prefilter, every raw scan
// goes through ndt_cloud_extract_clusters on the device -- what stands on the ground split into objects, Euclidean clusters of
// points nearer than <tolerance>, and only the objects of min_size ... max_size points (no upper limit without <max_size>) go
// on: rain, noise and pedestrians smaller than min_size stay out of the map -- and "clusters: <C> kept <k>/<n>" is printed per
// scan.
// --reject-unexplained <L> (with --scan-to-map, not with --localize, which accumulates nothing): after each registration the
// scan is accumulated as ndt_source_select_by_nvtl(h, NULL, L, 1, ...) -- its points whose nearest-voxel likelihood at the
// registered pose is at least L, and those no voxel is near (new ground) -- instead of as the whole scan, so that moving objects
// the target does not explain stay out of it; "rejected: <n - k>/<n>" is printed.  The first scan has no target and is
// accumulated whole.
// --clear-rays <min_rays> <margin> (with --scan-to-map, not with --localize): every registered scan clears the map before it is
// accumulated (ndt_target_accumulate_clear_rays at its registered pose, the sensor origin the pose's translation): a voxel that
// at least min_rays of the scan's beams cross, up to `margin` metres before their hits, and that holds no point of the scan
// is dropped -- a car that has left, a door that has opened.  "cleared: <removed>/<voxels before>" is printed per scan.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <limits>
#include <dirent.h>
#include <mutex>
#include <string>
#include <thread>
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

struct Pt {
  float x, y, z, w;
};

static void print_matrix(const char* title, const float* T) {
  std::printf("%s\n", title);
  for (int r = 0; r < 4; r++) std::printf("  %.9g %.9g %.9g %.9g\n", T[r], T[4 + r], T[8 + r], T[12 + r]);
}

using clock_type = std::chrono::steady_clock;
static double since(clock_type::time_point a) { return std::chrono::duration<double, std::milli>(clock_type::now() - a).count(); }

// --deskew: the file of scan `number` in the directory -- the sequence hands out numbers, not names: the *.pcd whose stem ends
// in _<number> as the sequence itself reads it (ndt_host_extract_file_number); empty: none
static std::string scan_file(const std::string& directory, int number) {
  std::string found;
  if (DIR* d = opendir(directory.c_str())) {
    while (const dirent* e = readdir(d)) {
      const std::string name = e->d_name;
      if (name.size() < 5 || name.compare(name.size() - 4, 4, ".pcd") != 0) continue;
      if (ndt_host_extract_file_number(name.substr(0, name.size() - 4).c_str()) != number) continue;
      if (found.empty() || name < found) found = name;  // (two files of one number: the first by name)
    }
    closedir(d);
  }
  return found.empty() ? found : directory + "/" + found;
}

static const float kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

// NDT_PIPELINE_PARTITION=1: the pipeline's handles live on CU partitions instead of sharing the whole device
static bool use_partitions() {
  const char* v = std::getenv("NDT_PIPELINE_PARTITION");
  return v && std::atoi(v) != 0;
}

static int configure(ndt_handle h) {  // initialize_parameters / initialize_ndt, :37-62
  CHECK(ndt_set_resolution(h, 1.0f));
  CHECK(ndt_set_step_size(h, 0.1));
  CHECK(ndt_set_transformation_epsilon(h, 0.01));
  CHECK(ndt_set_maximum_iterations(h, 64));
  CHECK(ndt_set_num_threads(h, 40));
  CHECK(ndt_set_neighborhood_search_method(h, NDT_DIRECT7));
  return 0;
}

// a small blocking queue
template <class T>
class Channel {
 public:
  void put(T v) {
    {
      std::lock_guard<std::mutex> g(m_);
      q_.push_back(std::move(v));
    }
    cv_.notify_one();
  }
  T take() {
    std::unique_lock<std::mutex> lk(m_);
    cv_.wait(lk, [&] { return !q_.empty(); });
    T v = std::move(q_.front());
    q_.pop_front();
    return v;
  }

 private:
  std::mutex m_;
  std::condition_variable cv_;
  std::deque<T> q_;
};

// what the two loops share: the state of the node and what happens with a registration's result
struct Node {
  bool rosbag = false;
  bool scan_to_map = false;  // --scan-to-map: registrations against the accumulated target; a result is a pose in the map
  float window = 0;          // --window: half-side of the cube the accumulated target is cropped to after every scan (0: never)
  size_t max_voxels = 0;     // the largest voxel count the windowed target reached
  bool have_map = false;     // --load-target: the target holds a map before the first scan, which is registered like the others
  bool localize = false;     // --localize: the loaded map stays as it is
  bool map_fitness = false;  // --map-fitness: the centroid fitness of every registration is printed
  bool nvtl = false;         // --nvtl: the nearest-voxel transformation likelihood of every registration is printed
  bool covariance = false;   // --covariance: the standard deviations of every registered pose are printed
  bool range = false;        // --range: every raw scan is cropped to [range_min, range_max] about the sensor before its prefilter
  float range_min = 0, range_max = 0;
  bool outliers_radius = false, outliers_stat = false;  // --outliers-radius / --outliers-stat: every raw scan loses its outliers before its prefilter
  ndt_outlier_spec radius_spec{}, stat_spec{};
  bool ground = false, ground_remove = false;  // --ground: every raw scan's ground plane is found (and with --ground-remove dropped) before its prefilter
  ndt_plane_spec ground_spec{};
  bool clusters = false;  // --clusters: every raw scan goes on with its clustered points only
  bool flat = false;      // --flat: every raw scan goes on with its points of low curvature only
  ndt_normal_spec flat_spec{};
  ndt_normal_filter flat_filter{};
  ndt_cluster_spec cluster_spec{};
  std::string deskew_field;  // --deskew: every raw scan is motion-compensated by this field of its file, first of all
  std::string directory;
  bool reject = false;       // --reject-unexplained: a registered scan is accumulated without the points the target does not explain
  double reject_below = 0;
  bool clear_rays = false;   // --clear-rays: a registered scan clears the voxels it sees through before it is accumulated
  ndt_ray_spec ray_spec{};
  gicp_handle gicp = nullptr;  // --gicp: the registrations are GICP's against the accumulated target (bound to the NDT handle's grid)
  std::vector<std::vector<float>> trajectory;                     // trajectory_
  std::vector<float> pose = std::vector<float>(kIdentity, kIdentity + 16);
  std::vector<float> pres_transform = std::vector<float>(kIdentity, kIdentity + 16);  // rosbag node :33,95
  size_t loaded = 0, registered = 0, not_converged = 0;
  double t_filter = 0, t_align = 0, t_map = 0, t_wait = 0;  // t_wait: for the next file (the reader runs ahead in the background)

  // --scan-to-map: the scan into the accumulated target at its pose in the map (column-major), then the window around it
  // (seen: the whole registered scan, whose beams clear the map first -- --clear-rays)
  int accumulate(ndt_handle h, ndt_cloud scan, const float* map_pose, ndt_cloud seen = nullptr) {
    if (localize) return 0;
    if (clear_rays && seen) {
      size_t before = 0, removed = 0;
      CHECK(ndt_target_accumulated(h, nullptr, &before, nullptr));
      ndt_ray_spec spec = ray_spec;
      spec.min_range = 0.f;
      spec.max_range = 65536.f * ndt_get_resolution(h);  // every beam, whatever its length
      CHECK(ndt_target_accumulate_clear_rays(h, seen, map_pose, nullptr, &spec));
      if (before) CHECK(ndt_diag_target_clear_rays(h, nullptr, nullptr, nullptr, nullptr, &removed, nullptr, nullptr, nullptr, nullptr));
      std::printf("cleared: %zu/%zu\n", removed, before);
    }
    CHECK(ndt_target_accumulate_cloud(h, scan, 1, map_pose));
    if (window > 0) {
      const float lo[3] = {map_pose[12] - window, map_pose[13] - window, map_pose[14] - window};
      const float hi[3] = {map_pose[12] + window, map_pose[13] + window, map_pose[14] + window};
      CHECK(ndt_target_accumulate_crop(h, lo, hi));
      size_t voxels = 0;
      CHECK(ndt_target_accumulated(h, nullptr, &voxels, nullptr));
      max_voxels = std::max(max_voxels, voxels);
    }
    return 0;
  }

  // after align: -> whether the scan goes into the global map, and with which pose
  bool after_align(ndt_handle h, float* T, int converged, int iterations, std::vector<float>& map_pose, std::string& err,
                   ndt_cloud scan = nullptr) {
    registered++;
    if (map_fitness) {  // against the target the scan was registered to: the scan has not been accumulated yet
      double fitness = 0;
      ndt_status fs = NDT_OK;
      if (gicp) {  // the NDT handle has no result of this registration: the scan moved by GICP's
        const void* d_pts = nullptr;
        size_t n = 0;
        fs = ndt_cloud_data(scan, &d_pts, &n);
        const size_t offsets[2] = {0, n};
        if (fs == NDT_OK) fs = ndt_batch_centroid_fitness_scores_device(h, d_pts, offsets, 1, 16, T, 1.7976931348623157e308, &fitness);
      } else {
        fs = ndt_get_centroid_fitness_score(h, 1.7976931348623157e308, &fitness);
      }
      if (fs != NDT_OK) {
        err = ndt_last_error();
        return false;
      }
      std::printf("map fitness: %.9g\n", fitness);
    }
    if (nvtl) {  // likewise against the target the scan was registered to
      double value = 0;
      size_t found = 0, n = 0;
      if (ndt_get_nvtl(h, &value, &found) != NDT_OK || ndt_source_point_count(h, &n) != NDT_OK) {
        err = ndt_last_error();
        return false;
      }
      std::printf("nvtl: %.9g found %zu/%zu\n", value, found, n);
    }
    if (covariance) {  // likewise; the sandwich estimate has no tuning constant
      double cov[36];
      if (ndt_pose_covariance(h, nullptr, NDT_COV_SANDWICH, 1.0, cov, nullptr) != NDT_OK) {
        err = ndt_last_error();
        return false;
      }
      std::printf("pose sigma:");
      for (int k = 0; k < 6; k++) std::printf(" %.9g", std::sqrt(cov[7 * k]));
      std::printf("\n");
    }
    if (rosbag) {  // perform_registration :119-141, then :63-68
      double fitness = 0;
      if (ndt_get_fitness_score(h, 1.7976931348623157e308, &fitness) != NDT_OK) {
        err = ndt_last_error();
        return false;
      }
      std::printf("fitness: %.9g (%d iterations%s)\n", fitness, iterations, converged ? "" : ", not converged");
      if (!converged) {
        not_converged++;
        for (int i = 0; i < 16; i++) T[i] = kIdentity[i];
      }
      pres_transform.assign(T, T + 16);
      ndt_host_chain_pose(pose.data(), T, pose.data());
      trajectory.push_back(pose);
      map_pose = pose;
      return true;
    }
    if (converged) {
      char title[96];
      if (loaded < 2) std::snprintf(title, sizeof(title), "Transform map to %zu: (%d iterations)", loaded - 1, iterations);  // --load-target
      else std::snprintf(title, sizeof(title), "Transform %zu to %zu: (%d iterations)", loaded - 2, loaded - 1, iterations);
      print_matrix(title, T);
      std::vector<float> global(T, T + 16);
      if (!scan_to_map && !trajectory.empty()) ndt_host_chain_pose(trajectory.back().data(), T, global.data());  // trajectory_.back() * transform
      trajectory.push_back(global);
      map_pose = global;
      return true;
    }
    not_converged++;
    return false;
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// the node's loop as it stands, one handle, one step after the other -- with every cloud staying in HBM (the default):
// the raw scan goes up once (by the reader thread, ahead of time: ndt_pcd_sequence_stage), the prefilter leaves its result on the device as an
// ndt_cloud, and that one object is the source of this registration, the target of the next one and what the map update
// adds -- no download, no second or third upload / repack / bounding-box pass of the same points
// ---------------------------------------------------------------------------------------------------------------------
static int run_resident(Node& node, ndt_pcd_sequence_handle seq, float voxel_leaf_size, ndt_handle h, size_t first_poll) {
  // The prefilter of scan k + 1 is BEGUN (queued on the handle's filter stream: ndt_cloud_voxel_filter_begin -- its input's
  // boxes were computed by the reader, so nothing has to come back from the device first) before scan k is registered,
  // and ended when scan k + 1's turn comes: the node's steps in the node's order, the GPU working on two of them at once.
  struct Raw {
    ndt_cloud view = nullptr;  // the staged scan (the sequence's memory)
    size_t n = 0;
    int dense = 1, number = -1;
  };
  const char* ov_env = std::getenv("MAP_SEQUENCE_OVERLAP");
  const bool overlap = ov_env && std::atoi(ov_env) != 0;  // (measured: no gain, the loop is bound by the GPU's time; off)
  ndt_cloud previous = nullptr;  // clouds_[current_index_ - 1]
  Raw begun;                     // the scan whose prefilter is under way
  bool have_begun = false, queue_dry = first_poll == 0;
  int rc = 0;
  // the next queued scan -> its prefilter begun; false: nothing queued right now
  auto begin_next = [&]() -> int {
    for (;;) {
      Raw r;
      const void* host = nullptr;
      const auto t_next = clock_type::now();
      const ndt_status s = ndt_pcd_sequence_next_cloud(seq, &r.view, &host, &r.n, &r.dense, &r.number);
      node.t_wait += since(t_next);
      if (s != NDT_OK) {  // loadPCDFile == -1 -> nullptr -> skipped (:140, :128)
        std::fprintf(stderr, "skipped: %s\n", ndt_last_error());
        continue;
      }
      if (!r.view) {
        queue_dry = true;
        return 0;
      }
      const auto t0 = clock_type::now();
      if (!node.deskew_field.empty()) {
        // the poses registered so far, the first scan's (the identity, unless a loaded map came first) included
        const size_t n_poses = node.trajectory.size() + (node.have_map ? 0 : (node.loaded > 0 ? 1 : 0));
        std::vector<double> times(r.n ? r.n : 1);
        size_t n_times = 0;
        const std::string path = scan_file(node.directory, r.number);
        if (path.empty()) {
          std::fprintf(stderr, "--deskew: no *_%d.pcd in %s\n", r.number, node.directory.c_str());
          return 1;
        }
        CHECK(ndt_pcd_read_field(path.c_str(), node.deskew_field.c_str(), times.data(), r.n, &n_times));
        if (n_times != r.n)  // (the file changed between the sequence's read and this one)
          std::fprintf(stderr, "--deskew: %s holds %zu times for %zu points: scan %d is not compensated\n", path.c_str(), n_times, r.n, r.number);
        double lo = INFINITY, hi = -INFINITY;
        for (size_t i = 0; i < r.n; i++)
          if (std::isfinite(times[i])) {
            lo = std::min(lo, times[i]);
            hi = std::max(hi, times[i]);
          }
        // (MAP_SEQUENCE_OVERLAP=1 begins this prefilter before the previous scan is registered: the increment is then one scan
        // older, still the constant-velocity guess)
        if (n_poses >= 2 && n_times == r.n && hi > lo) {
          const float* B = node.trajectory.back().data();
          const float* A = node.trajectory.size() >= 2 ? node.trajectory[node.trajectory.size() - 2].data() : kIdentity;
          float inc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};  // A^-1 B, column-major, in f64
          for (int c = 0; c < 4; c++)
            for (int rr = 0; rr < 3; rr++) {
              double v = 0;
              for (int k = 0; k < 3; k++) v += static_cast<double>(A[4 * rr + k]) * (static_cast<double>(B[4 * c + k]) - (c == 3 ? static_cast<double>(A[12 + k]) : 0.0));
              inc[4 * c + rr] = static_cast<float>(v);
            }
          ndt_deskew_motion motion;
          CHECK(ndt_host_deskew_motion(inc, lo, hi, lo, &motion));
          ndt_cloud moved = nullptr;
          size_t untimed = 0;
          CHECK(ndt_cloud_deskew(h, r.view, &motion, times.data(), 0, &moved, &untimed));
          std::printf("deskewed: %zu/%zu\n", r.n - untimed, r.n);
          ndt_cloud_release(r.view);
          r.view = moved;
          if (untimed) r.dense = 0;
        }
      }
      if (node.range) {  // the crop leaves finite points only
        ndt_select_spec spec{};
        spec.flags = NDT_SELECT_RANGE | NDT_SELECT_FINITE;
        spec.r_min = node.range_min;
        spec.r_max = node.range_max;
        ndt_cloud cropped = nullptr;
        size_t kept = 0;
        CHECK(ndt_cloud_select(h, r.view, &spec, nullptr, 0, &cropped, nullptr, &kept));
        std::printf("range kept: %zu/%zu\n", kept, r.n);
        ndt_cloud_release(r.view);
        r.view = cropped;
        r.n = kept;
        r.dense = 1;
      }
      for (const ndt_outlier_spec* spec : {node.outliers_radius ? &node.radius_spec : nullptr, node.outliers_stat ? &node.stat_spec : nullptr}) {
        if (!spec) continue;  // what is left holds finite points only
        ndt_cloud cleaned = nullptr;
        size_t kept = 0;
        CHECK(ndt_cloud_remove_outliers(h, r.view, spec, &cleaned, nullptr, &kept, nullptr));
        std::printf("outliers removed: %zu/%zu\n", r.n - kept, r.n);
        ndt_cloud_release(r.view);
        r.view = cleaned;
        r.n = kept;
        r.dense = 1;
      }
      if (node.ground) {
        ndt_plane_result plane{};
        ndt_cloud rest = nullptr;
        CHECK(ndt_cloud_segment_plane(h, r.view, &node.ground_spec, nullptr, &plane, nullptr, node.ground_remove ? &rest : nullptr));
        std::printf("ground: %zu/%zu normal %.9g %.9g %.9g d %.9g\n", plane.n_inliers, r.n, plane.coeff[0], plane.coeff[1], plane.coeff[2],
                    plane.coeff[3]);
        if (node.ground_remove) {  // what is left holds finite points only
          ndt_cloud_release(r.view);
          r.view = rest;
          r.n = plane.n_finite - plane.n_inliers;
          r.dense = 1;
        }
      }
      if (node.clusters) {  // what is left holds finite points only
        ndt_cloud objects = nullptr;
        size_t kept = 0;
        ndt_cluster_summary sum{};
        CHECK(ndt_cloud_extract_clusters(h, r.view, &node.cluster_spec, 0, &objects, nullptr, &kept, &sum));
        std::printf("clusters: %zu kept %zu/%zu\n", sum.n_clusters, kept, r.n);
        ndt_cloud_release(r.view);
        r.view = objects;
        r.n = kept;
        r.dense = 1;
      }
      if (node.flat) {  // what is left holds finite points only
        ndt_cloud smooth = nullptr;
        size_t kept = 0;
        CHECK(ndt_cloud_select_by_normals(h, r.view, &node.flat_spec, &node.flat_filter, &smooth, nullptr, &kept, nullptr));
        std::printf("flat kept: %zu/%zu\n", kept, r.n);
        ndt_cloud_release(r.view);
        r.view = smooth;
        r.n = kept;
        r.dense = 1;
      }
      CHECK(ndt_cloud_voxel_filter_begin(h, r.view, r.dense, voxel_leaf_size));
      node.t_filter += since(t0);
      begun = r;
      have_begun = true;
      return 0;
    }
  };
  for (; !rc;) {
    if (!have_begun) {
      if (queue_dry) {  // process_new_clouds looks at the directory (the first look ran before the device's start-up)
        size_t fresh = 0;
        CHECK(ndt_pcd_sequence_poll(seq, node.loaded, &fresh));
        if (fresh == 0) break;
        queue_dry = false;
      }
      if (begin_next()) return 1;
      if (!have_begun) continue;  // (every queued file was unreadable: look again)
    }
    // ---- load_and_filter_cloud of this scan ends (:142-148) ...
    auto t0 = clock_type::now();
    ndt_cloud current = nullptr;
    int overflowed = 0;
    size_t m = 0;
    if (ndt_cloud_voxel_filter_end(h, &current, &overflowed) != NDT_OK || ndt_cloud_size(current, &m) != NDT_OK) {
      std::fprintf(stderr, "voxel filter failed: %s\n", ndt_last_error());
      return 1;
    }
    node.t_filter += since(t0);
    const int number = begun.number;
    ndt_cloud_release(begun.view);
    have_begun = false;
    // ... and the next scan's begins.  Not across a look at the directory: process_new_clouds counts the clouds KEPT so far,
    // and whether the scan in flight is kept (not empty) is known only when its filter has ended.
    if (overlap && !queue_dry && begin_next()) return 1;
    if (m == 0) {  // :128 -- empty clouds are not kept
      ndt_cloud_release(current);
      continue;
    }
    node.loaded++;
    std::printf("Loaded cloud_%d.pcd (%zu points)\n", number, m);
    auto step = [&]() -> int {
      if (node.loaded == 1 && !node.have_map) {  // load_initial_clouds, :64-68
        t0 = clock_type::now();
        int ov = 0;
        CHECK(ndt_map_update_cloud(h, current, 1, kIdentity, 0.5f, &ov));
        if (node.scan_to_map && node.accumulate(h, current, kIdentity)) return 1;
        node.t_map += since(t0);
        return 0;
      }
      t0 = clock_type::now();  // process_available_clouds, :70-100
      if (!node.scan_to_map) CHECK(ndt_set_input_target_cloud(h, previous, 1));
      if (!node.gicp) CHECK(ndt_set_input_source_cloud(h, current));
      float T[16];
      int converged = 0, iterations = 0;
      double probability = 0;
      const float* guess = node.rosbag ? node.pres_transform.data() : nullptr;
      if (node.scan_to_map) guess = node.trajectory.empty() ? kIdentity : node.trajectory.back().data();  // the previous scan's pose
      if (node.gicp) {  // against the accumulated target as it is now: the binding reads the map's grid at every call
        CHECK(gicp_set_input_source_cloud(node.gicp, current));
        CHECK(gicp_align(node.gicp, guess, T, &converged, &iterations, nullptr));
      } else {
        CHECK(ndt_align(h, guess, T, &converged, &iterations, &probability, nullptr, 0));
      }
      node.t_align += since(t0);
      std::vector<float> map_pose;
      std::string err;
      const bool into_map = node.after_align(h, T, converged, iterations, map_pose, err, current);
      if (!err.empty()) {
        std::fprintf(stderr, "%s\n", err.c_str());
        return 1;
      }
      if (into_map) {
        t0 = clock_type::now();
        int ov = 0;
        CHECK(ndt_map_update_cloud(h, current, 1, map_pose.data(), 0.5f, &ov));  // :204 / map_voxel :88: leaf fixed at 0.5
        if (node.scan_to_map && node.reject && !node.localize) {  // the source is still `current`, the last result this registration's
          ndt_cloud explained = nullptr;
          size_t kept = 0;
          CHECK(ndt_source_select_by_nvtl(h, nullptr, node.reject_below, 1, &explained, &kept, nullptr));
          std::printf("rejected: %zu/%zu\n", m - kept, m);
          const int failed = node.accumulate(h, explained, map_pose.data(), current);
          ndt_cloud_release(explained);
          if (failed) return 1;
        } else if (node.scan_to_map && node.accumulate(h, current, map_pose.data(), current)) {
          return 1;
        }
        node.t_map += since(t0);
      }
      return 0;
    };
    rc = step();
    ndt_cloud_release(previous);
    previous = current;
  }
  if (have_begun) {  // (left over after an error)
    ndt_cloud c = nullptr;
    (void)ndt_cloud_voxel_filter_end(h, &c, nullptr);
    ndt_cloud_release(c);
    ndt_cloud_release(begun.view);
  }
  ndt_cloud_release(previous);
  return rc;
}

// ---------------------------------------------------------------------------------------------------------------------
// the same loop through host buffers, as a caller that holds its clouds in host memory (PCL) has to run it
// ---------------------------------------------------------------------------------------------------------------------
static int run_serial(Node& node, ndt_pcd_sequence_handle seq, float voxel_leaf_size, ndt_handle h) {
  std::vector<Pt> previous, current;  // clouds_[current_index_ - 1], clouds_[current_index_]
  for (;;) {  // the node polls the directory once per second (:28-34); here: until a poll brings nothing new
    size_t fresh = 0;
    CHECK(ndt_pcd_sequence_poll(seq, node.loaded, &fresh));
    if (fresh == 0) break;
    for (;;) {
      const void* raw = nullptr;
      size_t n = 0;
      int dense = 1, number = -1;
      const ndt_status s = ndt_pcd_sequence_next(seq, &raw, &n, &dense, &number);
      if (s != NDT_OK) {  // loadPCDFile == -1 -> nullptr -> skipped (:140, :128)
        std::fprintf(stderr, "skipped: %s\n", ndt_last_error());
        continue;
      }
      if (!raw) break;
      // load_and_filter_cloud, :142-148
      auto t0 = clock_type::now();
      current.resize(n ? n : 1);
      size_t m = 0;
      const ndt_status fs = ndt_voxel_grid_filter(h, raw, n, sizeof(Pt), dense, voxel_leaf_size, current.data(), sizeof(Pt), &m);
      if (fs != NDT_OK && fs != NDT_ERR_GRID_OVERFLOW) {
        std::fprintf(stderr, "voxel filter failed: %s\n", ndt_last_error());
        return 1;
      }
      current.resize(m);
      node.t_filter += since(t0);
      if (current.empty()) continue;  // :128 -- empty clouds are not kept
      node.loaded++;
      std::printf("Loaded cloud_%d.pcd (%zu points)\n", number, current.size());
      if (node.loaded == 1) {  // load_initial_clouds, :64-68
        t0 = clock_type::now();
        int overflowed = 0;
        CHECK(ndt_map_update(h, current.data(), current.size(), sizeof(Pt), 1, kIdentity, 0.5f, &overflowed));
        node.t_map += since(t0);
      } else {  // process_available_clouds, :70-100
        t0 = clock_type::now();
        CHECK(ndt_set_input_target(h, previous.data(), previous.size(), sizeof(Pt), 1));
        CHECK(ndt_set_input_source(h, current.data(), current.size(), sizeof(Pt)));
        float T[16];
        int converged = 0, iterations = 0;
        double probability = 0;
        CHECK(ndt_align(h, node.rosbag ? node.pres_transform.data() : nullptr, T, &converged, &iterations, &probability, nullptr, 0));
        node.t_align += since(t0);
        std::vector<float> map_pose;
        std::string err;
        const bool into_map = node.after_align(h, T, converged, iterations, map_pose, err);
        if (!err.empty()) {
          std::fprintf(stderr, "%s\n", err.c_str());
          return 1;
        }
        if (into_map) {
          t0 = clock_type::now();
          int overflowed = 0;
          CHECK(ndt_map_update(h, current.data(), current.size(), sizeof(Pt), 1, map_pose.data(), 0.5f, &overflowed));  // :204 / map_voxel :88: leaf fixed at 0.5
          node.t_map += since(t0);
        }
      }
      previous.swap(current);
    }
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// the same loop with the steps of consecutive scans overlapped
// ---------------------------------------------------------------------------------------------------------------------
struct Prepared {
  ndt_handle h = nullptr;   // prep handle holding the filtered scan as input source AND as (built) input target
  std::vector<Pt> cloud;    // the filtered scan on the host (for the map update)
  int number = -1;
  double filter_ms = 0;
  bool end = false;
  std::string error;
};
struct MapJob {
  std::vector<Pt> cloud;
  std::vector<float> pose;
  bool end = false;
};

static int run_pipelined(Node& node, ndt_pcd_sequence_handle seq, float voxel_leaf_size, ndt_handle h, ndt_handle map_handle) {
  // three prep handles rotate: one being prepared, one holding the current source, one holding the current target
  constexpr int kPrep = 3;
  ndt_handle prep[kPrep] = {nullptr, nullptr, nullptr};
  for (int i = 0; i < kPrep; i++) {
    CHECK(ndt_create(0, &prep[i]));
    if (configure(prep[i])) return 1;
    if (use_partitions()) CHECK(ndt_set_cu_partition(prep[i], 2));
  }
  Channel<ndt_handle> free_prep;
  for (int i = 0; i < kPrep; i++) free_prep.put(prep[i]);
  Channel<Prepared> prepared;
  Channel<MapJob> map_jobs;
  std::string map_error;
  double map_ms = 0;

  std::thread prep_thread([&] {
    size_t kept = 0;  // clouds_.size() as process_new_clouds sees it
    for (;;) {
      size_t fresh = 0;
      if (ndt_pcd_sequence_poll(seq, kept, &fresh) != NDT_OK) {
        Prepared e;
        e.end = true;
        e.error = ndt_last_error();
        prepared.put(std::move(e));
        return;
      }
      if (fresh == 0) break;
      for (;;) {
        const void* raw = nullptr;
        size_t n = 0;
        int dense = 1, number = -1;
        const ndt_status s = ndt_pcd_sequence_next(seq, &raw, &n, &dense, &number);
        if (s != NDT_OK) {
          std::fprintf(stderr, "skipped: %s\n", ndt_last_error());
          continue;
        }
        if (!raw) break;
        Prepared p;
        p.number = number;
        p.h = free_prep.take();
        const auto t0 = clock_type::now();
        p.cloud.resize(n ? n : 1);
        size_t m = 0;
        const ndt_status fs = ndt_voxel_grid_filter(p.h, raw, n, sizeof(Pt), dense, voxel_leaf_size, p.cloud.data(), sizeof(Pt), &m);
        if (fs != NDT_OK && fs != NDT_ERR_GRID_OVERFLOW) {
          p.end = true;
          p.error = std::string("voxel filter failed: ") + ndt_last_error();
          prepared.put(std::move(p));
          return;
        }
        p.cloud.resize(m);
        p.filter_ms = since(t0);
        if (p.cloud.empty()) {  // :128 -- empty clouds are not kept
          free_prep.put(p.h);
          continue;
        }
        kept++;
        // the scan is the source of this registration and the target of the next one
        if (ndt_set_input_source(p.h, p.cloud.data(), p.cloud.size(), sizeof(Pt)) != NDT_OK ||
            ndt_set_input_target(p.h, p.cloud.data(), p.cloud.size(), sizeof(Pt), 1) != NDT_OK) {
          p.end = true;
          p.error = std::string("preparing the inputs failed: ") + ndt_last_error();
          prepared.put(std::move(p));
          return;
        }
        prepared.put(std::move(p));
      }
    }
    Prepared e;
    e.end = true;
    prepared.put(std::move(e));
  });
  std::thread map_thread([&] {
    for (;;) {
      MapJob j = map_jobs.take();
      if (j.end) return;
      if (!map_error.empty()) continue;
      const auto t0 = clock_type::now();
      int overflowed = 0;
      if (ndt_map_update(map_handle, j.cloud.data(), j.cloud.size(), sizeof(Pt), 1, j.pose.data(), 0.5f, &overflowed) != NDT_OK)
        map_error = ndt_last_error();
      map_ms += since(t0);
    }
  });

  int rc = 0;
  bool producer_done = false;  // the prep thread's end message has been taken: nothing more will come
  Prepared previous;
  for (;;) {
    Prepared cur = prepared.take();
    if (cur.end) {
      producer_done = true;
      if (!cur.error.empty()) {
        std::fprintf(stderr, "%s\n", cur.error.c_str());
        rc = 1;
      }
      break;
    }
    node.t_filter += cur.filter_ms;
    node.loaded++;
    std::printf("Loaded cloud_%d.pcd (%zu points)\n", cur.number, cur.cloud.size());
    if (node.loaded == 1) {  // load_initial_clouds, :64-68
      MapJob j;
      j.cloud = cur.cloud;
      j.pose.assign(kIdentity, kIdentity + 16);
      map_jobs.put(std::move(j));
    } else {
      const auto t0 = clock_type::now();
      float T[16];
      int converged = 0, iterations = 0;
      double probability = 0;
      if (ndt_share_input_target(h, previous.h) != NDT_OK || ndt_share_input_source(h, cur.h) != NDT_OK ||
          ndt_align(h, node.rosbag ? node.pres_transform.data() : nullptr, T, &converged, &iterations, &probability, nullptr, 0) != NDT_OK) {
        std::fprintf(stderr, "registration failed: %s\n", ndt_last_error());
        rc = 1;
        free_prep.put(cur.h);
        break;
      }
      node.t_align += since(t0);
      std::vector<float> map_pose;
      std::string err;
      const bool into_map = node.after_align(h, T, converged, iterations, map_pose, err);
      if (!err.empty()) {
        std::fprintf(stderr, "%s\n", err.c_str());
        rc = 1;
        free_prep.put(cur.h);
        break;
      }
      if (into_map) {
        MapJob j;
        j.cloud = cur.cloud;
        j.pose = map_pose;
        map_jobs.put(std::move(j));
      }
    }
    if (previous.h) free_prep.put(previous.h);  // its grid stays alive for as long as the registration handle shares it
    previous = std::move(cur);
  }
  if (rc && !producer_done) {  // let the prep thread run dry: every handle it may be waiting for goes back to it
    if (previous.h) free_prep.put(previous.h);
    for (;;) {
      Prepared p = prepared.take();
      if (p.end) break;
      free_prep.put(p.h);
    }
  }
  MapJob stop;
  stop.end = true;
  map_jobs.put(std::move(stop));
  prep_thread.join();
  map_thread.join();
  node.t_map += map_ms;
  if (!map_error.empty()) {
    std::fprintf(stderr, "map update failed: %s\n", map_error.c_str());
    rc = 1;
  }
  for (int i = 0; i < kPrep; i++) ndt_destroy(prep[i]);
  return rc;
}

int main(int argc, char** argv) {
  bool scan_to_map = false, bad_window = false, localize = false, bad_file = false, map_fitness = false, nvtl = false, covariance = false;
  bool range = false, bad_range = false, reject = false, bad_reject = false;
  bool outliers_radius = false, outliers_stat = false, bad_outliers = false;
  bool use_gicp = false, have_gate = false, bad_gate = false;
  bool clear_rays = false, bad_clear = false;
  ndt_ray_spec ray_spec{};
  double gicp_gate = 5.0;
  ndt_outlier_spec radius_spec{}, stat_spec{};
  bool ground = false, ground_remove = false, bad_ground = false;
  ndt_plane_spec ground_spec{};
  bool clusters = false, bad_clusters = false;
  ndt_cluster_spec cluster_spec{};
  bool flat = false, bad_flat = false;
  ndt_normal_spec flat_spec{};
  ndt_normal_filter flat_filter{};
  float window = 0, range_min = 0, range_max = 0;
  double reject_below = 0;
  const char *save_target = nullptr, *load_target = nullptr, *deskew_field = nullptr;
  bool bad_deskew = false;
  static const char kUsage[] =
      "usage: map_sequence [--scan-to-map [--window <metres>] [--map-fitness] [--nvtl] [--covariance] [--gicp [--gicp-gate <m>]] [--deskew <field>] [--range <min> <max>] [--outliers-radius <r> <min_neighbors>] [--outliers-stat <mean_k> <stddev_mul>] [--ground <threshold> <hypotheses> <eps_deg> [--ground-remove]] [--clusters <tolerance> <min_size> [<max_size>]] [--flat <k> <curvature_max>] [--reject-unexplained <L>] [--clear-rays <min_rays> <margin>] [--save-target <file>] [--load-target <file> [--localize]]] <pcd_directory> "
      "[voxel_leaf_size] [global_map_out.pcd | -] [rosbag | node] [serial | pipeline] [host]\n";
  {  // the switches are taken out of the line before the positional arguments are read
    int kept = 1;
    for (int i = 1; i < argc; i++) {
      if (std::strcmp(argv[i], "--scan-to-map") == 0) {
        scan_to_map = true;
      } else if (std::strcmp(argv[i], "--window") == 0) {
        window = i + 1 < argc ? static_cast<float>(std::atof(argv[++i])) : 0.f;
        bad_window = !(window > 0);
      } else if (std::strcmp(argv[i], "--save-target") == 0 || std::strcmp(argv[i], "--load-target") == 0) {
        const char*& file = argv[i][2] == 's' ? save_target : load_target;
        file = i + 1 < argc ? argv[++i] : nullptr;
        bad_file = bad_file || !file;
      } else if (std::strcmp(argv[i], "--localize") == 0) {
        localize = true;
      } else if (std::strcmp(argv[i], "--map-fitness") == 0) {
        map_fitness = true;
      } else if (std::strcmp(argv[i], "--nvtl") == 0) {
        nvtl = true;
      } else if (std::strcmp(argv[i], "--covariance") == 0) {
        covariance = true;
      } else if (std::strcmp(argv[i], "--gicp") == 0) {
        use_gicp = true;
      } else if (std::strcmp(argv[i], "--gicp-gate") == 0) {
        have_gate = true;
        gicp_gate = i + 1 < argc ? std::atof(argv[++i]) : 0.0;
        bad_gate = !(gicp_gate > 0);
      } else if (std::strcmp(argv[i], "--deskew") == 0) {
        deskew_field = i + 1 < argc ? argv[++i] : nullptr;
        bad_deskew = !deskew_field || !*deskew_field;
      } else if (std::strcmp(argv[i], "--range") == 0) {
        range = true;
        bad_range = i + 2 >= argc;
        if (!bad_range) {
          range_min = static_cast<float>(std::atof(argv[++i]));
          range_max = static_cast<float>(std::atof(argv[++i]));
          bad_range = !(range_min >= 0 && range_min <= range_max);
        }
      } else if (std::strcmp(argv[i], "--outliers-radius") == 0 || std::strcmp(argv[i], "--outliers-stat") == 0) {
        const bool by_radius = argv[i][11] == 'r';
        (by_radius ? outliers_radius : outliers_stat) = true;
        ndt_outlier_spec& spec = by_radius ? radius_spec : stat_spec;
        if (i + 2 >= argc) {
          bad_outliers = true;
        } else if (by_radius) {
          spec.method = NDT_OUTLIER_RADIUS;
          spec.radius = static_cast<float>(std::atof(argv[++i]));
          spec.min_neighbors = std::atoi(argv[++i]);
        } else {
          spec.method = NDT_OUTLIER_STATISTICAL;
          spec.mean_k = std::atoi(argv[++i]);
          spec.stddev_mul = std::atof(argv[++i]);
        }
        bad_outliers = bad_outliers || ndt_host_outlier_spec_check(&spec) != NDT_OK;
      } else if (std::strcmp(argv[i], "--ground") == 0) {
        ground = true;
        bad_ground = i + 3 >= argc;
        if (!bad_ground) {
          ground_spec.distance_threshold = static_cast<float>(std::atof(argv[++i]));
          ground_spec.n_hypotheses = std::atoi(argv[++i]);
          const double eps_deg = std::atof(argv[++i]);
          ground_spec.eps_angle = static_cast<float>(eps_deg * 3.14159265358979323846 / 180.0);
          if (eps_deg <= 90.0 && static_cast<double>(ground_spec.eps_angle) > 1.5707963267948966)  // (90 degrees round up in f32)
            ground_spec.eps_angle = std::nextafterf(ground_spec.eps_angle, 0.0f);
          ground_spec.use_axis = 1;
          ground_spec.axis[2] = 1.0f;
          bad_ground = ndt_host_plane_spec_check(&ground_spec) != NDT_OK;
        }
      } else if (std::strcmp(argv[i], "--ground-remove") == 0) {
        ground_remove = true;
      } else if (std::strcmp(argv[i], "--clusters") == 0) {
        clusters = true;
        bad_clusters = i + 2 >= argc;
        if (!bad_clusters) {
          cluster_spec.tolerance = static_cast<float>(std::atof(argv[++i]));
          cluster_spec.min_size = std::atoi(argv[++i]);
          cluster_spec.max_size = std::numeric_limits<int>::max();
          // (the optional <max_size> is a number; the directory that follows the switches is not)
          if (i + 1 < argc && argv[i + 1][0] != '\0' && std::strspn(argv[i + 1], "0123456789") == std::strlen(argv[i + 1]))
            cluster_spec.max_size = std::atoi(argv[++i]);
          bad_clusters = ndt_host_cluster_spec_check(&cluster_spec) != NDT_OK;
        }
      } else if (std::strcmp(argv[i], "--flat") == 0) {
        flat = true;
        bad_flat = i + 2 >= argc;
        if (!bad_flat) {
          flat_spec.method = NDT_NORMAL_KNN;
          flat_spec.k = std::atoi(argv[++i]);
          flat_spec.min_neighbors = 3;  // (the viewpoint stays the origin: the sensor of a raw scan)
          flat_filter.flags = NDT_NORMAL_KEEP_CURVATURE;
          flat_filter.curvature_lo = 0.f;
          flat_filter.curvature_hi = static_cast<float>(std::atof(argv[++i]));
          bad_flat = ndt_host_normal_spec_check(&flat_spec) != NDT_OK || ndt_host_normal_filter_check(&flat_filter) != NDT_OK;
        }
      } else if (std::strcmp(argv[i], "--clear-rays") == 0) {
        clear_rays = true;
        bad_clear = i + 2 >= argc;
        if (!bad_clear) {
          ray_spec.min_rays = std::atoi(argv[++i]);
          ray_spec.margin = static_cast<float>(std::atof(argv[++i]));
          bad_clear = !(ray_spec.min_rays >= 1 && ray_spec.margin >= 0 && std::isfinite(ray_spec.margin));
        }
      } else if (std::strcmp(argv[i], "--reject-unexplained") == 0) {
        reject = true;
        bad_reject = i + 1 >= argc;
        if (!bad_reject) {
          reject_below = std::atof(argv[++i]);
          bad_reject = reject_below != reject_below;
        }
      } else {
        argv[kept++] = argv[i];
      }
    }
    argc = kept;
  }
  if (bad_window || (window > 0 && !scan_to_map)) {
    std::fprintf(stderr, "--window <metres> takes a positive half-side and goes with --scan-to-map\n");
    return 2;
  }
  if (bad_file || ((save_target || load_target) && !scan_to_map) || (localize && !load_target)) {
    std::fprintf(stderr, "--save-target <file> and --load-target <file> go with --scan-to-map, --localize goes with --load-target\n%s", kUsage);
    return 2;
  }
  if ((map_fitness || nvtl || covariance) && !scan_to_map) {
    std::fprintf(stderr, "--map-fitness, --nvtl and --covariance go with --scan-to-map\n%s", kUsage);
    return 2;
  }
  if (bad_range || bad_reject || ((range || reject) && !scan_to_map) || (reject && localize)) {
    std::fprintf(stderr, "--range <min> <max> (0 <= min <= max) and --reject-unexplained <L> go with --scan-to-map; --localize accumulates "
                         "nothing, so it does not go with --reject-unexplained\n%s", kUsage);
    return 2;
  }
  if (bad_clear || (clear_rays && (!scan_to_map || localize))) {
    std::fprintf(stderr, "--clear-rays <min_rays> <margin> (min_rays >= 1, margin >= 0) goes with --scan-to-map; --localize leaves the map as it "
                         "is, so it does not go with --clear-rays\n%s", kUsage);
    return 2;
  }
  if (bad_deskew || (deskew_field && !scan_to_map)) {
    std::fprintf(stderr, "--deskew <field> names the time field of the scans' files and goes with --scan-to-map\n%s", kUsage);
    return 2;
  }
  if (bad_outliers || ((outliers_radius || outliers_stat) && !scan_to_map)) {
    std::fprintf(stderr, "--outliers-radius <r> <min_neighbors> (r > 0, min_neighbors >= 0) and --outliers-stat <mean_k> <stddev_mul> (mean_k 1 ... 256) "
                         "go with --scan-to-map\n%s", kUsage);
    return 2;
  }
  if (bad_ground || (ground && !scan_to_map) || (ground_remove && !ground)) {
    std::fprintf(stderr, "--ground <threshold> <hypotheses> <eps_deg> (threshold > 0, hypotheses 1 ... 65536, 0 <= eps_deg <= 90) goes with "
                         "--scan-to-map and --ground-remove with --ground\n%s", kUsage);
    return 2;
  }
  if (bad_clusters || (clusters && !scan_to_map)) {
    std::fprintf(stderr, "--clusters <tolerance> <min_size> [<max_size>] (tolerance > 0, 1 <= min_size <= max_size) goes with --scan-to-map\n%s",
                 kUsage);
    return 2;
  }
  if (bad_flat || (flat && !scan_to_map)) {
    std::fprintf(stderr, "--flat <k> <curvature_max> (k 3 ... 256, curvature_max >= 0) goes with --scan-to-map\n%s", kUsage);
    return 2;
  }
  if (bad_gate || (have_gate && !use_gicp) || (use_gicp && (!scan_to_map || nvtl || covariance || reject))) {
    std::fprintf(stderr, "--gicp goes with --scan-to-map and --gicp-gate <m> (m > 0) with --gicp; --nvtl, --covariance and --reject-unexplained "
                         "read the NDT registration's result, so they do not go with --gicp\n%s", kUsage);
    return 2;
  }
  if (argc < 2) {
    std::printf("%s", kUsage);
    return 0;
  }
  Node node;
  node.rosbag = argc > 4 && std::strcmp(argv[4], "rosbag") == 0;
  const bool serial = !(argc > 5 && std::strcmp(argv[5], "pipeline") == 0);
  const bool host_clouds = argc > 6 && std::strcmp(argv[6], "host") == 0;  // serial only: every cloud through host buffers
  node.scan_to_map = scan_to_map;
  node.window = window;
  node.have_map = load_target != nullptr;
  node.localize = localize;
  node.map_fitness = map_fitness;
  node.nvtl = nvtl;
  node.covariance = covariance;
  node.clear_rays = clear_rays;
  node.ray_spec = ray_spec;
  node.range = range;
  node.range_min = range_min;
  node.range_max = range_max;
  node.outliers_radius = outliers_radius;
  node.outliers_stat = outliers_stat;
  node.radius_spec = radius_spec;
  node.stat_spec = stat_spec;
  node.ground = ground;
  node.ground_remove = ground_remove;
  node.ground_spec = ground_spec;
  node.clusters = clusters;
  node.cluster_spec = cluster_spec;
  node.flat = flat;
  node.flat_spec = flat_spec;
  node.flat_filter = flat_filter;
  if (deskew_field) node.deskew_field = deskew_field;
  node.directory = argv[1];
  node.reject = reject;
  node.reject_below = reject_below;
  if (scan_to_map && (node.rosbag || !serial || host_clouds)) {
    // (the rosbag loop prints getFitnessScore, which needs the target's points: an accumulated target keeps none --
    // --map-fitness prints the fitness against its voxel centroids instead)
    std::fprintf(stderr, "--scan-to-map runs the node's serial loop with resident clouds: not with rosbag, pipeline or host\n");
    return 2;
  }
  const float voxel_leaf_size = argc > 2 ? static_cast<float>(std::atof(argv[2])) : (node.rosbag ? 0.3f : 0.5f);  // :44 / rosbag :87
  ndt_handle h = nullptr, map_handle = nullptr;
  CHECK(ndt_create(0, &h));
  if (configure(h)) return 1;
  if (!serial) {
    if (use_partitions()) CHECK(ndt_set_cu_partition(h, 1));
    CHECK(ndt_create(0, &map_handle));
    if (use_partitions()) CHECK(ndt_set_cu_partition(map_handle, 2));
  }

  ndt_pcd_sequence_handle seq = nullptr;
  CHECK(ndt_pcd_sequence_open(argv[1], &seq));
  // a node constructs its objects (and a GPU library loads its code, creates its streams, page-locks its slots) before the
  // first scan arrives: not part of any scan's time
  const auto t_warm = clock_type::now();
  size_t first_poll = 0;
  if (serial && !host_clouds) {
    CHECK(ndt_pcd_sequence_stage(seq, 0));             // the reader uploads every scan as soon as it has parsed it
    CHECK(ndt_pcd_sequence_poll(seq, 0, &first_poll));  // process_new_clouds' first look at the directory: the reads start now
  }
  CHECK(ndt_warm_up(h, 65536));  // (a node knows its sensor: the reference's scans are lidar sweeps of some ten thousand points)
  if (map_handle) CHECK(ndt_warm_up(map_handle, 65536));
  if (load_target) CHECK(ndt_target_accumulate_load(h, load_target));  // the map is there before the first scan arrives
  if (use_gicp) {  // (bound once: every registration reads the accumulated target as it is then)
    CHECK(gicp_create(0, &node.gicp));
    CHECK(gicp_set_max_correspondence_distance(node.gicp, gicp_gate));
    CHECK(gicp_set_input_target_grid(node.gicp, h, GICP_VOXEL_COV_PLANE));
  }
  const double warm_ms = since(t_warm);
  const auto t_begin = clock_type::now();
  const int rc = !serial ? run_pipelined(node, seq, voxel_leaf_size, h, map_handle)
                         : host_clouds ? run_serial(node, seq, voxel_leaf_size, h) : run_resident(node, seq, voxel_leaf_size, h, first_poll);
  if (rc) return rc;

  ndt_handle mh = serial ? h : map_handle;
  size_t map_points = 0;
  CHECK(ndt_map_size(mh, &map_points));
  std::printf("\nclouds %zu  registrations %zu (not converged %zu)  global map %zu points\n", node.loaded, node.registered, node.not_converged, map_points);
  for (size_t i = 0; i < node.trajectory.size(); i++) {
    char title[64];
    std::snprintf(title, sizeof(title), "trajectory[%zu]:", i);
    print_matrix(title, node.trajectory[i].data());
  }
  if (node.window > 0) std::printf("window %g m: the accumulated target reached %zu voxels at most\n", node.window, node.max_voxels);
  if (save_target) {
    size_t voxels = 0;
    CHECK(ndt_target_accumulate_save(h, nullptr, nullptr, save_target));
    CHECK(ndt_diag_target_export(h, &voxels, nullptr, nullptr));
    std::printf("accumulated target saved: %zu voxels, %zu bytes\n", voxels, 64 + 104 * voxels);
  }
  std::printf("start-up (device, code object, page-locked slots; ndt_warm_up): %.1f ms, not in the times below\n", warm_ms);
  std::printf("time: total %.2f ms  (prefilter %.2f, %s %.2f, map update %.2f, waiting for the next file %.2f; %s)\n", since(t_begin), node.t_filter,
              serial ? "set inputs + align" : "take inputs over + align", node.t_align, node.t_map, node.t_wait,
              !serial ? "file reading, prefilter + input preparation and map update overlapped with the registrations"
                      : host_clouds ? "file reading overlapped; clouds through host buffers" : "file reading overlapped; clouds resident in HBM");
  if (argc > 3 && std::strcmp(argv[3], "-") != 0 && map_points) {
    std::vector<Pt> map(map_points);
    CHECK(ndt_map_get(mh, map.data(), sizeof(Pt)));
    CHECK(ndt_pcd_write_xyz(argv[3], map.data(), map.size(), sizeof(Pt), 1));
    std::printf("global map written to %s\n", argv[3]);
  }
  ndt_pcd_sequence_close(seq);
  if (node.gicp) gicp_destroy(node.gicp);  // (before the handle it borrows)
  ndt_destroy(h);
  if (map_handle) ndt_destroy(map_handle);
  return 0;
}
