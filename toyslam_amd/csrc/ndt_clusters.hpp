// ndt_clusters.hpp -- what the host entries and the kernels of the Euclidean cluster extraction (ndt_clusters.hip) share: the
// validity of an ndt_cluster_spec and the launch plans.  The extraction is modelled on pcl::EuclideanClusterExtraction; the
// class is not in the reference and PCL was not at hand, so no bit parity with PCL is claimed: the definitions in
// include/ndt_mi355.h are the contract.
#pragma once
#include <cmath>
#include <cstddef>

#include "ndt_cloud_ops.hpp"
#include "ndt_mi355.h"

namespace ndt {

constexpr int kClusterTeams = 8;          // queries of one pass of a link block: one wave, eight lanes per query
constexpr int kClusterMaxBlocks = 4096;   // link blocks of one cloud at most: beyond it the blocks stride over the queries
constexpr int kClusterPointBlock = 256;   // threads of a block of the per-point passes (parents, flatten, keys, labels)
constexpr int kClusterPointMaxBlocks = 1024;  // such blocks of one cloud at most: beyond it a block's range grows
constexpr int kClusterInfoBlock = 256;    // threads of the block that reduces one cluster's run of points

// null = a valid spec, else what is wrong with it
inline const char* cluster_spec_error(const ndt_cluster_spec& s) {
  if (!std::isfinite(s.tolerance) || !(s.tolerance > 0.0f)) return "the tolerance must be finite and > 0";
  if (s.min_size < 1) return "min_size must be at least 1";
  if (s.max_size < s.min_size) return "max_size must not be below min_size";
  return nullptr;
}

// The link kernel's grid over a cloud of n points: one wave per block, kClusterTeams queries per pass; a block per pass
// until that would take more than max_blocks, then block b takes the passes b, b + blocks, ...
// *qpb: the queries a block works on at most.  n == 0: no block.
inline void cluster_plan(size_t n, int max_blocks, int* blocks, int* qpb) {
  const size_t passes = (n + kClusterTeams - 1) / kClusterTeams;
  const size_t b = passes < static_cast<size_t>(max_blocks) ? passes : static_cast<size_t>(max_blocks);
  *blocks = static_cast<int>(b);
  *qpb = b ? static_cast<int>((passes + b - 1) / b) * kClusterTeams : 0;
}

// The per-point passes' plan (range_plan): block b owns the points [b * ppb, min(n, (b + 1) * ppb))
inline void cluster_point_plan(size_t n, int* blocks, int* ppb) { range_plan(n, kClusterPointBlock, kClusterPointMaxBlocks, blocks, ppb); }

// The centroid of a cluster of `size` points, a plan that depends on the size alone: thread t of kClusterInfoBlock adds the
// widened coordinates of the run's entries t, t + 256, ... in that order, and block_sum adds the threads in its fixed tree.

}  // namespace ndt
