// ndt_outliers.hpp -- what the host entries and the kernels of the outlier filters (ndt_outliers.hip) share: the validity of
// an ndt_outlier_spec, the block plan of the value kernel and the plan of the statistics.  The filters are modelled on
// pcl::RadiusOutlierRemoval and pcl::StatisticalOutlierRemoval; neither class is in the reference and PCL was not at hand, so
// no bit parity with PCL is claimed: the definitions in include/ndt_mi355.h are the contract.
#pragma once
#include <cmath>
#include <cstddef>

#include "ndt_cloud_ops.hpp"
#include "ndt_mi355.h"

namespace ndt {

constexpr int kOutlierTeams = 8;          // queries of one pass of a block: one wave, eight lanes per query
constexpr int kOutlierMaxBlocks = 4096;   // blocks of one cloud at most: beyond it the blocks stride over the queries
constexpr int kOutlierMaxK = 256;         // mean_k at most (the per-team list lives in LDS)
constexpr int kOutlierStatBlock = 256;    // threads of a block of the statistics
constexpr int kOutlierStatChunk = 4096;   // values of one such block, until ...
constexpr int kOutlierStatMaxBlocks = 256;  // ... that would take more blocks than this

// null = a valid spec, else what is wrong with it
inline const char* outlier_spec_error(const ndt_outlier_spec& s) {
  if (s.method == NDT_OUTLIER_RADIUS) {
    if (!std::isfinite(s.radius) || !(s.radius > 0.0f)) return "the radius must be finite and > 0";
    if (s.min_neighbors < 0) return "min_neighbors must not be negative";
    return nullptr;
  }
  if (s.method == NDT_OUTLIER_STATISTICAL) {
    if (s.mean_k < 1 || s.mean_k > kOutlierMaxK) return "mean_k must be 1 ... 256";
    if (!std::isfinite(s.stddev_mul)) return "stddev_mul must be finite";
    return nullptr;
  }
  return "unknown outlier method";
}

// The value kernel's grid over a cloud of n points: one wave per block, kOutlierTeams queries per pass; a block per pass
// until that would take more than kOutlierMaxBlocks, then block b takes the passes b, b + blocks, ...
// *qpb: the queries a block works on at most.  n == 0: no block.
inline void outlier_plan(size_t n, int* blocks, int* qpb) {
  const size_t passes = (n + kOutlierTeams - 1) / kOutlierTeams;
  const size_t b = passes < static_cast<size_t>(kOutlierMaxBlocks) ? passes : static_cast<size_t>(kOutlierMaxBlocks);
  *blocks = static_cast<int>(b);
  *qpb = b ? static_cast<int>((passes + b - 1) / b) * kOutlierTeams : 0;
}

// The statistics' plan (range_plan), a function of n alone: block b reduces the values [b * chunk, min(n, (b + 1) * chunk)) to
// (count, sum, M2 about its own mean); the rows are merged in block order by Chan's rule.
inline void outlier_stat_plan(size_t n, int* blocks, int* chunk) { range_plan(n, kOutlierStatChunk, kOutlierStatMaxBlocks, blocks, chunk); }

}  // namespace ndt
