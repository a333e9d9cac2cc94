// ndt_deskew.hip -- motion compensation of resident scans by the time of every point (ndt_cloud_deskew,
// ndt_cloud_deskew_clouds; the per-point body is ndt_deskew.hpp): every record of a cloud is moved by a rigid motion of its
// own -- the sensor's pose at the point's time, seen from its pose at t_ref -- in ONE launch whatever the number of clouds.
//   plan   : every cloud gets blocks of its own (deskew_plan: 256 threads, one contiguous range of points_per_block points
//            per block, at most 1024 blocks per cloud); a call is a table of segments (cloud -> first block, points, motion),
//            and a block finds its segment by bisection.  A block never spans two clouds.  A call of one cloud hands its
//            segment (the motion with it) over as a kernel argument.
//   point  : one 16-byte record load and one 8-byte time load, the f64 body, one 16-byte store; both boxes are folded in
//            registers from the f32 values that were stored, as k_select_place folds them.
//   block  : wave folds, then one row of 12 floats and the untimed count, written straight into page-locked memory and read
//            behind the call's one wait; the host folds the rows.  No global atomics, no second pass.
// The rest of the file is host only: the motion of a sweep from a registration increment (ndt_host_deskew_motion), the body for
// one point and the plan.  The entries that fetch the per-point times are in ndt_io.hip.  The member table, the box fold
// (device and host), the output slices and the entry preambles are ndt_cloud_ops.hpp / .hip's.
#include "ndt_internal.hpp"
#include "ndt_deskew.hpp"
#include "ndt_device.hpp"

namespace ndtc {
namespace {

constexpr int kDskBlock = ndt::kDeskewBlock;
constexpr int kDskWaves = kDskBlock / 64;
constexpr int kDskRow = 16;  // words of a block's row: 12 box floats, the untimed count, 3 unused

struct DskSeg {
  const float4* in;
  float4* out;
  const double* times;
  ndt_deskew_motion m;
  int n, ppb;
  int first_block, n_blocks;
};

__global__ __launch_bounds__(kDskBlock) void k_deskew(DskSeg one, const DskSeg* __restrict__ segs, int n_segs, float* __restrict__ rows) {
  __shared__ float wave_box[kDskWaves][12];
  __shared__ unsigned wave_untimed[kDskWaves];
  const DskSeg g = ndt::block_member(one, segs, n_segs, blockIdx.x, &DskSeg::first_block);
  long long start;
  const int len = ndt::block_range(static_cast<int>(blockIdx.x) - g.first_block, g.ppb, g.n, &start);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double dt = g.m.t_end - g.m.t_begin;
  const float4* __restrict__ in = g.in + start;
  float4* __restrict__ out = g.out + start;
  const double* __restrict__ times = g.times + start;
  ndt::TwoBox<kDskWaves> box;  // of the f32 values that were stored
  unsigned untimed = 0;
  for (int i = threadIdx.x; i < len; i += kDskBlock) {
    float4 p = in[i];
    const double t = times[i];
    float q[3];
    const int kind = ndt::deskew_point(g.m, dt, p.x, p.y, p.z, t, q);
    if (kind != 1) {  // (a record with a non-finite coordinate goes out as it came in, bit for bit)
      p.x = q[0];
      p.y = q[1];
      p.z = q[2];
    }
    untimed += kind == 2 ? 1u : 0u;
    out[i] = p;
    box.add(p);
  }
  box.to_lds(wave_box);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) untimed += __shfl_xor(untimed, o);
  if (lane == 0) wave_untimed[wave] = untimed;
  __syncthreads();
  float* row = rows + static_cast<size_t>(blockIdx.x) * kDskRow;
  if (threadIdx.x < 12) {
    row[threadIdx.x] = box.block_value(wave_box, threadIdx.x);
  } else if (threadIdx.x == 12) {
    unsigned u = 0;
    for (int w = 0; w < kDskWaves; w++) u += wave_untimed[w];
    reinterpret_cast<unsigned*>(row)[12] = u;
  }
}

int max_blocks_switch() {  // development switch, read once: small values reach the strided regime with small clouds
  static const int v = env_block_cap("NDT_DESKEW_MAX_BLOCKS", ndt::kDeskewMaxBlocks);
  return v;
}

// One cloud of a call: n records at `in` with their n device times, the moved records to `out` (room for n); results: the
// untimed count, and n, the boxes and the route in `res`.
struct DskJob {
  const float4* in = nullptr;
  size_t n = 0;
  const double* times = nullptr;
  const ndt_deskew_motion* m = nullptr;
  float4* out = nullptr;
  size_t untimed = 0;
  DeviceCloud* res = nullptr;
};

// the one launch over all jobs and the call's one wait
ndt_status deskew_run(ndt_handle h, std::vector<DskJob>& jobs) {
  hipStream_t st = h->stream;
  h->dsk_launches = h->dsk_blocks = 0;
  h->dsk_clouds = jobs.size();
  MemberTable<DskSeg> segs;
  std::vector<size_t> slot;
  long long total_blocks = 0;
  for (size_t k = 0; k < jobs.size(); k++) {
    DskJob& j = jobs[k];
    j.untimed = 0;
    if (j.res) j.res->n = j.n;
    if (j.n == 0) continue;
    DskSeg g{};
    int blocks = 0, ppb = 0;
    ndt::deskew_plan(j.n, max_blocks_switch(), &blocks, &ppb);
    g.in = j.in;
    g.out = j.out;
    g.times = j.times;
    g.m = *j.m;
    g.n = static_cast<int>(j.n);
    g.ppb = ppb;
    g.first_block = static_cast<int>(total_blocks);
    g.n_blocks = blocks;
    segs.host.push_back(g);
    slot.push_back(k);
    total_blocks += blocks;
  }
  if (segs.host.empty()) return NDT_OK;
  if (total_blocks > std::numeric_limits<int>::max()) return fail(NDT_ERR_INVALID, "too many points");
  const size_t nb = static_cast<size_t>(total_blocks);
  // page-locked: [segment table | rows, one per block]
  const size_t seg_bytes = (segs.bytes() + 15) / 16 * 16;
  const size_t row_bytes = nb * kDskRow * sizeof(float);
  ndt_status s = pinned_at_least(h->dsk_pinned, h->dsk_pinned_bytes, seg_bytes + row_bytes, st);
  if (s) return s;
  unsigned char* pin = static_cast<unsigned char*>(h->dsk_pinned);
  float* rows = reinterpret_cast<float*>(pin + seg_bytes);
  std::memcpy(pin, segs.host.data(), segs.bytes());
  if ((s = segs.upload(st, pin))) return s;
  hipLaunchKernelGGL(k_deskew, dim3(static_cast<unsigned>(nb)), dim3(kDskBlock), 0, st, segs.one(), segs.table(), segs.n(), rows);
  HIP_TRY(hipGetLastError());
  h->dsk_launches = 1;
  h->dsk_blocks = nb;
  HIP_TRY(hipStreamSynchronize(st));
  for (size_t q = 0; q < segs.host.size(); q++) {
    const DskSeg& g = segs.host[q];
    DskJob& j = jobs[slot[q]];
    for (int b = g.first_block; b < g.first_block + g.n_blocks; b++) {
      unsigned u;
      std::memcpy(&u, rows + static_cast<size_t>(b) * kDskRow + 12, sizeof u);
      j.untimed += u;
    }
    if (j.res) fold_box_rows(j.res, rows, kDskRow, g.first_block, g.n_blocks, NDT_BOX_ROUTE_DESKEW);
  }
  return NDT_OK;
}

ndt_status motion_checks(const ndt_deskew_motion* m) { return spec_checks(m, ndt::deskew_motion_error, "null motion"); }

// Rodrigues' formula: Exp(angle * k) v, in f64
void rotate_about(const double k[3], double angle, const double v[3], double out[3]) {
  const double sn = std::sin(angle), cs = std::cos(angle);
  const double kxv[3] = {k[1] * v[2] - k[2] * v[1], k[2] * v[0] - k[0] * v[2], k[0] * v[1] - k[1] * v[0]};
  const double kv = k[0] * v[0] + k[1] * v[1] + k[2] * v[2];
  for (int a = 0; a < 3; a++) out[a] = v[a] * cs + kxv[a] * sn + k[a] * kv * (1.0 - cs);
}

}  // namespace
}  // namespace ndtc

extern "C" {

ndt_status ndt_cloud_deskew(ndt_handle h, ndt_cloud in, const ndt_deskew_motion* motion, const double* times, int times_on_device,
                            ndt_cloud* out, size_t* n_untimed) {
  if (out) *out = nullptr;
  if (!h || !out) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = cloud_entry(h, in, [&]() -> ndt_status {
    if (ndt_status e = motion_checks(motion)) return e;
    if (in->c->n && !times) return fail(NDT_ERR_INVALID, "a deskew needs the points' times");
    return NDT_OK;
  });
  if (s) return s;
  const size_t n = in->c->n;
  DevBuf<double> d_times;
  const double* tp = times;
  auto c = new_cloud(h);
  if (n) HIP_TRY(c->pts.reserve(n));  // (before anything is queued: a failure gives back what was reserved, and nothing uses it)
  Drain drain{h->stream};             // (from here on nothing queued may still read or write what goes back to the pool)
  if ((s = doubles_in(h->stream, times, n, times_on_device, d_times, &tp))) return s;
  std::vector<DskJob> jobs(1);
  jobs[0].in = in->c->pts.p;
  jobs[0].n = n;
  jobs[0].times = tp;
  jobs[0].m = motion;
  jobs[0].out = c->pts.p;
  jobs[0].res = c.get();
  if ((s = deskew_run(h, jobs))) return s;
  drain.done = true;  // (the run has waited)
  if (n_untimed) *n_untimed = jobs[0].untimed;
  *out = new ndt_cloud_s{c};
  return NDT_OK;
}

ndt_status ndt_cloud_deskew_clouds(ndt_handle h, const ndt_cloud* in, size_t n_clouds, const ndt_deskew_motion* motions, const double* times,
                                   int times_on_device, ndt_cloud* out, size_t* n_untimed) {
  if (!h || !out) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = clouds_begin(n_clouds, out);
  if (s) return s;
  if (n_clouds && !in) return fail(NDT_ERR_INVALID, "null clouds");
  if (n_clouds && !motions) return fail(NDT_ERR_INVALID, "null motion");
  std::vector<size_t> first;
  if ((s = clouds_total(h, in, n_clouds, first, [&](size_t k) { return motion_checks(&motions[k]); }))) return s;
  const size_t total = first[n_clouds];
  if (total && !times) return fail(NDT_ERR_INVALID, "a deskew needs the points' times");
  if (n_clouds == 0) return NDT_OK;
  s = ensure_device(h);
  if (s) return s;
  OutSlices outs;
  std::vector<DskJob> jobs(n_clouds);
  DevBuf<double> d_times;
  const double* tp = times;
  if ((s = outs.reserve(h, first))) return s;  // (before anything is queued)
  Drain drain{h->stream};  // (from here on nothing queued may still read or write what goes back to the pool)
  if ((s = doubles_in(h->stream, times, total, times_on_device, d_times, &tp))) return s;
  for (size_t k = 0; k < n_clouds; k++) {
    DeviceCloud* c = in[k]->c.get();
    if ((s = cloud_use_on(h, c))) return s;
    jobs[k].in = c->pts.p;
    jobs[k].n = c->n;
    jobs[k].times = tp ? tp + first[k] : nullptr;
    jobs[k].m = &motions[k];
    jobs[k].out = outs.at(k);
    jobs[k].res = outs.cloud(k);
  }
  if ((s = deskew_run(h, jobs))) return s;
  drain.done = true;  // (the run has waited)
  for (size_t k = 0; k < n_clouds; k++) {
    out[k] = outs.publish(k, jobs[k].n);
    if (n_untimed) n_untimed[k] = jobs[k].untimed;
  }
  return NDT_OK;
}

ndt_status ndt_diag_deskew(ndt_handle h, size_t* launches, size_t* blocks, size_t* clouds) {
  if (!h || !launches || !blocks || !clouds) return fail(NDT_ERR_INVALID, "bad arguments");
  *launches = h->dsk_launches;
  *blocks = h->dsk_blocks;
  *clouds = h->dsk_clouds;
  return NDT_OK;
}

ndt_status ndt_host_deskew_motion(const float* T, double t_begin, double t_end, double t_ref, ndt_deskew_motion* out) {
  if (!T || !out) return fail(NDT_ERR_INVALID, "bad arguments");
  for (int i = 0; i < 16; i++)
    if (!std::isfinite(T[i])) return fail(NDT_ERR_INVALID, "the transformation must be finite");
  if (!std::isfinite(t_begin) || !std::isfinite(t_end) || !std::isfinite(t_ref)) return fail(NDT_ERR_INVALID, "the times must be finite");
  if (!(t_end > t_begin)) return fail(NDT_ERR_INVALID, "a motion needs t_end > t_begin");
  double R[3][3];  // R[row][column] of the column-major T
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) R[r][c] = static_cast<double>(T[4 * c + r]);
  const double tau[3] = {static_cast<double>(T[12]), static_cast<double>(T[13]), static_cast<double>(T[14])};
  // the logarithm: v = sin(angle) * axis from the antisymmetric part, cos(angle) from the trace
  const double v[3] = {0.5 * (R[2][1] - R[1][2]), 0.5 * (R[0][2] - R[2][0]), 0.5 * (R[1][0] - R[0][1])};
  const double sn = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  const double cs = 0.5 * (R[0][0] + R[1][1] + R[2][2] - 1.0);
  ndt_deskew_motion m{};
  m.t_begin = t_begin;
  m.t_end = t_end;
  m.t_ref = t_ref;
  m.angle = std::atan2(sn, cs);
  double k[3] = {1.0, 0.0, 0.0};
  if (m.angle == 0.0) {
    // the identity (or nothing the f32 matrix can tell from it)
  } else if (cs >= 0.0) {
    for (int a = 0; a < 3; a++) k[a] = v[a] / sn;
  } else {
    // beyond a quarter turn the antisymmetric part shrinks towards nothing at pi while the symmetric part
    // (R + R^T)/2 = cos I + (1 - cos) k k^T grows: k from its largest diagonal entry and that row, the sign from v
    double S[3][3];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) S[r][c] = (0.5 * (R[r][c] + R[c][r]) - (r == c ? cs : 0.0)) / (1.0 - cs);
    int b = 0;
    for (int a = 1; a < 3; a++)
      if (S[a][a] > S[b][b]) b = a;
    const double kb = std::sqrt(std::max(S[b][b], 0.0));
    if (kb > 0.0) {
      for (int a = 0; a < 3; a++) k[a] = a == b ? kb : S[b][a] / kb;
      if (v[b] < 0.0)
        for (int a = 0; a < 3; a++) k[a] = -k[a];
    }
  }
  const double len = std::sqrt(k[0] * k[0] + k[1] * k[1] + k[2] * k[2]);
  for (int a = 0; a < 3; a++) m.axis[a] = k[a] / len;
  const double u_ref = (t_ref - t_begin) / (t_end - t_begin);
  rotate_about(m.axis, -u_ref * m.angle, tau, m.tau_ref);
  if (const char* why = ndt::deskew_motion_error(m)) return fail(NDT_ERR_INVALID, why);
  *out = m;
  return NDT_OK;
}

ndt_status ndt_host_deskew_point(const ndt_deskew_motion* motion, const float* xyz, double t, float* out, int* untimed) {
  if (!xyz || !out) return fail(NDT_ERR_INVALID, "bad arguments");
  if (ndt_status s = motion_checks(motion)) return s;
  const int kind = ndt::deskew_point(*motion, motion->t_end - motion->t_begin, xyz[0], xyz[1], xyz[2], t, out);
  if (untimed) *untimed = kind == 2 ? 1 : 0;
  return NDT_OK;
}

ndt_status ndt_host_deskew_plan(size_t n_points, int* blocks, int* points_per_block) {
  if (!blocks || !points_per_block) return fail(NDT_ERR_INVALID, "bad arguments");
  if (n_points > static_cast<size_t>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, "too many points");
  ndt::deskew_plan(n_points, max_blocks_switch(), blocks, points_per_block);
  return NDT_OK;
}

}  // extern "C"
