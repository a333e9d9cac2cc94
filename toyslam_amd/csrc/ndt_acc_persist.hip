// ndt_acc_persist.hip -- the accumulating target across the boundary of a handle (ndt_target_accumulate_export / _import /
// _save / _load): a voxel leaves or enters as its cell, count and sums -- a row of the blob (include/ndt_mi355.h)
#include <unistd.h>

#include <cerrno>

#include "ndt_acc.hpp"

namespace ndtc {
namespace {

// a whole file into memory / a buffer to a file through a temporary one beside it; "" = done, else the failure
std::string acc_read_file(const char* path, std::vector<unsigned char>& out) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return std::string("cannot open ") + path + ": " + std::strerror(errno);
  unsigned char chunk[1 << 16];
  size_t got;
  while ((got = std::fread(chunk, 1, sizeof(chunk), f)) > 0) out.insert(out.end(), chunk, chunk + got);
  const bool bad = std::ferror(f) != 0;
  const int err = errno;
  std::fclose(f);
  return bad ? std::string("cannot read ") + path + ": " + std::strerror(err) : std::string();
}
std::string acc_write_file(const char* path, const unsigned char* data, size_t bytes) {
  const std::string tmp = std::string(path) + ".tmp" + std::to_string(static_cast<long long>(getpid()));
  FILE* f = std::fopen(tmp.c_str(), "wb");
  if (!f) return std::string("cannot write ") + path + ": " + std::strerror(errno);
  const bool wrote = std::fwrite(data, 1, bytes, f) == bytes;
  int err = errno;
  const bool closed = std::fclose(f) == 0;
  if (wrote && !closed) err = errno;
  if (wrote && closed && std::rename(tmp.c_str(), path) == 0) return std::string();
  if (wrote && closed) err = errno;
  std::remove(tmp.c_str());
  return std::string("cannot write ") + path + ": " + std::strerror(err);
}

}  // namespace
}  // namespace ndtc

extern "C" {

// The bounds as cells; buf == null: only the size (the mark alone).  Else mark, sort of the (key, slot) pairs, gather -- queued
// together -- then ONE read-back (rows, their points, their cell box) and the copy of the rows; the host writes the header and
// the checksum.  Nothing of the target is written
ndt_status ndt_target_accumulate_export(ndt_handle h, const float* min_xyz, const float* max_xyz, void* buf, size_t capacity, size_t* bytes) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (!bytes) return fail(NDT_ERR_INVALID, "null bytes");
  if ((min_xyz == nullptr) != (max_xyz == nullptr)) return fail(NDT_ERR_INVALID, "one bound of the export box is null: give both, or neither for every voxel");
  AccTarget* a = nullptr;
  ndt::AccCropBox box;
  ndt_status s = acc_box_of_bounds(h, min_xyz, max_xyz, "no accumulated target to export", &a, &box);
  if (!s && a->n_slots) s = ensure_device(h);
  if (s) return s;
  h->exp_voxels = h->exp_points = h->exp_launches = 0;
  hipStream_t st = h->stream;
  const int n_slots = a->n_slots;
  AccInfo seen = {};  // (no voxel: the header alone, zeros for its box, nothing queued)
  DevBuf<ndt::AccRow> rows;
  if (n_slots) {
    DevBuf<unsigned> keep;
    DevBuf<int> info;
    HIP_TRY(keep.reserve(static_cast<size_t>(n_slots)));
    if (buf) HIP_TRY(rows.reserve(static_cast<size_t>(n_slots)));
    HIP_TRY(acc_info_reset(info, st));
    HIP_TRY(ndt::launch_acc_mark(a->view(), n_slots, box, keep.p, info.p, nullptr, rows.p, st));
    h->exp_launches = buf ? 3 : 1;
    HIP_TRY(acc_info_read(info, st, &seen));  // ---- the one read-back
  }
  const int n = seen.word6;
  if (n < 0 || n > n_slots) return fail(NDT_ERR_HIP, "export: the row count is out of range");
  const size_t payload = static_cast<size_t>(n) * ndtc::kAccBlobRowBytes, need = ndtc::kAccBlobHeaderBytes + payload;
  if (buf) {
    if (capacity < need) return fail(NDT_ERR_INVALID, "the export buffer is too small for the blob");
    unsigned char* out = static_cast<unsigned char*>(buf);
    if (n) {
      HIP_TRY(hipMemcpyAsync(out + ndtc::kAccBlobHeaderBytes, rows.p, payload, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
    acc_blob_write_header(out, a->resolution, static_cast<uint64_t>(n), seen.lo, seen.hi, out + ndtc::kAccBlobHeaderBytes);
  }
  *bytes = need;
  h->exp_voxels = static_cast<size_t>(n);
  h->exp_points = static_cast<size_t>(seen.points);
  return NDT_OK;
}

// An accumulate call whose input is voxels.  Upload, ONE check launch over the rows, ONE read-back, the refusals; then growth
// and relink as an update, the rows placed behind the existing slots and finished (acc_commit)
ndt_status ndt_target_accumulate_import(ndt_handle h, const void* blob, size_t bytes) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  ndtc::AccBlobHeader hd;
  if (const char* why = acc_blob_parse(blob, bytes, &hd)) return fail(NDT_ERR_INVALID, why);
  AccTarget* a = acc_live(h);
  const float resolution = a ? a->resolution : h->resolution;
  if (std::memcmp(&hd.resolution, &resolution, sizeof(float)) != 0)
    return fail(NDT_ERR_INVALID, "the blob's resolution is not the resolution of the target it is imported into");
  if (static_cast<unsigned long long>(a ? a->n_slots : 0) + hd.n_voxels > (1ull << 30)) return fail(NDT_ERR_INVALID, "too many voxels in the accumulated target");
  if (hd.n_voxels == 0) return NDT_OK;
  ndt_status s = ensure_device(h);
  if (s) return s;
  hipStream_t st = h->stream;
  std::shared_ptr<AccTarget> started;
  a = acc_begin(h, started);
  const int n = static_cast<int>(hd.n_voxels);
  const size_t N = static_cast<size_t>(n);
  DevBuf<ndt::AccRow> rows;
  DevBuf<int> info;
  HIP_TRY(rows.reserve(N));
  HIP_TRY(acc_info_reset(info, st));
  HIP_TRY(hipMemcpyAsync(rows.p, static_cast<const unsigned char*>(blob) + ndtc::kAccBlobHeaderBytes, N * sizeof(ndt::AccRow), hipMemcpyHostToDevice, st));
  ndt::AccCropBox box;
  std::memcpy(box.lo, hd.lo, sizeof(box.lo));
  std::memcpy(box.hi, hd.hi, sizeof(box.hi));
  HIP_TRY(ndt::launch_acc_import_check(rows.p, n, box, a->view(), info.p, st));
  h->acc_launches++;
  // ---- the one read-back (the blob is the caller's pageable memory: the copy has read it by then)
  AccInfo seen;
  HIP_TRY(acc_info_read(info, st, &seen));
  // ---- refusals: nothing of the target has been written so far
  const int flags = seen.word6;
  if (flags & ndt::kAccRowOutside) return fail(NDT_ERR_INVALID, "a row of the blob lies outside the cell box of its header");
  if (flags & ndt::kAccRowCount) return fail(NDT_ERR_INVALID, "a row of the blob has a count below 1");
  if (flags & ndt::kAccRowNonFinite) return fail(NDT_ERR_INVALID, "a row of the blob holds a non-finite sum");
  if (flags & ndt::kAccRowOrder) return fail(NDT_ERR_INVALID, "the rows of the blob are not in strictly ascending key order");
  for (int k = 0; k < 3; k++)
    if (seen.lo[k] != hd.lo[k] || seen.hi[k] != hd.hi[k]) return fail(NDT_ERR_INVALID, "the header's cell box is not the tight box of the blob's rows");
  if (flags & ndt::kAccRowPresent) return fail(NDT_ERR_INVALID, "cell already in the target: a blob's cells must be absent from the target it is imported into");
  // ---- the box: the union with the centres of the blob's corner cells, the float a cropped target carries
  ndt::AccPlan plan;
  plan.rows = rows.p;
  plan.n_touched = plan.n_new = n;
  plan.n_points = a->n_points + static_cast<size_t>(seen.points);
  acc_box_of_cells(a, hd.lo, hd.hi, true, plan.mn, plan.mx);
  return acc_commit(h, a, started, plan);
}

ndt_status ndt_target_accumulate_save(ndt_handle h, const float* min_xyz, const float* max_xyz, const char* path) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (!path) return fail(NDT_ERR_INVALID, "null path");
  const AccTarget* a = acc_live(h);
  // room for every voxel: one export, whatever the box selects
  std::vector<unsigned char> blob(ndtc::kAccBlobHeaderBytes + (a ? static_cast<size_t>(a->n_slots) : 0) * ndtc::kAccBlobRowBytes);
  size_t bytes = 0;
  ndt_status s = ndt_target_accumulate_export(h, min_xyz, max_xyz, blob.data(), blob.size(), &bytes);
  if (s) return s;
  const std::string err = acc_write_file(path, blob.data(), bytes);
  if (!err.empty()) return fail(NDT_ERR_INVALID, err);
  return NDT_OK;
}
ndt_status ndt_target_accumulate_load(ndt_handle h, const char* path) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (!path) return fail(NDT_ERR_INVALID, "null path");
  std::vector<unsigned char> blob;
  const std::string err = acc_read_file(path, blob);
  if (!err.empty()) return fail(NDT_ERR_INVALID, err);
  return ndt_target_accumulate_import(h, blob.data(), blob.size());
}
ndt_status ndt_diag_target_export(ndt_handle h, size_t* voxels, size_t* points, size_t* launches) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (voxels) *voxels = h->exp_voxels;
  if (points) *points = h->exp_points;
  if (launches) *launches = h->exp_launches;
  return NDT_OK;
}
ndt_status ndt_host_acc_blob_info(const void* blob, size_t bytes, float* resolution, size_t* n_voxels, int* lo, int* hi) {
  ndtc::AccBlobHeader hd;
  if (const char* why = acc_blob_parse(blob, bytes, &hd)) return fail(NDT_ERR_INVALID, why);
  if (resolution) *resolution = hd.resolution;
  if (n_voxels) *n_voxels = static_cast<size_t>(hd.n_voxels);
  for (int k = 0; k < 3; k++) {
    if (lo) lo[k] = hd.lo[k];
    if (hi) hi[k] = hd.hi[k];
  }
  return NDT_OK;
}
ndt_status ndt_host_acc_blob_checksum(const void* data, size_t bytes, uint64_t* out) {
  if (!out) return fail(NDT_ERR_INVALID, "null out");
  if (bytes && !data) return fail(NDT_ERR_INVALID, "null data");
  if (bytes % 8) return fail(NDT_ERR_INVALID, "the checksum runs over 8-byte words: bytes must be a multiple of 8");
  *out = acc_blob_hash(ndtc::kAccBlobHashSeed, data, bytes);
  return NDT_OK;
}

ndt_status ndt_host_acc_pack_cell(int i, int j, int k, uint64_t* key) {
  const int lim = ndt::kAccCellBias;
  if (!key) return fail(NDT_ERR_INVALID, "null key");
  if (i < -lim || i >= lim || j < -lim || j >= lim || k < -lim || k >= lim)
    return fail(NDT_ERR_INVALID, "cell indices must be within [-2^20, 2^20) on every axis");
  *key = ndt::acc_pack(i, j, k);
  return NDT_OK;
}
void ndt_host_acc_unpack_cell(uint64_t key, int* i, int* j, int* k) { ndt::acc_unpack(key, *i, *j, *k); }

}  // extern "C"
