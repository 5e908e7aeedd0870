// corner_check — the host text of the LiDAR flat- and corner-feature extraction
// (csrc/lidar_feat_host.h over lidar_feat_dev.h and lidar_corner_dev.h) in a
// stand-alone program: plain g++, neither HIP nor libsqrtlm.so, so that it can be
// built with -fsanitize=address,undefined
// (tests/test_lidar_corner_host_checked.py). Every array is a heap block of
// exactly the size the interface promises, so an access out of bounds is an error
// the sanitizer reports.
//
//   corner_check IN OUT
//
// IN  (little endian): int32 row_num, col_num, num_scan_subregions,
//     num_curvature_regions_flat, num_curvature_regions_corner, max_surf_flat,
//     max_surf_less_flat, max_corner_sharp, max_corner_less_sharp, n, has_ext;
//     double surf_curv_th, max_sq_dis, deg_diff, sharp_curv_th, ground_z_bound,
//     extrinsic[16]; uint8 ring_enabled[128], corner_ring_enabled[128];
//     float xyz[n][3]. One sweep.
// OUT: int32 status; then, when status is 0, every output and state array at its
//     full promised size, S = row_num, C = col_num: int64 flat_off[2],
//     less_off[2], sharp_off[2], less_sharp_off[2]; float flat_xyz[n][3],
//     flat_normal[n][3], less_xyz[n][3], less_normal[n][3]; int32 less_rc[n][2];
//     float sharp_xyz[n][3], less_sharp_xyz[n][3]; int32 less_sharp_label[n],
//     less_sharp_rc[n][2]; int64 scan_off[S + 1]; int32 cell_state[S][C];
//     uint8 mask[n]; float curvature[n]; int32 sorted[n]; uint8 reason[n],
//     edge[S][C]; float angle[S][C][6].
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../sqrtlm-slam_amd/csrc/lidar_feat_host.h"

namespace {

template <class T>
std::unique_ptr<T[]> block(size_t n) {
  return std::unique_ptr<T[]>(new T[n]());
}

template <class T>
bool get(FILE *f, T *p, size_t n) {
  return n == 0 || std::fread(p, sizeof(T), n, f) == n;
}

template <class T>
bool put(FILE *f, const T *p, size_t n) {
  return n == 0 || std::fwrite(p, sizeof(T), n, f) == n;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: corner_check IN OUT\n");
    return 2;
  }
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) {
    std::perror(argv[1]);
    return 2;
  }
  int32_t h[11];
  double dv[5], ext[16];
  sqlm_lidar_feat_params prm;
  sqlm_lidar_corner_params cp;
  if (!get(in, h, 11) || !get(in, dv, 5) || !get(in, ext, 16) || !get(in, prm.ring_enabled, SQLM_LF_MAX_ROWS) ||
      !get(in, cp.corner_ring_enabled, SQLM_LF_MAX_ROWS) || h[9] < 0) {
    std::fprintf(stderr, "corner_check: short or bad header\n");
    return 2;
  }
  prm.row_num = h[0];
  prm.col_num = h[1];
  prm.num_scan_subregions = h[2];
  prm.num_curvature_regions_flat = h[3];
  prm.num_curvature_regions_corner = h[4];
  prm.max_surf_flat = h[5];
  prm.max_surf_less_flat = h[6];
  prm.using_sharp_point = 1;
  prm.surf_curv_th = dv[0];
  prm.max_sq_dis = dv[1];
  prm.deg_diff = dv[2];
  cp.max_corner_sharp = h[7];
  cp.max_corner_less_sharp = h[8];
  cp.sharp_curv_th = dv[3];
  cp.ground_z_bound = dv[4];
  const size_t n = (size_t)h[9];
  const bool has_ext = h[10] != 0;
  auto xyz = block<float>(3 * n);
  if (!get(in, xyz.get(), 3 * n)) {
    std::fprintf(stderr, "corner_check: short input\n");
    return 2;
  }
  std::fclose(in);
  const int64_t soff[2] = {0, (int64_t)n};
  auto flat_off = block<int64_t>(2), less_off = block<int64_t>(2), sharp_off = block<int64_t>(2), lsharp_off = block<int64_t>(2);
  auto flat_xyz = block<float>(3 * n), flat_nrm = block<float>(3 * n), less_xyz = block<float>(3 * n),
       less_nrm = block<float>(3 * n), sharp_xyz = block<float>(3 * n), lsharp_xyz = block<float>(3 * n);
  auto less_rc = block<int32_t>(2 * n), lsharp_label = block<int32_t>(n), lsharp_rc = block<int32_t>(2 * n);
  const void *fouts[7] = {flat_off.get(), less_off.get(), flat_xyz.get(), flat_nrm.get(),
                          less_xyz.get(), less_nrm.get(), less_rc.get()};
  const void *couts[6] = {sharp_off.get(), sharp_xyz.get(), lsharp_off.get(), lsharp_xyz.get(), lsharp_label.get(),
                          lsharp_rc.get()};
  sqlm::LfParams p;
  sqlm::LcParams q;
  int32_t status = sqlm::lf_check(1, soff, xyz.get(), &prm, fouts, 7, &p, true);
  if (status == SQLM_OK) status = sqlm::lc_check((int64_t)n, &prm, &cp, couts, 6, &q);
  FILE *out = std::fopen(argv[2], "wb");
  if (!out) {
    std::perror(argv[2]);
    return 2;
  }
  bool ok = put(out, &status, 1);
  int64_t picked = 0;
  if (status == SQLM_OK) {
    const size_t S = (size_t)prm.row_num, cells = S * (size_t)prm.col_num;
    auto scan_off = block<int64_t>(S + 1);
    auto cell_state = block<int32_t>(cells), sorted = block<int32_t>(n);
    auto mask = block<uint8_t>(n), reason = block<uint8_t>(n), edge = block<uint8_t>(cells);
    auto curv = block<float>(n), angle = block<float>(cells * sqlm::kLcOffsets);
    sqlm_lidar_feat_state fs = {};
    fs.scan_off = scan_off.get();
    sqlm_lidar_corner_state cs = {cell_state.get(), mask.get(), curv.get(), sorted.get(), reason.get(), edge.get(),
                                  angle.get()};
    const sqlm::LcOut co{sharp_off.get(), lsharp_off.get(), sharp_xyz.get(), lsharp_xyz.get(), lsharp_label.get(),
                         lsharp_rc.get()};
    status = sqlm::lf_host(1, soff, xyz.get(), p, has_ext ? ext : nullptr, true, flat_off.get(), flat_xyz.get(),
                           flat_nrm.get(), less_off.get(), less_xyz.get(), less_nrm.get(), less_rc.get(), &fs, &q, co, &cs);
    picked = lsharp_off[1];
    ok = ok && put(out, flat_off.get(), 2) && put(out, less_off.get(), 2) && put(out, sharp_off.get(), 2) &&
         put(out, lsharp_off.get(), 2) && put(out, flat_xyz.get(), 3 * n) && put(out, flat_nrm.get(), 3 * n) &&
         put(out, less_xyz.get(), 3 * n) && put(out, less_nrm.get(), 3 * n) && put(out, less_rc.get(), 2 * n) &&
         put(out, sharp_xyz.get(), 3 * n) && put(out, lsharp_xyz.get(), 3 * n) && put(out, lsharp_label.get(), n) &&
         put(out, lsharp_rc.get(), 2 * n) && put(out, scan_off.get(), S + 1) && put(out, cell_state.get(), cells) &&
         put(out, mask.get(), n) && put(out, curv.get(), n) && put(out, sorted.get(), n) && put(out, reason.get(), n) &&
         put(out, edge.get(), cells) && put(out, angle.get(), cells * sqlm::kLcOffsets);
  }
  if (std::fclose(out) != 0 || !ok) {
    std::fprintf(stderr, "corner_check: write failed\n");
    return 2;
  }
  std::printf("ok status %d points %zu less_sharp %lld\n", status, n, (long long)picked);
  return 0;
}
