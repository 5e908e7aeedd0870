// include/utils/lidarconfig.h:13-58 (the fields of the flat-point path and of the corner branch; defaults as there).
#pragma once
struct lidarConfig {
  int sensor_type = 64;
  double deg_diff = 0.2;
  int lower_ring_num_z_trans = 5;
  int upper_ring_num_z_trans = 50;
  int lower_ring_num_x_rot = 5;
  int upper_ring_num_x_rot = 50;
  int lower_ring_num_y_rot = 5;
  int upper_ring_num_y_rot = 50;
  int lower_ring_num_z_rot_xy_trans = 5;
  int upper_ring_num_z_rot_xy_trans = 50;
  int num_scan_subregions = 8;
  int num_curvature_regions_corner = 3;
  int num_curvature_regions_flat = 5;
  double surf_curv_th = 0.001;
  int max_surf_flat = 2;
  int max_surf_less_flat = 6;
  double max_sq_dis = 1;
  double ground_z_bound = -1.5;
  int lower_ring_num_sharp_point = 1;
  int upper_ring_num_sharp_point = 40;
  double sharp_curv_th = 20;
  int max_corner_sharp = 3;
  int max_corner_less_sharp = 8;
  bool using_sharp_point = true;
  bool using_flat_point = true;
  int row_num_ = sensor_type, col_num_ = 360.0 / deg_diff;
};
