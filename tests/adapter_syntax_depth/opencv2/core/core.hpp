// OpenCV 3.3 cv::Mat / cv::KeyPoint subset (modules/core/include/opencv2/core/mat.hpp, types.hpp):
// what the depth adapter uses of a CV_64F image and of a keypoint.
#pragma once
#define CV_32F 5
#define CV_64F 6
namespace cv {
class Mat {
 public:
  Mat();
  Mat(int rows, int cols, int type);
  int type() const;
  bool isContinuous() const;
  bool empty() const;
  template <typename T> T *ptr(int i0 = 0);
  template <typename T> const T *ptr(int i0 = 0) const;
  template <typename T> T &at(int row, int col);
  template <typename T> const T &at(int row, int col) const;
  int rows, cols;
};
struct Point2f {
  float x, y;
};
struct Point3f {
  float x, y, z;
};
class KeyPoint {
 public:
  Point2f pt;
  float size, angle, response;
  int octave, class_id;
};
}  // namespace cv
