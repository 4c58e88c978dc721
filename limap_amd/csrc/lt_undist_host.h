// lt_undist_host.h -- what the device entry points (lt_undist.cpp) and the host-only entry points (lt_undist_host.cpp)
// of the undistortion share on the host: the validated camera table and image table.  lt_undist_host.cpp links
// without the device side (tools/undist_host_asan.cpp builds it into a sanitizer program of its own).
#pragma once

#include "../../include/limap_amd.h"
#include "lt_undist.h"

#include <cstdint>
#include <string>
#include <vector>

namespace lt_impl {

// validates the cameras and brings them into the table's form; 0, or 1 with msg set
int ud_prepare_cams(int n_cam, const lt_undist_camera *cams, std::vector<lt::UdCam> &out, std::string &msg);

struct UdBatch {
  std::vector<lt::UdImage> imgs;  // offsets not set
  long long n_units = 0;
  int on_device = 0;              // of every image of the batch
};

// validates the images of a warp batch against the camera table and lays out its work units; 0, or 1 with msg set
int ud_prepare_images(const std::vector<lt::UdCam> &cams, int n_img, const lt_undist_image *imgs, UdBatch &out,
                      std::string &msg);

// validates the points' camera indices; 0, or 1 with msg set
int ud_check_points(int n_cam, int64_t n, const double *xy, const int32_t *cam_src, const int32_t *cam_dst,
                    const double *out_xy, const int32_t *status, const int32_t *iters, std::string &msg);

}  // namespace lt_impl
