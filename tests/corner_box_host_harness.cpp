// Compiles the PRODUCT's corner-box arithmetic (automatic-as-built-reconstruction_amd/csrc/corner_box.h) for the host, so
// that the exact statement sequence the HIP kernels run can be compared with the reference's vectors on the CPU and,
// bit for bit, with the list kernels on the GPU.
#include <stdint.h>
#include "../automatic-as-built-reconstruction_amd/csrc/corner_box.h"
extern "C" void host_box_to_2corners(const float *boxes, int64_t n, float *out) {
  for (int64_t i = 0; i < n; ++i) aabr::yxzb_to_2corners(boxes + 7 * i, out + 7 * i);
}
extern "C" void host_box_from_2corners(const float *corners, int64_t n, float *out) {
  for (int64_t i = 0; i < n; ++i) aabr::corners_to_yxzb(corners + 7 * i, out + 7 * i);
}
extern "C" void host_box_encode_corner(const float *targets, const float *anchors, int64_t n, const float *w, float *out) {
  for (int64_t i = 0; i < n; ++i) aabr::box_encode7_corner(targets + 7 * i, anchors + 7 * i, w, out + 7 * i);
}
extern "C" void host_box_decode_corner(const float *enc, const float *anchors, int64_t n, int nc, const float *w,
                                       float clip, float *out) {
  for (int64_t i = 0; i < n * nc; ++i) aabr::box_decode7_corner(enc + 7 * i, anchors + 7 * (i / nc), w, clip, out + 7 * i);
}
