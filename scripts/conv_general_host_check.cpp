// Host side of csrc/conv_general.hip (descriptor checks, _supported, _out_shape, _sizes and the weight-gradient plan of all three headers) as a stand-alone program for
// AddressSanitizer / UndefinedBehaviorSanitizer: the row list of tests/conv_general_cases.py, FlowNet's classes, the invalid descriptors
// and descriptors at the ends of the int range.  No GPU and no Python involved; built and run by scripts/conv_general_host_check.sh.
#include <cstdio>
#include <string>
#include <climits>
#include "flownet2_hip_conv_general.h"
#include "flownet2_hip_conv_geometry.h"
#include "flownet2_hip_conv_volume.h"
namespace fn2 { std::string& last_error() { static std::string s; return s; } int& batch_invariant_flag() { static int f = 0; return f; } }
int main() {
  const int rows[][9] = {
    {0,1,1,5,7,1,1,1,0},{0,2,3,11,13,7,3,1,2},{0,3,5,9,12,33,4,2,1},{0,1,17,23,19,20,11,4,0},{0,2,6,8,8,16,2,3,0},{0,2,40,9,12,33,3,2,2},
    {0,2,64,16,24,96,5,2,2},{0,1,4,3,3,8,5,1,2},{0,1,2,4,4,3,3,1,3},{0,1,8,6,70,4,1,2,0},
    {1,2,5,4,6,3,4,2,1},{1,1,7,5,5,9,3,1,1},{1,2,3,4,5,6,2,2,0},{1,1,6,3,4,5,5,3,2},{1,1,2,6,6,2,3,2,2},
    {0,8,3,320,448,64,7,2,3},{0,8,64,160,224,128,5,2,2},{0,8,256,40,56,256,3,1,1},{0,8,256,40,56,512,3,2,1},{0,8,256,40,56,32,1,1,0},{1,8,1024,5,7,512,4,2,1}};
  const int bad[][9] = {
    {0,1,3,4,4,8,7,1,1},{1,1,3,1,1,8,2,1,1},{0,1,3,8,8,8,0,1,0},{0,1,3,8,8,8,3,0,1},{0,1,3,8,8,8,3,1,-1},{0,1,0,8,8,8,3,1,1},{1,1,3,8,8,0,3,1,1},
    {0,0,3,8,8,8,3,1,1},{0,1,3,1<<20,1<<20,8,3,1,1},{0,INT_MAX,INT_MAX,INT_MAX,INT_MAX,INT_MAX,INT_MAX,1,INT_MAX},{1,INT_MAX,INT_MAX,INT_MAX,INT_MAX,INT_MAX,INT_MAX,INT_MAX,0},
    {0,1,1,INT_MAX,INT_MAX,1,1,1,0},{1,1,1,INT_MAX,1,1,INT_MAX,INT_MAX,0},{0,1,INT_MAX,1,1,INT_MAX,1,1,0},{0,1,1,1,1,1,46341,1,INT_MAX/2}};
  int fails = 0;
  for (auto& r : rows) {
    fn2_conv_desc d{r[1],r[2],r[3],r[4],r[5],r[6],r[7],r[8]};
    size_t a=0,b=0,c=1,w=0;
    if (fn2_conv_general_supported(&d, r[0]) != 1 || fn2_conv_general_sizes(&d, r[0], &a, &b, &c, &w) != 0 || !a || !b || c || !w) { printf("row refused\n"); ++fails; }
    else printf("ok %zu %zu %zu\n", a, b, w);
  }
  for (auto& r : bad) {
    fn2_conv_desc d{r[1],r[2],r[3],r[4],r[5],r[6],r[7],r[8]};
    size_t a=1,b=1,c=1,w=1;
    if (fn2_conv_general_supported(&d, r[0]) != 0 || fn2_conv_general_sizes(&d, r[0], &a, &b, &c, &w) != FN2_ERR_UNSUPPORTED || a || b || c || w) { printf("bad accepted %d %d\n", r[1], r[6]); ++fails; }
  }
  // the 14-int geometries of include/flownet2_hip_conv_geometry.h: {transposed, N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, group}: rows of
  // tests/conv_geometry_cases.py, its invalid list, and values at the ends of the int range in every field
  const int M = INT_MAX;
  const int grows[][15] = {
    {0,2,3,6,11,5,1,7,1,1,0,3,1,1,1},{0,2,4,12,9,20,3,3,2,2,1,1,3,1,1},{0,1,2,4,4,3,3,3,1,1,4,4,4,4,1},{0,2,19,8,9,19,3,3,1,1,1,1,1,1,19},
    {0,2,6,11,14,9,2,3,2,1,1,2,2,3,3},{1,2,5,4,6,3,4,2,2,1,1,0,1,1,1},{1,1,6,3,4,9,3,2,3,2,0,1,1,2,3},{1,1,5,4,4,5,4,4,2,2,1,1,1,1,5}};
  const int gbad[][15] = {
    {0,1,4,8,8,4,3,3,1,1,1,1,1,1,0},{0,1,5,8,8,4,3,3,1,1,1,1,1,1,2},{0,1,4,8,8,5,3,3,1,1,1,1,1,1,2},{0,1,4,8,8,4,3,3,1,1,1,1,0,1,1},
    {0,1,4,8,8,4,3,0,1,1,1,1,1,1,1},{0,1,4,8,8,4,3,3,0,1,1,1,1,1,1},{0,1,4,8,8,4,3,3,1,1,1,-1,1,1,1},{0,1,4,8,8,4,3,3,1,1,1,1,5,1,1},
    {1,1,4,1,1,4,2,2,1,1,1,1,1,1,2},{0,1,4,1<<20,1<<20,4,3,3,1,1,1,1,1,1,2},
    {0,M,M,M,M,M,M,M,M,M,M,M,M,M,M},{1,M,M,M,M,M,M,M,M,M,M,M,M,M,1},{0,1,1,8,8,1,M,M,1,1,M,M,M,M,1},{1,1,1,M,M,1,2,2,M,M,0,0,M,M,1},
    {0,1,M,1,1,M,1,1,1,1,0,0,1,1,M},{0,1,1,8,8,1,3,3,1,1,M/2,M/2,M/2,M/2,1},{1,1,1,1,1,1,M,1,1,1,0,0,M,1,1},{0,1,1,1,1,1,1,1,M,M,M/2,M/2,1,1,1}};
  for (auto& r : grows) {
    size_t a=0,b=0,c=1,w=0; int oh=0, ow=0;
    if (fn2_conv_geometry_supported(r + 1, r[0]) != 1 || fn2_conv_geometry_sizes(r + 1, r[0], &a, &b, &c, &w) != 0 || !a || !b || c || !w ||
        fn2_conv_geometry_out_shape(r + 1, r[0], &oh, &ow) != 0 || oh < 1 || ow < 1) { printf("geometry row refused\n"); ++fails; }
    else printf("ok %zu %zu %zu %d x %d\n", a, b, w, oh, ow);
  }
  for (auto& r : gbad) {
    size_t a=1,b=1,c=1,w=1; int oh=1, ow=1;
    if (fn2_conv_geometry_supported(r + 1, r[0]) != 0 || fn2_conv_geometry_sizes(r + 1, r[0], &a, &b, &c, &w) != FN2_ERR_UNSUPPORTED || a || b || c || w ||
        fn2_conv_geometry_out_shape(r + 1, r[0], &oh, &ow) != FN2_ERR_UNSUPPORTED || oh || ow) { printf("bad geometry accepted %d %d\n", r[6], r[14]); ++fails; }
  }
  // the 19-int geometries of include/flownet2_hip_conv_volume.h: {transposed, N, Cin, D, H, W, Cout, kd, kh, kw, sd, sh, sw, pd, ph, pw, dd, dh, dw,
  // group}: rows of tests/conv_volume_cases.py, its invalid list, and values at the ends of the int range in every field
  const int vrows[][20] = {
    {0,2,3,4,5,6,5,3,3,3,1,1,1,1,1,1,1,1,1,1},{0,1,4,3,7,6,6,1,3,2,1,2,1,0,1,0,1,1,1,1},{0,2,3,7,5,8,4,3,2,2,2,1,1,1,0,2,2,1,3,1},
    {0,1,4,3,4,5,34,2,2,2,1,1,1,0,0,0,1,1,1,2},{0,2,3,4,4,5,3,3,3,3,1,1,1,1,1,1,1,1,1,3},{0,1,20,3,4,4,6,2,2,2,1,1,1,0,0,0,1,1,1,1},
    {0,2,2,3,5,7,3,3,3,3,1,1,1,1,1,1,1,1,1,1},{0,1,2,3,6,5,3,5,3,3,1,1,1,1,1,1,1,1,1,1},
    {1,2,5,2,3,4,3,4,4,4,2,2,2,1,1,1,1,1,1,1},{1,1,3,2,3,3,4,3,3,3,3,3,3,1,1,1,2,2,2,1},{1,1,4,3,4,5,3,3,2,2,2,1,1,1,0,2,2,1,3,1},
    {1,1,4,2,3,3,6,2,3,2,1,2,1,0,1,0,1,1,1,2},
    {0,2,4,1,1,9,6,1,1,3,1,1,2,0,0,1,1,1,2,2},{1,2,4,1,1,1,6,1,1,1,1,1,1,0,0,0,1,1,1,1}};      // (one and no spatial axis, folded)
  const int vbad[][20] = {
    {0,1,5,4,4,4,4,3,3,3,1,1,1,1,1,1,1,1,1,2},{0,1,4,4,4,4,5,3,3,3,1,1,1,1,1,1,1,1,1,2},{0,1,4,4,4,4,4,3,3,3,1,1,1,1,1,1,0,1,1,1},
    {0,1,4,4,8,8,4,3,3,3,1,1,1,1,1,1,3,1,1,1},{1,1,4,1,4,4,4,2,2,2,1,1,1,1,0,0,1,1,1,2},{0,1,4,4,4,4,4,0,3,3,1,1,1,1,1,1,1,1,1,1},
    {0,1,4,4,4,4,4,3,3,3,0,1,1,1,1,1,1,1,1,1},{0,1,4,4,4,4,4,3,3,3,1,1,1,-1,1,1,1,1,1,1},{0,1,4,4,4,4,4,3,3,3,1,1,1,1,1,1,1,1,1,0},
    {0,1,4,1<<10,1<<10,1<<10,4,3,3,3,1,1,1,1,1,1,1,1,1,2},{0,1,4,0,4,4,4,3,3,3,1,1,1,1,1,1,1,1,1,1},
    {0,M,M,M,M,M,M,M,M,M,M,M,M,M,M,M,M,M,M,M},{1,M,M,M,M,M,M,M,M,M,M,M,M,M,M,M,M,M,M,1},{0,1,1,8,8,8,1,M,M,M,1,1,1,M,M,M,M,M,M,1},
    {1,1,1,M,M,M,1,2,2,2,M,M,M,0,0,0,M,M,M,1},{0,1,M,1,1,1,M,1,1,1,1,1,1,0,0,0,1,1,1,M},{0,1,1,8,8,8,1,3,3,3,1,1,1,M/2,M/2,M/2,M/2,M/2,M/2,1},
    {1,1,1,1,1,1,1,M,1,1,1,1,1,0,0,0,M,1,1,1},{0,1,1,1,1,1,1,1,1,1,M,M,M,M/2,M/2,M/2,1,1,1,1},{0,1,1,M,2,2,1,1,1,1,1,1,1,0,0,0,1,1,1,1},
    {0,1,1,1291,1291,1291,1,1,1,1,1,1,1,0,0,0,1,1,1,1},{0,1,1,8,8,8,1,1291,1291,1291,1,1,1,645,645,645,1,1,1,1}};
  for (auto& r : vrows) {
    size_t a=0,b=0,c=1,w=0; int od=0, oh=0, ow=0;
    if (fn2_conv_volume_supported(r + 1, r[0]) != 1 || fn2_conv_volume_sizes(r + 1, r[0], &a, &b, &c, &w) != 0 || !a || !b || c || !w ||
        fn2_conv_volume_out_shape(r + 1, r[0], &od, &oh, &ow) != 0 || od < 1 || oh < 1 || ow < 1) { printf("volume row refused\n"); ++fails; }
    else printf("ok %zu %zu %zu %d x %d x %d\n", a, b, w, od, oh, ow);
  }
  for (auto& r : vbad) {
    size_t a=1,b=1,c=1,w=1; int od=1, oh=1, ow=1;
    if (fn2_conv_volume_supported(r + 1, r[0]) != 0 || fn2_conv_volume_sizes(r + 1, r[0], &a, &b, &c, &w) != FN2_ERR_UNSUPPORTED || a || b || c || w ||
        fn2_conv_volume_out_shape(r + 1, r[0], &od, &oh, &ow) != FN2_ERR_UNSUPPORTED || od || oh || ow) { printf("bad volume accepted %d %d\n", r[7], r[19]); ++fails; }
  }
  if (fn2_conv_volume_supported(nullptr, 0) != 0 || fn2_conv_volume_out_shape(nullptr, 1, nullptr, nullptr, nullptr) != FN2_ERR_UNSUPPORTED ||
      fn2_conv_volume_sizes(nullptr, 0, nullptr, nullptr, nullptr, nullptr) != FN2_ERR_UNSUPPORTED) ++fails;
  if (fn2_conv_geometry_supported(nullptr, 0) != 0 || fn2_conv_geometry_out_shape(nullptr, 1, nullptr, nullptr) != FN2_ERR_UNSUPPORTED) ++fails;
  if (fn2_conv_general_supported(nullptr, 0) != 0 || fn2_conv_general_sizes(nullptr, 1, nullptr, nullptr, nullptr, nullptr) != FN2_ERR_UNSUPPORTED) ++fails;
  printf("%s: %s\n", fails ? "FAILED" : "clean", fn2::last_error().c_str());
  return fails;
}
