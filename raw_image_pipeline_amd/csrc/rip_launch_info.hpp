// rip_launch_info.hpp -- what a launch function of a kernel library reports back: the one record behind every launch_* of
// rip_output/resize/area/fit/aa/heads/mask/yuv/clahe/jpeg.hpp.
#pragma once

namespace rip {

// what was launched, for the launch record (rip_kernels.hpp RIP_LOG_LAUNCH; the record's sink is private to librip_hip.so)
struct LaunchInfo {
  const char* kernel;  // the instantiation as the demangler prints it, without namespaces
  unsigned grid_x, grid_y, block;
};

}  // namespace rip
