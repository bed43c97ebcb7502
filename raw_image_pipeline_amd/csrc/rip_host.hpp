// rip_host.hpp -- the host side of one pipeline, one header per subject: module parameters and their checks, the YAML-subset reader
// of the three config files, and the builders of the constant tables, undistortion maps and remap plan the HIP kernels consume.
// No device code here.
#pragma once
#include "rip_ccc_model.hpp"
#include "rip_color_tables.hpp"
#include "rip_output_tables.hpp"
#include "rip_params.hpp"
#include "rip_png.hpp"
#include "rip_undistort.hpp"
#include "rip_yaml.hpp"
