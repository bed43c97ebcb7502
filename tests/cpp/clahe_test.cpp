// CLAHE through include/raw_image_pipeline/raw_image_pipeline.hpp: setOutputClahe / getOutputClahe -- the default, values that are
// accepted, the refusals and that a refused call changes nothing -- without a device.  Built as C++14 like the reference.
// usage: clahe_test host
#include <raw_image_pipeline/raw_image_pipeline.hpp>

#include <cmath>
#include <cstdio>
#include <limits>
#include <string>

using raw_image_pipeline::RawImagePipeline;

static int fail(const char* what) {
  std::printf("FAIL: %s\n", what);
  return 1;
}

static bool is(const RawImagePipeline& proc, double clip, int tx, int ty) {
  double c = -1;
  int x = -1, y = -1;
  proc.getOutputClahe(c, x, y);
  return c == clip && x == tx && y == ty;
}

int main(int argc, char** argv) {
  if (argc != 2 || std::string(argv[1]) != "host") return fail("usage: clahe_test host");
  RawImagePipeline proc(false, "", "", "");
  if (!is(proc, 0.0, 0, 0)) return fail("the default is off");
  proc.setOutputClahe(3.0, 8, 8);
  if (!is(proc, 3.0, 8, 8)) return fail("the getter does not return what was set");
  proc.setOutputClahe(0.0, 16, 1);
  if (!is(proc, 0.0, 16, 1)) return fail("no clipping, 16 x 1 tiles");
  proc.setOutputClahe(40.0, 3, 5);
  const double bad_clip[] = {-1.0, std::numeric_limits<double>::infinity(), std::nan("")};
  for (double clip : bad_clip) {
    try {
      proc.setOutputClahe(clip, 8, 8);
      return fail("a clip limit that is negative or not finite accepted");
    } catch (const std::invalid_argument&) {
    }
  }
  const int bad_tiles[][2] = {{0, 8}, {8, 0}, {17, 8}, {8, 17}, {-1, -1}};
  for (const auto& t : bad_tiles) {
    try {
      proc.setOutputClahe(2.0, t[0], t[1]);
      return fail("tiles outside 1..16 accepted");
    } catch (const std::invalid_argument& e) {
      if (std::string(e.what()).find("1..16") == std::string::npos) return fail("the refusal does not name the range");
    }
  }
  if (!is(proc, 40.0, 3, 5)) return fail("a refused call changed the setting");
  proc.setOutputFormat("mono8");
  if (!is(proc, 40.0, 3, 5)) return fail("the format changed the setting");
  proc.setOutputClahe(0.0, 0, 0);
  if (!is(proc, 0.0, 0, 0)) return fail("off");
  std::printf("clahe host OK\n");
  return 0;
}
