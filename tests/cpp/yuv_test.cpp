// The YUV 4:2:0 output formats through include/raw_image_pipeline/raw_image_pipeline.hpp: setOutputFormat("nv12" / "i420") and
// setOutputYuvMatrix / getOutputYuvMatrix -- defaults, the four names and the refusal of an unknown one, without a device.
// Built as C++14 like the reference.
// usage: yuv_test host
#include <raw_image_pipeline/raw_image_pipeline.hpp>

#include <cstdio>
#include <string>

using raw_image_pipeline::RawImagePipeline;

static int fail(const char* what) {
  std::printf("FAIL: %s\n", what);
  return 1;
}

int main(int argc, char** argv) {
  if (argc != 2 || std::string(argv[1]) != "host") return fail("usage: yuv_test host");
  RawImagePipeline proc(false, "", "", "");
  if (proc.getOutputYuvMatrix() != "bt601") return fail("the default matrix");
  for (const char* name : {"bt709", "bt601_full", "bt709_full", "bt601"}) {
    proc.setOutputYuvMatrix(name);
    if (proc.getOutputYuvMatrix() != name) return fail("the getter does not return what was set");
  }
  proc.setOutputYuvMatrix("bt709_full");
  for (const char* bad : {"bt2020", "BT601", "", "bt601 ", "full"}) {
    try {
      proc.setOutputYuvMatrix(bad);
      return fail("an unknown matrix accepted");
    } catch (const std::invalid_argument& e) {
      const std::string what = e.what();
      for (const char* name : {"'bt601'", "'bt709'", "'bt601_full'", "'bt709_full'"})
        if (what.find(name) == std::string::npos) return fail("the refusal does not list the names");
    }
  }
  if (proc.getOutputYuvMatrix() != "bt709_full") return fail("a refused name changed the setting");
  for (const char* fmt : {"nv12", "i420", "native"}) {
    proc.setOutputFormat(fmt);
    if (proc.getOutputFormat() != fmt) return fail("the format getter");
    if (proc.getOutputYuvMatrix() != "bt709_full") return fail("the format changed the matrix");
  }
  try {
    proc.setOutputFormat("nv21");
    return fail("an unknown format accepted");
  } catch (const std::invalid_argument& e) {
    const std::string what = e.what();
    if (what.find("'nv12'") == std::string::npos || what.find("'i420'") == std::string::npos) return fail("the format refusal does not list the new names");
  }
  std::printf("yuv host OK\n");
  return 0;
}
