// The debayer-method extension through the C++ facade (include/raw_image_pipeline/raw_image_pipeline.hpp): default, set /
// get, and an unknown name rejected with std::invalid_argument and nothing changed.  Parameters only (RIP_DEVICE=-1 works).
#include <raw_image_pipeline/raw_image_pipeline.hpp>

#include <cstdio>
#include <stdexcept>
#include <string>

using raw_image_pipeline::RawImagePipeline;

static int fail(const char* what) {
  std::printf("FAIL: %s\n", what);
  return 1;
}

int main() {
  RawImagePipeline proc(false, "", "", "");
  if (proc.getDebayerMethod() != "bilinear") return fail("default method");
  proc.setDebayerMethod("mht");
  if (proc.getDebayerMethod() != "mht") return fail("set mht");
  bool threw = false;
  try {
    proc.setDebayerMethod("vng");
  } catch (const std::invalid_argument& e) {
    threw = std::string(e.what()).find("'bilinear', 'mht'") != std::string::npos;
  }
  if (!threw) return fail("unknown method not rejected with the valid names");
  if (proc.getDebayerMethod() != "mht") return fail("rejected method changed the handle");
  proc.setDebayerMethod("bilinear");
  if (proc.getDebayerMethod() != "bilinear") return fail("set bilinear");
  std::printf("debayer method OK\n");
  return 0;
}
