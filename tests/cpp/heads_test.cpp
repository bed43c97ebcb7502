// Output heads through include/raw_image_pipeline/raw_image_pipeline.hpp: setOutputHeads, selectOutputHead and their getters, the
// single-output setters and queries under a selection, the refusals, and processHeads as far as it goes without a device.
// Built as C++14 like the reference.
#include <raw_image_pipeline/raw_image_pipeline.hpp>

#include <cstdio>
#include <cstring>

using raw_image_pipeline::Mat;
using raw_image_pipeline::RawImagePipeline;

#ifdef RIP_HAVE_OPENCV
static Mat make_u8(int rows, int cols, int channels) { return Mat(rows, cols, CV_8UC(channels)); }
#else
static Mat make_u8(int rows, int cols, int channels) { return Mat(rows, cols, channels); }
#endif

static int fail(const char* what) {
  std::printf("FAIL: %s\n", what);
  return 1;
}

int main() {
  RawImagePipeline proc(false, "", "", "");
  proc.setFlip(false);
  proc.setUndistortion(false);
  if (proc.getOutputHeads() != 1 || proc.getSelectedOutputHead() != 0) return fail("defaults");
  for (int bad : {0, -1, 9}) {
    try {
      proc.setOutputHeads(bad);
      return fail("invalid head count accepted");
    } catch (const std::invalid_argument&) {
    }
  }
  try {
    proc.selectOutputHead(1);
    return fail("a head beyond n selected");
  } catch (const std::invalid_argument& e) {
    if (std::string(e.what()).find("0..0") == std::string::npos) return fail("the refusal does not name the heads");
  }
  proc.setOutputHeads(3);
  proc.selectOutputHead(2);
  proc.setOutputFormat("rgb8");
  proc.setOutputSize(64, 48);
  proc.setOutputFit("letterbox");
  proc.selectOutputHead(1);
  proc.setOutputRoi(8, 4, 64, 32);
  proc.setOutputFormat("mono8");
  int w = -1, h = -1, x = -1, y = -1, rw = -1, rh = -1;
  proc.selectOutputHead(0);
  proc.getOutputSize(w, h);
  proc.getOutputRoi(x, y, rw, rh);
  if (w || h || rw || rh || proc.getOutputFormat() != "native" || proc.getOutputFit() != "stretch") return fail("head 0 changed by the setters of heads 1 and 2");
  int rows = 0, cols = 0;
  Mat K, P;
  proc.getOutputCameraInfo(72, 136, 1, "bayer_rggb8", rows, cols, K, P);
  if (rows != 72 || cols != 136) return fail("head 0 delivers F");
  proc.selectOutputHead(1);
  proc.getOutputCameraInfo(72, 136, 1, "bayer_rggb8", rows, cols, K, P);
  if (rows != 32 || cols != 64 || proc.getOutputFormat() != "mono8") return fail("head 1 delivers its window");
  proc.selectOutputHead(2);
  int src[4], dst[4];
  proc.getOutputWindow(72, 136, 1, "bayer_rggb8", src, dst);
  if (dst[0] != 0 || dst[1] != 7 || dst[2] != 64 || dst[3] != 34 || proc.getSelectedOutputHead() != 2) return fail("head 2's letterbox");
  proc.setOutputHeads(2);  // head 2 goes, and the selection with it
  if (proc.getOutputHeads() != 2 || proc.getSelectedOutputHead() != 0) return fail("shrinking keeps the selection");
  proc.setOutputHeads(3);
  proc.selectOutputHead(2);
  proc.getOutputSize(w, h);
  if (w || h || proc.getOutputFormat() != "native" || proc.getOutputFit() != "stretch") return fail("a removed head kept its settings");
  proc.selectOutputHead(1);
  if (proc.getOutputFormat() != "mono8") return fail("head 1 lost its settings");
  // processHeads: refused without a device, selection unchanged
  Mat frame = make_u8(72, 136, 1);
  std::memset(frame.data, 0, 72 * 136);
  std::string enc = "bayer_rggb8";
  std::vector<Mat> outs;
  try {
    proc.processHeads(frame, enc, outs);
    return fail("frames processed without a device");
  } catch (const std::exception&) {
  }
  if (proc.getSelectedOutputHead() != 1 || enc != "bayer_rggb8" || !outs.empty()) return fail("a refused processHeads changed something");
  proc.selectOutputHead(2);
  proc.setOutputFormat("rgb_chw_f32");
  try {
    proc.processHeads(frame, enc, outs);
    return fail("a planar float head accepted");
  } catch (const std::invalid_argument& e) {
    if (std::string(e.what()).find("planar float") == std::string::npos) return fail("the refusal does not name the rule");
  }
  if (proc.getSelectedOutputHead() != 2) return fail("the selection after a refusal");
  std::printf("heads host OK\n");
  return 0;
}
