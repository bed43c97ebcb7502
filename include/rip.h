/*
 * rip.h -- C-ABI of the MI355X-native RAW image pipeline (librip_hip.so).
 *
 * Drop-in boundary for raw_image_pipeline::RawImagePipeline (reference
 * raw_image_pipeline/include/raw_image_pipeline/raw_image_pipeline.hpp:36-137, "hpp" below;
 * implementation raw_image_pipeline/src/raw_image_pipeline/raw_image_pipeline.cpp, "cpp").
 * One rip_pipeline == one reference RawImagePipeline object == one camera stream; like the
 * reference it is not re-entrant (raw_image_pipeline_ros.cpp:14: one spinner thread per
 * node).  Plain pointers and sizes only; no C++/torch/OpenCV types cross this boundary.
 *
 * Every per-frame stage runs as hand-written HIP kernels on gfx950; there is no CPU
 * fallback.  Results follow the reference's CPU/OpenCV path (the parity target named by
 * BASELINE.json), whatever `use_gpu` says; rip_set_debayer_method("mht") opts into the CUDA
 * path's Malvar-He-Cutler demosaic.
 *
 * Errors: every function returns a rip_status; rip_last_error() gives the message.  The
 * C++ facade (include/raw_image_pipeline/raw_image_pipeline.hpp) maps
 * RIP_ERR_INVALID_ARGUMENT -> std::invalid_argument (reference debayer.cpp:76-78,
 * white_balance.hpp:82-84), RIP_ERR_ASSERT -> the cv::Exception an OpenCV assert would
 * have raised, RIP_ERR_IO -> YAML::Exception-class failures, the rest -> std::runtime_error.
 */
#ifndef RIP_H
#define RIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rip_pipeline rip_pipeline;

typedef enum {
  RIP_OK = 0,
  RIP_ERR_INVALID_ARGUMENT = 1, /* unsupported encoding / method / bad vector length */
  RIP_ERR_ASSERT = 2,           /* input the reference's OpenCV call would assert on */
  RIP_ERR_IO = 3,               /* malformed YAML / model file */
  RIP_ERR_DEVICE = 4,           /* HIP runtime failure, no device */
  RIP_ERR_CAPACITY = 5          /* caller's output buffer too small */
} rip_status;

/* Image taps kept per frame (reference keeps all three, unconditionally):
 *   DEBAYERED  FlipModule::image_  (flip.cpp:60-62)   -> getDistDebayeredImage (cpp:222-224)
 *   COLOR      UndistortionModule::dist_image_ (undistortion.cpp:247-249) -> getDistColorImage
 *   PROCESSED  RawImagePipeline::image_ (hpp:174-177) -> getProcessedImage */
enum { RIP_TAP_DEBAYERED = 1, RIP_TAP_COLOR = 2, RIP_TAP_PROCESSED = 4 };
enum { RIP_IMAGE_DEBAYERED = 0, RIP_IMAGE_COLOR = 1, RIP_IMAGE_PROCESSED = 2, RIP_IMAGE_RECT_MASK = 3 };

/* Device ordinal for a handle that only manages parameters (setters, getters, loaders, host-side
 * tables and maps) -- used by the CPU-only tests.  Every frame call on it fails with
 * RIP_ERR_DEVICE: there is no CPU execution path. */
#define RIP_DEVICE_NONE (-1)

/* ---- lifetime ------------------------------------------------------------------------ */
/* RawImagePipeline(bool use_gpu) / RawImagePipeline(use_gpu, params, calib, color_calib)
 * (hpp:39-41, cpp:16-40).  NULL or "" paths: parameters take the loader defaults of
 * cpp:44-165, no camera calibration, identity colour calibration *not available* (the
 * reference bakes source-tree default paths in at compile time, cpp:9-12; this library
 * ships no data files, so an empty params / colour-calibration path selects the VALUES of the
 * reference's example files instead).  `device` is the HIP device ordinal. */
rip_status rip_create(int device, int use_gpu, const char* params_path, const char* calibration_path,
                      const char* color_calibration_path, rip_pipeline** out);
/* RawImagePipeline(bool use_gpu) (hpp:39, cpp:16-21): the values of the reference's three example
 * config files (params, 720x540 equidistant camera, colour matrix). */
rip_status rip_create_default(int device, int use_gpu, rip_pipeline** out);
void rip_destroy(rip_pipeline* p);
/* Message of the last failure on this handle (p == NULL: of the last failed rip_create on
 * this thread).  Valid until the next call on the handle. */
const char* rip_last_error(const rip_pipeline* p);
/* HIP stream (hipStream_t) all device work of this handle is enqueued on; default: the
 * null stream.  The caller keeps ownership.  A switch orders the new stream behind the work this handle left on the old
 * one (its scratch state crosses frame calls in stream order): an event is recorded on the OLD stream during this call, so the
 * stream passed to the previous rip_set_stream must still exist when the next one is made -- destroy it only afterwards. */
rip_status rip_set_stream(rip_pipeline* p, void* hip_stream);

/* ---- frame API ----------------------------------------------------------------------- */
/* bool apply(cv::Mat& image, std::string& encoding) (hpp:47, cpp:190-205) on host memory:
 * uploads `image` (rows x cols x channels, `step` bytes per row), runs the chain, downloads
 * into `out` (tightly packed, capacity in bytes) and rewrites the encoding ("bayer_*8" ->
 * "bgr8").  The reference re-seats the caller's Mat; here the caller passes the output
 * buffer, whose geometry is returned (90/270 flips swap rows/cols).  Synchronous.
 *
 * Packed Bayer frames (extension beyond the reference): bayer_{rggb,bggr,gbrg,grbg} followed by one of
 *   10p       PFNC lsb-first bit stream (BayerRG10p ...): sample x of a row is bits [10 x, 10 x + 10) of its bytes read as a
 *             little-endian bit string
 *   12p       the same with 12 bits (BayerRG12p ...): even x: b[k] | (b[k+1] & 15) << 8, odd x: b[k] >> 4 | b[k+1] << 4, k = 12 x >> 3
 *   10_csi2   MIPI CSI-2 RAW10: groups of 4 samples in 5 bytes, g = x >> 2, j = x & 3: b[5g+j] << 2 | (b[5g+4] >> 2j) & 3
 *   12_csi2   MIPI CSI-2 RAW12: groups of 2 samples in 3 bytes, g = x >> 1: even x: b[3g] << 4 | b[3g+2] & 15,
 *             odd x: b[3g+1] << 4 | b[3g+2] >> 4
 * `rows` and `cols` count PIXELS, channels is 1, and a row occupies ceil(cols * B / 8) bytes (B = 10 or 12) from
 * image + y * step; `step` is in bytes, 0 = tight, smaller than a row: RIP_ERR_INVALID_ARGUMENT.  Bits of a row's last byte
 * beyond its last pixel and bytes beyond its payload are never interpreted.  The p layouts take any cols >= 3; 10_csi2 needs
 * cols % 4 == 0 and 12_csi2 cols % 2 == 0 (whole groups; RIP_ERR_INVALID_ARGUMENT otherwise); rows >= 3.  The bytes are
 * unpacked inside the demosaic kernel, and the frame produces exactly what the bayer_<pattern>16 frame holding the unpacked
 * samples produces under rip_set_debayer_16bit(1) and the effective range: the one of rip_set_debayer_16bit_range when one is
 * set, else the format's natural range (0, 2^B - 1).  The result is always "bgr8" (never bgr16), with taps, and does not
 * depend on rip_set_debayer_16bit. */
rip_status rip_apply(rip_pipeline* p, const uint8_t* image, int rows, int cols, int channels, size_t step,
                     const char* encoding, uint8_t* out, size_t out_capacity, int* out_rows, int* out_cols,
                     int* out_channels, char encoding_out[32]);
/* cv::Mat process(const cv::Mat&, std::string&) (hpp:50, cpp:182-188) is rip_apply with
 * distinct in/out buffers -- which rip_apply already requires; the facade maps both. */

/* Geometry/encoding rip_apply would produce for such an input (no device work). */
rip_status rip_query_output(rip_pipeline* p, int rows, int cols, int channels, const char* encoding,
                            int* out_rows, int* out_cols, int* out_channels, char encoding_out[32]);
/* Size of that result: *bytes = the tightly packed frame rip_apply / rip_submit_to / rip_collect check their capacities against
 * (out_rows * out_cols * out_channels * *elem_bytes), *elem_bytes = bytes per delivered element (1; 2 for bgr16 and the f16 / bf16
 * formats, 4 for f32), *planar = 1 for the planar output formats (rip_set_output_format), else 0.  Any pointer may be null.  Fails
 * where rip_query_output fails.  Works on RIP_DEVICE_NONE handles. */
rip_status rip_query_output_bytes(rip_pipeline* p, int rows, int cols, int channels, const char* encoding, size_t* bytes,
                                  int* elem_bytes, int* planar);
/* Geometry of the two tap images for such an input: the post-flip debayered image (flip.cpp:60-62, what
 * getDistDebayeredImage returns) and the pre-undistortion colour image (undistortion.cpp:247-249) share it;
 * rows * cols * channels tightly packed bytes per frame is what rip_apply_device writes to each tap buffer. */
rip_status rip_query_taps(rip_pipeline* p, int rows, int cols, int channels, const char* encoding,
                          int* tap_rows, int* tap_cols, int* tap_channels);

/* Device-resident, batched form of apply(): n_frames consecutive frames of THIS stream,
 * already in HBM (frame f at d_in + f*in_frame_stride, rows of in_step bytes), results to
 * d_out (frame stride out_frame_stride, row pitch out_step bytes; 0 = tightly packed).
 * Asynchronous on the handle's stream; frames are processed in order (the ccc Kalman state
 * advances frame by frame).  d_tap_debayered / d_tap_color (may be NULL) receive the
 * per-frame taps, tightly packed, same frame count.  Packed Bayer frames (rip_apply): rows / cols in pixels, in_step in
 * bytes (0 = ceil(cols * B / 8)); tiles of a 4-aligned d_in / in_step / in_frame_stride are read in aligned dwords -- the last
 * dword of a row's span may reach into the pitch, never beyond it and never beyond the last row's payload --, any other
 * alignment is read byte by byte. */
rip_status rip_apply_device(rip_pipeline* p, const void* d_in, size_t in_step, size_t in_frame_stride,
                            int n_frames, int rows, int cols, int channels, const char* encoding, void* d_out,
                            size_t out_step, size_t out_frame_stride, void* d_tap_debayered, void* d_tap_color);

/* ---- asynchronous host-memory frames: the path a streaming caller (raw_image_pipeline_ros.cpp:219-288: one host frame
 * per image callback) uses to keep the GPU and both PCIe directions busy at once --------------------------------------
 * rip_submit() is apply() split in two.  It uploads `image` (same arguments as rip_apply), enqueues the chain and the
 * download into a PINNED result buffer owned by the handle, and returns a ticket without waiting for any of it: upload of
 * frame f + 1, kernels of frame f and download of frame f - 1 run concurrently (three HIP streams, events in between).
 * Frames are processed in submission order (the ccc Kalman state advances frame by frame, exactly as with rip_apply).
 * The handle owns `depth` frame slots (rip_set_ring_depth, default 3, 1..16): with all of them in flight one more
 * rip_submit fails with RIP_ERR_CAPACITY and changes nothing.  A pageable `image` is read before rip_submit returns
 * (the library copies it into a pinned staging buffer of the frame's slot -- it does not rely on what the HIP runtime does
 * with an asynchronous copy from pageable memory); pinned memory (rip_host_alloc(), hipHostMalloc, hipHostRegister) is read
 * asynchronously, with no staging copy, and must stay untouched until the frame's rip_collect().  Debug dumps (rip_set_debug) are written by rip_apply only.
 * Whatever the depth, at most three host frames are in flight per DEVICE (all handles together; RIP_RING_INFLIGHT, 0 = no
 * limit): rip_submit waits for the oldest one to finish first -- beyond three the runtime's downloads slow down fourfold
 * (measured: tools/probes/ring_depth_probe.py), so a deeper ring only adds slots whose results can be held longer. */
rip_status rip_submit(rip_pipeline* p, const uint8_t* image, int rows, int cols, int channels, size_t step,
                      const char* encoding, uint64_t* ticket);
/* rip_submit with the destinations given by the caller: `out` (and, for the taps the handle keeps -- rip_set_taps --
 * `tap_debayered` / `tap_color`; NULL = not wanted here) are page-locked buffers (rip_host_alloc, hipHostMalloc,
 * hipHostRegister) the downloads are written into directly.  A caller that needs every frame in memory of its own -- the
 * deep copies the reference's process() and getters hand out (cpp:182-236) -- gets them without a pinned buffer of the handle
 * in between and without a memcpy: rip_collect only waits (its *out_view is `out`; the taps' views are the buffers given
 * here).  The buffers must stay valid and untouched until the ticket is collected.  Capacities in bytes; a buffer that is
 * too small, not page-locked, or a tap the handle does not keep: an error and nothing is enqueued. */
rip_status rip_submit_to(rip_pipeline* p, const uint8_t* image, int rows, int cols, int channels, size_t step,
                         const char* encoding, uint8_t* out, size_t out_capacity, uint8_t* tap_debayered, uint8_t* tap_color,
                         size_t tap_capacity, uint64_t* ticket);
/* Waits for the frame of `ticket` (tickets of one handle may be collected in any order) and hands over the result:
 * copied into `out` (tightly packed, `out_capacity` bytes) when out != NULL, and / or as a pointer to the handle's pinned
 * buffer in *out_view when out_view != NULL -- no copy.  The view, and the taps rip_get_image returns afterwards (those of
 * the collected frame), stay valid until the next rip_collect on this handle -- or until a rip_submit finds every other slot
 * in flight and takes this one: keep at most depth - 1 frames in flight to hold on to a result while submitting.  Geometry /
 * encoding as rip_apply.  Unknown or already collected ticket: RIP_ERR_INVALID_ARGUMENT. */
rip_status rip_collect(rip_pipeline* p, uint64_t ticket, uint8_t* out, size_t out_capacity, const uint8_t** out_view,
                       int* out_rows, int* out_cols, int* out_channels, char encoding_out[32]);
/* Frames the handle keeps in flight (1..16; default 3).  Only while nothing is in flight. */
rip_status rip_set_ring_depth(rip_pipeline* p, int depth);
/* Page-locked host memory for frames handed to rip_submit / rip_apply (hipHostMalloc): uploads from it are asynchronous
 * and run at the full PCIe rate.  NULL when the allocation fails. */
void* rip_host_alloc(size_t bytes);
void rip_host_free(void* ptr);
/* memcpy for whole frames: the deep copies the reference's API hands out (process(), every image getter: cpp:182-236) of a
 * 15 MB result are slower on one host thread than the frame's kernels and PCIe transfers together; copies of 4 MB and more
 * are split over a few library threads (RIP_COPY_THREADS, default 3 beside the caller; 0 = plain memcpy).  rip_collect and
 * rip_get_image copy this way themselves; this entry is for callers that copy out of a view. */
void rip_copy_host(void* dst, const void* src, size_t bytes);

/* Image getters (hpp:134-137, cpp:222-236): copy of the tap of the most recent rip_apply
 * frame.  RIP_IMAGE_RECT_MASK: the reference never writes rect_mask_ (undistortion.cpp:150-152), and under the rect mask
 * mode "off" (the default, rip_set_rect_mask) the image is empty here too (rows = cols = 0).  Under "coverage" / "valid",
 * after a frame call whose frame was undistorted, it is the valid-pixel mask of that frame's geometry: rows x cols of the maps,
 * one channel, built on the device when this getter asks; empty when the last frame was not undistorted. */
rip_status rip_get_image(rip_pipeline* p, int which, uint8_t* out, size_t out_capacity, int* rows, int* cols,
                         int* channels);
/* The same image without a copy, for frames that came through rip_collect: the final image always, the taps named by
 * rip_set_tap_download are downloaded together with the result, so after rip_collect *view points into the handle's pinned host memory (valid as long as the
 * rip_collect view: until the next rip_collect on the handle or until a rip_submit takes the slot).  *view is NULL -- with
 * the geometry still reported -- when the image only exists on the device (frames of rip_apply; images whose download went
 * into a buffer the caller named with rip_submit_to: that buffer is the caller's again once the ticket is collected and the
 * library does not look at it any more): use rip_get_image then.  RIP_IMAGE_RECT_MASK always reports its geometry with a NULL
 * view: the mask lives on the device.
 * hpp:134-137 (getDistDebayeredImage / getDistColorImage / getProcessedImage return Mat headers, no copy either). */
rip_status rip_get_image_view(rip_pipeline* p, int which, const uint8_t** view, int* rows, int* cols, int* channels);
/* Which of the kept taps (RIP_TAP_DEBAYERED | RIP_TAP_COLOR) rip_submit ALSO downloads into pinned host memory together
 * with the result, for rip_get_image_view / a copy-free rip_get_image after rip_collect.  Default 0: the taps stay on the
 * device until a getter asks (one synchronous device read each), and a caller that only wants the final image moves no
 * extra bytes.  A front end that publishes the taps of every frame (raw_image_pipeline_ros.cpp:245-287) sets the bits of
 * the images it publishes. */
rip_status rip_set_tap_download(rip_pipeline* p, int tap_mask);
/* Which taps rip_apply materialises (default: all three, as the reference does). */
rip_status rip_set_taps(rip_pipeline* p, int tap_mask);

/* ---- loaders (hpp:53-56) ---------------------------------------------------------------- */
rip_status rip_load_params(rip_pipeline* p, const char* file_path);             /* cpp:44-165 */
rip_status rip_load_camera_calibration(rip_pipeline* p, const char* file_path); /* undistortion.cpp:157-195 */
rip_status rip_load_color_calibration(rip_pipeline* p, const char* file_path);  /* color_calibration.cpp:52-76 */
rip_status rip_init_undistortion(rip_pipeline* p);                              /* undistortion.cpp:197-238 */
/* CCC model ("default.bin" layout: int32 w, int32 h, float32 filter[h*w], bias[h*w];
 * convolutional_color_constancy.cpp:116-132).  The reference loads a file baked in at
 * compile time; this library ships none, so method "ccc" needs one of these calls. */
rip_status rip_load_ccc_model(rip_pipeline* p, const char* file_path);
rip_status rip_set_ccc_model(rip_pipeline* p, int width, int height, const float* filter, const float* bias);
/* Kalman measurement model of the ccc temporal filter.  Default (h=0, r=1) is what the
 * pipeline's one-argument ConvolutionalColorConstancyWB constructor leaves behind
 * (convolutional_color_constancy.cpp:43-46 replaces the configured filter by a default
 * cv::KalmanFilter: H = 0); (h=1, r=10) is loadModel's configuration (:186-202). */
rip_status rip_set_ccc_kalman_model(rip_pipeline* p, double h, double r);

/* ---- other interfaces (hpp:59-61) -------------------------------------------------------- */
rip_status rip_reset_white_balance_temporal_consistency(rip_pipeline* p); /* cpp:218-220 */
rip_status rip_set_gpu(rip_pipeline* p, int use_gpu);                     /* cpp:210-212; recorded only (the CUDA path's
                                                                           demosaic: rip_set_debayer_method "mht") */
/* cpp:214-216.  While on, every rip_apply() of an 8-bit frame also writes the image after each of the eight modules --
 * enabled or not -- as the reference's pipeline() does (raw_image_pipeline.hpp:143-172 -> saveDebugImage :179-186: copy,
 * cv::normalize(0, 255, NORM_MINMAX), cv::imwrite): /tmp/00_debayer.png, 01_flip, 02_white_balancing, 03_color_calibration,
 * 04_gamma_correction, 05_vignetting_correction, 06_color_enhancer, 07_undistortion (.png).  The environment variable
 * RIP_DEBUG_DIR (read when the handle is created) replaces /tmp.  The fused kernel is re-run once per module prefix with the
 * gains of the real pass (outside any rip_profile_begin/end session).  The PNGs (stored, not compressed) hold the reference's
 * normalisation formula, scale / shift in double applied in float as separate multiply and add; an OpenCV built with FMA3
 * contracts that pair, so single values on a rounding tie may differ by 1 LSB from such a build.  The file names are fixed,
 * as in the reference: handles that share a directory overwrite each other's dumps (give each camera its own RIP_DEBUG_DIR).
 * A file that cannot be written does not fail the frame (cv::imwrite's result is ignored by the reference too); the paths are
 * left in rip_last_error().  rip_apply_device() never dumps. */
rip_status rip_set_debug(rip_pipeline* p, int debug);
/* Not in the reference: which OpenCV BUILD the float stages reproduce.  The colour matrix (color_calibration.cpp:93-103 ->
 * cv::gemm), the pca map (white_balance.cpp:122-127 -> cv::addWeighted), the HSV inverse (color_enhancer.cpp:44 ->
 * HSV2RGB_f) and the vignetting mask (vignetting_correction.cpp:42-43) are C expressions of the form a*b + c, which GCC and
 * Clang contract into fused multiply-adds wherever the target has them: every aarch64 build (the reference's Jetson
 * deployment, README.md:191-201), never the baseline x86-64 one.  mode 0 (default; environment RIP_FP_CONTRACT): every
 * product and every sum rounded; mode 1: the fused forms (oracle/rip_oracle.c contraction model 1).  The two differ by at
 * most 1 LSB per stage on rounding ties (PARITY.md).  Anything else: RIP_ERR_INVALID_ARGUMENT. */
rip_status rip_set_fp_contraction(rip_pipeline* p, int mode);

/* ---- setters (hpp:66-104; cpp:241-383) ---------------------------------------------------- */
rip_status rip_set_debayer(rip_pipeline* p, int enabled);                         /* hpp:66 */
rip_status rip_set_debayer_encoding(rip_pipeline* p, const char* encoding);       /* hpp:67 */
/* Extension beyond the reference, off by default.  DebayerModule lists bayer_{rggb,bggr,gbrg,grbg}16 (debayer.hpp:73-80)
 * and throws for them (debayer.cpp:76-78; so does this library).  With the extension on such frames (one channel of
 * uint16, pitches in bytes) are accepted.  What happens to them depends on the 16-bit range (below):
 *   range (0, 0), the default: demosaiced with the 8-bit path's formulas on 16-bit samples -- what cv::demosaicing does for
 *     CV_16UC1 -- and flipped; the result is 3 x uint16 per pixel, encoding "bgr16", rows * cols * 6 bytes.  Every other
 *     stage is an 8-bit stage in the reference and must be disabled (RIP_ERR_ASSERT otherwise); no taps are kept.
 *   range (black, white): demosaiced at 16 bits, narrowed to 8 bits, then the whole pipeline; "bgr8" out, taps kept. */
rip_status rip_set_debayer_16bit(rip_pipeline* p, int enabled);
/* Extension: black and white level of bayer_*16 frames.  (0, 0) (default) = off.  With rip_set_debayer_16bit(1) and
 * 0 <= black < white <= 65535 a bayer_*16 frame is (1) demosaiced at 16 bits by the method of rip_set_debayer_method
 * ("bilinear": the formulas and border rule above; "mht": the PARITY.md filters on 16-bit samples, clamped to [0, 65535],
 * reflect-101), (2) narrowed, every channel value v, in integers, with R = white - black:
 *     n(v) = min(255, floor((510 * max(v - black, 0) + R) / (2 * R)))
 * -- 255 (v - black) / R rounded half up; values below black give 0, values at or above white 255 -- and (3) processed from
 * there on exactly like a bgr8 frame holding the narrowed image: flip, white balance (ccc track included), colour matrix,
 * gamma, vignetting, enhancer, undistortion, the three taps (DEBAYERED = the flipped narrowed image), debug dumps,
 * rip_get_white_balance_info; the result is 3 x uint8 per pixel, encoding "bgr8".  Input pitches stay in bytes of uint16 rows.
 * Cost: as for "mht" -- a pass of its own, and without a DEBAYERED tap n_frames x rows x cols x 3 bytes of device memory
 * (rows padded to 16 bytes) kept by the handle.  Without rip_set_debayer_16bit(1) the range has no effect (the names throw).
 * Invalid ranges (black < 0, white > 65535, black >= white other than (0, 0)): RIP_ERR_INVALID_ARGUMENT, nothing changed.
 * Works on RIP_DEVICE_NONE handles.  Params YAML: `debayer: accept_16bit:` (bool, default false), `debayer: black_level:`,
 * `debayer: white_level:` (ints, default 0); rip_load_params re-creates the modules, so absent keys mean off, and fails with
 * RIP_ERR_INVALID_ARGUMENT on an invalid range, leaving the parameters as they were. */
rip_status rip_set_debayer_16bit_range(rip_pipeline* p, int black, int white);
rip_status rip_get_debayer_16bit_range(const rip_pipeline* p, int* black, int* white); /* either pointer may be null */
/* Extension beyond the reference: the demosaic of bayer_{rggb,bggr,gbrg,grbg}8 frames (and of bayer_*16 frames under
 * rip_set_debayer_16bit, clamped to [0, 65535]).  "bilinear" (default): the CPU path (debayer.cpp:49-70), what every other
 * function here describes.  "mht": Malvar-He-Cutler, the 5 x 5 gradient-corrected filter the reference's CUDA path runs
 * (cv::cuda::demosaicing(..., COLOR_Bayer**2BGR_MHT), debayer.cpp:93-108): integer weights over 16, rounded half to even,
 * reflect-101 reads outside the frame (PARITY.md gives the contract; pixels within 2 px of an edge are defined by that rule,
 * not checked against OpenCV's CUDA kernel).  Everything after the demosaic sees the MHT image exactly as it would see a bgr8
 * frame holding it.  Like bilinear it runs whatever rip_set_debayer says (debayer.hpp:38-40); mono8 / bgr8 / rgb8 frames are
 * not affected.  Cost: an MHT batch is demosaiced in a pass of its own, and without a DEBAYERED tap to hold its image it takes
 * n_frames x rows x cols x 3 bytes of extra device memory (rows padded to 16 bytes), kept by the handle.  rip_set_gpu does not
 * select it.  Unknown names: RIP_ERR_INVALID_ARGUMENT naming the two methods, nothing changed.  Works on RIP_DEVICE_NONE
 * handles.  The params YAML key `debayer: method:` (default "bilinear") sets it too; rip_load_params fails with
 * RIP_ERR_INVALID_ARGUMENT on an unknown value and leaves the parameters as they were. */
rip_status rip_set_debayer_method(rip_pipeline* p, const char* method);
rip_status rip_get_debayer_method(const rip_pipeline* p, char* out, size_t capacity); /* NUL-terminated copy */
/* Extension beyond the reference: the output stage.  The pipeline's final image F is 8-bit with channels 0, 1, 2 = B, G, R;
 * one exact per-pixel conversion behind the last module turns it into what rip_apply / rip_apply_device / rip_submit /
 * rip_collect deliver:
 *   native (default)   F itself: exactly the result without this extension, no extra launch, no extra memory
 *   rgb8               F with the channels of every pixel reversed; uint8, interleaved, 3 channels
 *   mono8              (3735 B + 19235 G + 9798 R + 16384) >> 15 -- OpenCV 4's 15-bit BGR2GRAY restated (PARITY.md; grey in gives
 *                      grey out, the primaries give R 76, G 150, B 29); uint8, 1 channel
 *   rgb_chw_f32 / rgb_chw_f16 / rgb_chw_bf16   planes R, G, B of T_c[v] (rip_set_output_normalization); 4 / 2 / 2 bytes per
 *   bgr_chw_f32 / bgr_chw_f16 / bgr_chw_bf16   planes B, G, R                       element; planar, 3 planes of out_rows x out_cols
 *   nv12 / i420        YUV 4:2:0 for encoders (rip_set_output_yuv_matrix below); uint8, one channel of 3 H / 2 rows x W bytes
 *   jpeg               one baseline JFIF stream per frame, encoded on the device (rip_set_output_jpeg below); uint8, one row of
 *                      `slot` bytes per frame; also takes a one-channel result
 * A format other than native needs a three-channel 8-bit pipeline result (Bayer 8-bit, 16-bit with a range, packed, bgr8 and rgb8
 * frames).  mono8 on a one-channel 8-bit result is the identity (no kernel); every other format on a one-channel result, and every
 * format other than native on a bgr16 result, fails the frame call and rip_query_output with RIP_ERR_INVALID_ARGUMENT: nothing is
 * enqueued and the ccc / Kalman state does not advance.
 * Geometry: the frame calls and rip_query_output report out_rows, out_cols, out_channels (3, or 1 for mono8) and the format's name
 * as encoding_out; rip_query_output_bytes gives the bytes.  rip_apply_device: for the interleaved formats out_step (0 = tight) and
 * out_frame_stride mean what they mean without a format; for the planar formats out_step is the row pitch in BYTES inside a plane
 * (0 = out_cols * element size), plane c of a frame starts at c * out_step * out_rows, and out_frame_stride is 0 for
 * 3 * out_step * out_rows or at least that -- a contiguous [n, 3, R, C] tensor is (0, 0).  d_out, out_step and out_frame_stride
 * must be multiples of the element size; the limits of 16 MiB per row and 4 GiB per frame apply to the converted frame.  Nothing
 * is written beyond out_cols elements of a row: row padding, gaps between planes and between frames stay untouched.
 * Unchanged by the format: the DEBAYERED and COLOR taps and their getters, rip_get_white_balance_info, rip_get_ccc_track and the
 * debug dumps (written from F).  RIP_IMAGE_PROCESSED reports an empty image under a format other than native, as it does for
 * bgr16 results: the delivered buffer is the result.
 * Cost: one more launch per batch (a memory-rate pass: 3 bytes read, up to 12 written per pixel), and n_frames x out_rows x
 * out_cols x 3 bytes of device memory (rows padded to 16 bytes) kept by the handle for F, as for "mht".
 * Unknown names: RIP_ERR_INVALID_ARGUMENT listing the names, nothing changed.  Works on RIP_DEVICE_NONE handles.  Params YAML:
 * `output: format:` (default "native"), `output: divisor:`, `output: mean: [3]`, `output: std: [3]`; rip_load_params re-creates
 * the modules, so absent keys mean the defaults, and fails with RIP_ERR_INVALID_ARGUMENT on an invalid value, leaving the
 * parameters as they were. */
rip_status rip_set_output_format(rip_pipeline* p, const char* name);
rip_status rip_get_output_format(const rip_pipeline* p, char* out, size_t capacity); /* NUL-terminated copy */
/* The formats "nv12" and "i420": the delivered 8-bit B, G, R picture of H rows x W columns (F, or F' behind a resize, window or
 * letterbox, the pad colour in it) as Y, Cb, Cr with one chroma sample per 2 x 2 block.  Exact integer arithmetic, this library's own
 * definition from the ITU matrices, not pinned against any encoder's or OpenCV's converter (PARITY.md "Output formats: YUV 4:2:0"):
 *   Y  = (yb B + yg G + yr R + (yoff << 15) + 16384) >> 15                       per pixel
 *   Cb = min(255, (cbb SB + cbg SG + cbr SR + (128 << 17) + 65536) >> 17)         per 2 x 2 block, SB, SG, SR the plain sums of the
 *   Cr = min(255, (crb SB + crg SG + crr SR + (128 << 17) + 65536) >> 17)         four pixels' channels: one rounding, no mean
 * with the matrix `name` of rip_set_output_yuv_matrix, a setting of the selected output head like every rip_set_output_*:
 *   bt601 (default)  yoff 16  y 3208 16520 8414   cb 14392  -9535 -4857   cr -2341 -12051 14392     limited range, Y 16..235
 *   bt709            yoff 16  y 2032 20127 5983   cb 14392 -11094 -3298   cr -1320 -13072 14392     limited range
 *   bt601_full       yoff 0   y 3735 19235 9798   cb 16384 -10855 -5529   cr -2664 -13720 16384     full range; Y is mono8's
 *   bt709_full       yoff 0   y 2366 23436 6966   cb 16384 -12630 -3754   cr -1502 -14882 16384     full range
 * (weights of B, G, R).  An unknown name: RIP_ERR_INVALID_ARGUMENT listing the names, nothing changed.  Works on RIP_DEVICE_NONE
 * handles; without effect under any other format; rip_set_output_heads resets it for the heads it resets.  Params YAML:
 * `yuv_matrix:` in `output:` and `output_1:` .. `output_7:`, absent = bt601, an invalid value fails the load.
 * Layout: the delivered frame is ONE-CHANNEL, 3 H / 2 rows x W bytes (cv::cvtColor(..., COLOR_BGR2YUV_I420)'s convention): the frame
 * calls and rip_query_output report out_rows = 3 H / 2, out_cols = W, out_channels = 1, encoding_out = the format's name;
 * rip_query_output_bytes gives 3 H W / 2, elem_bytes 1, planar 0.  The capacity, pitch and stride rules are those of that image:
 * out_step >= W, frame stride >= out_step * 3 H / 2, 16 MiB per row, 4 GiB per frame; any byte alignment of d_out and the pitch.
 * With P the resolved row pitch: Y row y at y * P.  nv12: chroma row j (0 <= j < H / 2) at (H + j) * P, byte 2 i = Cb and byte
 * 2 i + 1 = Cr of block (j, i).  i420: Cb row j at H * P + j * (P / 2), Cr row j at H * P + (H / 2) * (P / 2) + j * (P / 2); tight
 * rows give the standard contiguous I420.  Written: W bytes of each Y row, W bytes of each nv12 chroma row, W / 2 bytes of each i420
 * chroma row; row padding and the gaps between frames keep their bytes.
 * What describes the PICTURE stays H x W: rip_get_output_camera_info (matrices unchanged by the format), rip_get_output_window,
 * rip_get_output_mask; taps, white-balance info, the ccc track and the debug dumps stay on F; RIP_IMAGE_PROCESSED is empty.
 * Refusals, RIP_ERR_INVALID_ARGUMENT before anything is enqueued (the ccc filter does not advance), from the frame calls, the heads
 * calls (prefixed "output head <k>: ") and the queries, in this order: (1) the format rules above in their place -- a bgr16 result,
 * then a one-channel result; (2) an odd W or an odd H of the delivered picture, the message names the size; (3) rip_apply_device and
 * rip_apply_device_heads under i420: an odd row pitch.
 * Cost: one launch per batch in the converter's place (3 bytes read, 1.5 written per pixel) and the staging image of F as above. */
rip_status rip_set_output_yuv_matrix(rip_pipeline* p, const char* name);
rip_status rip_get_output_yuv_matrix(const rip_pipeline* p, char* out, size_t capacity); /* NUL-terminated copy */
/* Extension beyond the reference: CLAHE -- contrast-limited adaptive histogram equalisation, cv::createCLAHE(clip_limit,
 * Size(tiles_x, tiles_y))->apply() for CV_8UC1 restated (PARITY.md "Local contrast: CLAHE"; pinned against no OpenCV binary) -- on the
 * delivered ONE-CHANNEL picture of the selected output head: what a visual-inertial front end computes on the grey image before it
 * tracks features.  clip_limit: finite, >= 0, 0 = no clipping.  tiles_x, tiles_y: both in 1 .. 16, or both 0 = off (the default; a
 * handle that never turns it on launches what it launched before).  Anything else: RIP_ERR_INVALID_ARGUMENT, nothing changed.
 * The picture is the rectangle the resize writes (rip_get_output_window's dst), or all of the image: letterbox bands are neither
 * counted nor changed.  CLAHE is the last launch of the head: a one-channel frame under native (or mono8) without a resize goes
 * through the staging image, behind a resize it is equalised in place in the delivered buffer, and a colour frame under mono8 is
 * equalised in place behind the converter -- cv::CLAHE of the grey image.  The result does not depend on rip_set_fp_contraction.
 * Refusals, RIP_ERR_INVALID_ARGUMENT before anything is enqueued (the ccc filter does not advance), from the frame calls, the heads
 * calls (prefixed "output head <k>: ") and rip_query_output, rip_query_output_bytes, rip_get_output_camera_info and
 * rip_get_output_window, behind every other refusal of that head and in this order: (a) the delivered picture has more than one
 * channel (a colour result under native, rgb8, a planar or a YUV format; a bgr16 result) -- set the format mono8; (b) a picture
 * narrower than 2 tiles_x or lower than 2 tiles_y pixels.
 * Unchanged: the delivered geometry, rip_get_output_camera_info, rip_get_output_window, the masks, the taps, the white-balance info,
 * the ccc track and the debug dumps (all on F).  RIP_IMAGE_PROCESSED is empty while CLAHE is active, as under a resize.
 * Cost: two launches per batch -- one table per (tile, frame), 1 byte read per pixel; the blend, 1 byte read and 1 written per
 * pixel -- and n_frames x tiles_x x tiles_y x 256 bytes of device memory for the tables.  Works on RIP_DEVICE_NONE handles.
 * Params YAML: `clahe_clip_limit: 3.0` and `clahe_tiles: [8, 8]` in `output:` and `output_1:` .. `output_7:`; absent keys mean off,
 * an invalid value fails the load. */
rip_status rip_set_output_clahe(rip_pipeline* p, double clip_limit, int tiles_x, int tiles_y);
rip_status rip_get_output_clahe(const rip_pipeline* p, double* clip_limit, int* tiles_x, int* tiles_y); /* any pointer may be null */
/* The format "jpeg" (PARITY.md "Output formats: JPEG"): the delivered 8-bit picture of H rows x W columns (F, or F' behind a resize,
 * window or letterbox, where "nv12" sits) as a baseline JFIF 1.01 stream -- three components Y Cb Cr 4:2:0 from a three-channel
 * result, one component from a one-channel result -- that every JPEG decoder opens.  Exact integer arithmetic, tolerance 0 against
 * tests/jpeg_reference.py: full-range BT.601 (the "bt601_full" row of rip_set_output_yuv_matrix, whatever that setting says), the
 * picture extended to whole MCUs (16 x 16, or 8 x 8 for one component) by repeating its last column and row -- odd sizes are fine
 * --, an integer forward DCT, the Annex K tables scaled by the IJG rule for `quality` (1 .. 100, default 90), the Annex K Huffman
 * tables, a restart interval of `restart_rows` MCU rows (1 .. 64, default 1) with RSTm markers.  Header: SOI, APP0, DQT, SOF0 (the
 * true H and W), DHT, DRI, SOS; then the scan and EOI.  The setting has no effect under any other format; anything outside the
 * ranges: RIP_ERR_INVALID_ARGUMENT, nothing changed.
 * Delivered buffer: one SLOT per frame.  rip_query_output reports out_rows 1, out_cols slot, out_channels 1 and "jpeg";
 * rip_query_output_bytes gives the default slot: header (613 bytes, 330 for one component) + one byte per coded sample of the
 * extended picture (1.5 per pixel, 1 for one component) + 2 per restart interval + 2.  rip_apply_device(_heads): a non-zero out_step
 * is the capacity of a slot the caller chose, at least header + 2; out_frame_stride (0 = the slot) is at least the slot.  A stream
 * starts at its slot's first byte, at any alignment; the bytes of a slot behind the stream and between slots keep their contents.
 * A stream's length depends on the picture: rip_get_output_jpeg_sizes gives the lengths of the frames of the selected head's last
 * frame call (it waits for the handle's stream; sizes null: the count only; capacity below the count: RIP_ERR_CAPACITY).  The
 * count is 0 before the first frame call, after a frame call that delivered another format from that head and for a head
 * rip_set_output_heads has reset; a refused frame call, which enqueues nothing, leaves the lengths of the call before;
 * rip_get_output_jpeg_sizes_device the device array the kernels wrote (valid until that head's next frame call, ordered on the
 * handle's stream).  OVERFLOW: a frame whose stream does not fit its slot gets the length 0 and its slot is not written at all;
 * the call still returns RIP_OK and the other frames are unaffected.  The lengths are known before a byte of a stream is written.
 * rip_apply and rip_apply_heads check the capacity against the default slot, download the length first and then only the used
 * bytes; rip_submit, rip_submit_to (and so rip_collect) refuse a jpeg head with RIP_ERR_INVALID_ARGUMENT before anything is enqueued.
 * Refusals, RIP_ERR_INVALID_ARGUMENT before anything is enqueued (the ccc filter does not advance), behind the refusals of the
 * resize and in this order: a bgr16 result (the message of every other format); CLAHE on the same head; a picture beyond 65535
 * pixels per side or a restart interval beyond 65535 MCUs (the stream's 16-bit fields); from rip_apply_device(_heads) a slot below
 * header + 2.
 * Unchanged: rip_get_output_camera_info, rip_get_output_window and rip_get_output_mask (they describe the picture), the taps, the
 * white-balance info, the ccc track and the debug dumps.  A handle that never asks for "jpeg" launches, allocates and delivers what
 * it did before.
 * Cost: four launches per batch slice -- transform, sizing pass, scan, writing pass -- and device memory of 2 bytes per coded sample
 * (the quantised coefficients) plus 4 bytes per restart interval and frame; no stream is staged.  Works on RIP_DEVICE_NONE handles
 * (the setters, getters and queries).  Params YAML: `jpeg_quality: 90` and `jpeg_restart_rows: 1` in `output:` and `output_1:` ..
 * `output_7:`; absent keys mean the defaults, an invalid value fails the load. */
rip_status rip_set_output_jpeg(rip_pipeline* p, int quality, int restart_rows);
rip_status rip_get_output_jpeg(const rip_pipeline* p, int* quality, int* restart_rows); /* any pointer may be null */
rip_status rip_get_output_jpeg_sizes(rip_pipeline* p, uint32_t* sizes, int capacity, int* n);
rip_status rip_get_output_jpeg_sizes_device(rip_pipeline* p, const uint32_t** d_sizes, int* n);
/* The tables of a quality as the kernels read them, in natural (row-major) order, luminance then chrominance: the 2 x 64 divisors Q,
 * the reciprocals ceil(2^32 / (8 Q)) and the rounding terms 4 Q.  No handle is needed. */
rip_status rip_debug_jpeg_tables(int quality, uint8_t* q, uint32_t* recip, uint32_t* half);
/* Normalisation of the planar output formats; mean and std hold 3 values in the order of the format's planes.  Defaults:
 * divisor 255, mean (0, 0, 0), std (1, 1, 1); divisor 1 gives the raw values.  For plane c and channel value v in 0..255 the
 * delivered element is the table entry T_c[v]: y = (v / divisor - mean_c) / std_c evaluated in double with every operation
 * rounded, T_c[v] = (float)y; the f16 and bf16 formats deliver that float rounded to nearest even (overflow to +-inf and
 * subnormals as IEEE 754 says).  The tables are built on the host and uploaded when the format or the normalisation changes.
 * A non-finite divisor / mean / std, divisor == 0 or a std_c == 0: RIP_ERR_INVALID_ARGUMENT, nothing changed.  Works on
 * RIP_DEVICE_NONE handles. */
rip_status rip_set_output_normalization(rip_pipeline* p, double divisor, const double mean[3], const double std[3]);
rip_status rip_get_output_normalization(const rip_pipeline* p, double* divisor, double mean[3], double std[3]); /* any pointer may be null */
/* Extension beyond the reference: the resize stage.  A target size (width, height) makes rip_apply / rip_apply_device / rip_submit /
 * rip_collect deliver the output format applied to F' = resize(F, height rows, width cols) instead of F, the pipeline's final image
 * (rows x cols after flip / undistortion, 8-bit, 3 channels BGR or 1 channel); under "native" they deliver F' itself.  (0, 0), the
 * default, is off; otherwise both values are in 1..16384.  Anything else (one of them 0, negative, above 16384):
 * RIP_ERR_INVALID_ARGUMENT naming the rule, nothing changed.  A target equal to F's size delivers exactly what a handle without a
 * target delivers: no launch, no extra memory.
 * resize(F, H, W) is cv::resize(F, Size(W, H), 0, 0, INTER_LINEAR) on 8-bit data as oracle/rip_oracle.c restates it (PARITY.md
 * "Resize"; all integers behind two small per-axis tables built on the host): with R x C the size of F, the 2 x 2 mean
 * (a + b + c + d + 2) >> 2 when R == 2 H and C == 2 W, else two taps per axis with 11-bit weights and the source position
 * (x + 0.5) * C / W - 0.5 of output column x (pixel centres; rows alike), clamped at the edges.
 * Refused by the frame calls and by rip_query_output / rip_query_output_bytes / rip_get_output_camera_info with
 * RIP_ERR_INVALID_ARGUMENT, before anything is enqueued (the ccc / Kalman state does not advance): a target on a bgr16 result, and an
 * F larger than 16384 on a side.  The format rules are unchanged; mono8 on a one-channel result stays the identity, on F'.
 * Geometry: rip_query_output, rip_query_output_bytes, the frame calls' out_rows / out_cols, their capacity checks, rip_apply_device's
 * out_step / out_frame_stride rules and limits and the planar formats' plane stride all refer to the delivered height x width.
 * Unchanged and still on F: rip_query_taps, the DEBAYERED / COLOR taps and their getters, rip_get_white_balance_info,
 * rip_get_ccc_track, the debug dumps and every camera getter.  RIP_IMAGE_PROCESSED reports an empty image while a resize is active,
 * as it does under a format.
 * Cost: one more launch per batch slice in front of the converter, n_frames x rows x cols x channels bytes of device memory (rows
 * padded to 16 bytes) kept by the handle for F, and as much for F' under a format other than native.
 * Works on RIP_DEVICE_NONE handles.  Params YAML: `output: size: [width, height]`; rip_load_params re-creates the modules, so an
 * absent key means off; an invalid value fails with RIP_ERR_INVALID_ARGUMENT and leaves the parameters as they were. */
rip_status rip_set_output_size(rip_pipeline* p, int width, int height);
rip_status rip_get_output_size(const rip_pipeline* p, int* width, int* height); /* either pointer may be null */
/* Extension beyond the reference: the filter of the resize stage, "linear" (the default; the text above), "area", "linear_aa" or
 * "cubic_aa".  Any other name, or a null one: RIP_ERR_INVALID_ARGUMENT, nothing changed.  Without effect until a target size is active; it never touches the ccc
 * estimator's own resize, which stays linear.
 * Under "area" resize(F, H, W) is cv::resize(F, Size(W, H), 0, 0, INTER_AREA) for downscales (PARITY.md "Resize: area
 * interpolation"), per channel, with R x C the size of F: a target equal to F's size launches nothing; R == 2 H and C == 2 W is the
 * same 2 x 2 mean (a + b + c + d + 2) >> 2 as under "linear"; R % H == 0 and C % W == 0 otherwise: the integer sum of every
 * (R / H) x (C / W) block times the float 1.f / ((R / H) * (C / W)), rounded half to even; any other pair of sizes: per-axis lists of
 * consecutive taps with float weights built on the host in double, summed in float32 in tap order with every product and every sum
 * rounded (columns first, then rows), rounded half to even and clamped to 0..255.  The result does not depend on
 * rip_set_fp_contraction.
 * Refused under "area" with an active target, by the frame calls and by rip_query_output / rip_query_output_bytes /
 * rip_get_output_camera_info with RIP_ERR_INVALID_ARGUMENT before anything is enqueued (the ccc / Kalman state does not advance), on
 * top of the refusals above: a target wider or higher than F (area is a downscale filter), and an F more than 256 times the target
 * on an axis.  Geometry, pitches, taps, white-balance info, the ccc track, the dumps and rip_get_output_camera_info are what they are
 * under "linear": output pixel u' averages the source interval whose centre is (u' + 0.5) * C / W - 0.5.
 * Under "linear_aa" / "cubic_aa" resize(F, H, W) is, byte for byte, torch.nn.functional.interpolate(F as uint8 NCHW, size=(H, W),
 * mode='bilinear' / 'bicubic', antialias=True, align_corners=False) -- what torchvision.transforms.v2.Resize gives on uint8 tensors --
 * for downscales and upscales alike (PARITY.md "Resize: antialiased filters"): a separable triangle (support 1) or cubic (a = -0.5,
 * support 2) filter, stretched by the scale factor on a downscaled axis, with int16 fixed-point weights built on the host in double;
 * one pass is clamp((2^(prec - 1) + sum of taps) >> prec, 0, 255) in int32, and the picture is the horizontal pass over every source
 * row, rounded to uint8, then the vertical pass over that.  An axis that keeps its size is skipped; a target equal to F's size
 * launches nothing; there is no 2 x 2 special case (torch's taps are 1/8, 3/8, 3/8, 1/8).  Integer work only: the result does not
 * depend on rip_set_fp_contraction.  Refused under these two names, in the same calls and at the same place in the order as the
 * rules of "area": an F (or window) more than 64 times the target (or picture) on an axis.  Upscales are accepted up to 16384 per
 * side.  Everything else -- geometry, window, fit modes, pad, formats, what stays on F, camera info -- is what it is under "linear".
 * Works on RIP_DEVICE_NONE handles.  Params YAML: `output: interpolation: linear | area | linear_aa | cubic_aa`; an absent key means linear; an invalid
 * value fails with RIP_ERR_INVALID_ARGUMENT and leaves the parameters as they were. */
rip_status rip_set_output_interpolation(rip_pipeline* p, const char* name);
rip_status rip_get_output_interpolation(const rip_pipeline* p, char* out, size_t capacity); /* NUL-terminated copy */
/* Extension beyond the reference: the window and the fit mode of the resize stage (PARITY.md "Resize: window and fit").  All three
 * settings are off by default, and with the defaults every call behaves bit for bit as without them.
 * rip_set_output_roi: the rectangle (x, y, width, height) of F, the pipeline's final image, that the stage reads in place of all of F.
 * (0, 0, 0, 0) is off; otherwise x, y >= 0 and width, height in 1..16384.  Without a target size the frame calls deliver the window
 * itself, height x width; a window equal to all of F launches nothing.
 * rip_set_output_fit: how the window is placed in the target size, without effect while none is set.  "stretch" (default):
 * resize(window, H, W), each axis with its own ratio.  "crop": the window is first shrunk to the centred sub-window that has the
 * target's aspect, then stretched.  "letterbox": the whole window is resized to the largest Wi x Hi picture with the window's aspect
 * that fits the target (rounded to nearest, at least 1), centred at (left, top) = ((W - Wi) / 2, (H - Hi) / 2); every other pixel
 * of the H x W image gets the pad colour.  With equal aspects letterbox is stretch and nothing is padded.
 * rip_set_output_pad: that colour as B, G, R of F', each in 0..255, default (114, 114, 114).  It is applied before the output
 * format, so padded pixels show what the format makes of those bytes; a one-channel result is padded with the grey value
 * (3735 b + 19235 g + 9798 r + 16384) >> 15.
 * The bytes of the picture are those the stage delivers for a frame that holds only the window, under the handle's interpolation,
 * with the rule (copy, 2 x 2 mean, whole factors, tap lists, linear tables) decided on window size -> picture size; pixels of F
 * outside the window never influence them.  The window is read where F lies: there is no copy of it.
 * Invalid values (a negative origin, a side of 0 or above 16384, an unknown or null name, a component outside 0..255):
 * RIP_ERR_INVALID_ARGUMENT naming the rule, nothing changed.  A window that does not lie inside F (x + width > C or y + height > R)
 * can only be told when a frame's geometry is known: the frame calls, rip_query_output, rip_query_output_bytes,
 * rip_get_output_camera_info and rip_get_output_window refuse it with RIP_ERR_INVALID_ARGUMENT before anything is enqueued (the
 * ccc / Kalman state does not advance).  The refusals of rip_set_output_size and rip_set_output_interpolation apply as before, in
 * this order: a bgr16 result (also for a window without a target), the window outside F, an F above 16384 on a side, and under
 * "area" the upscale and factor-256 rules on window size -> picture size.
 * Everything rip_set_output_size lists as staying on F stays on F; RIP_IMAGE_PROCESSED is empty with a window and no target too.
 * Work on RIP_DEVICE_NONE handles.  Params YAML: `output: roi: [x, y, w, h]`, `output: fit: stretch | letterbox | crop`,
 * `output: pad: [b, g, r]`; absent keys mean the defaults; an invalid value fails with RIP_ERR_INVALID_ARGUMENT and leaves the
 * parameters as they were. */
rip_status rip_set_output_roi(rip_pipeline* p, int x, int y, int width, int height);
rip_status rip_get_output_roi(const rip_pipeline* p, int* x, int* y, int* width, int* height); /* any pointer may be null */
rip_status rip_set_output_fit(rip_pipeline* p, const char* name);
rip_status rip_get_output_fit(const rip_pipeline* p, char* out, size_t capacity); /* NUL-terminated copy */
rip_status rip_set_output_pad(rip_pipeline* p, int b, int g, int r);
rip_status rip_get_output_pad(const rip_pipeline* p, int* b, int* g, int* r); /* any pointer may be null */
/* For an input frame of that geometry (arguments as for rip_query_output): src_xywh, the rectangle (x, y, width, height) of F that is
 * read -- the window, after "crop" -- and dst_xywh, the rectangle of the delivered image that holds picture; everything outside it
 * is pad.  Maps detections back to the source: u = (u' - dst x + 0.5) * src width / dst width - 0.5 + src x, rows alike.  Without
 * a window, a fit mode or a target both are (0, 0, C, R).  Either pointer may be null.  Fails where rip_query_output fails.  Works
 * on RIP_DEVICE_NONE handles. */
rip_status rip_get_output_window(rip_pipeline* p, int rows, int cols, int channels, const char* encoding, int src_xywh[4], int dst_xywh[4]);
/* Camera matrix K (3 x 3) and projection matrix P (3 x 4) of the image the frame calls deliver for such an input frame (arguments as
 * for rip_query_output), with its size in *height / *width.  They start from the rect K / P when that frame would be undistorted,
 * else from the dist K / P; with a target size and a = width / C, b = height / R in double (R x C: the size of F; every operation
 * rounded): K[0] *= a, K[1] *= a, K[2] = a * (K[2] + 0.5) - 0.5, K[4] *= b, K[5] = b * (K[5] + 0.5) - 0.5, rows 0 and 1 of P
 * likewise with P[3] *= a and P[7] *= b -- the inverse of the pixel-centre mapping u = (u' + 0.5) / a - 0.5 the resize uses.  With a window
 * or a fit mode (rip_set_output_roi, rip_set_output_fit), (xs, ys, ws, hs) and (left, top, Wi, Hi) the two rectangles of
 * rip_get_output_window, a = Wi / ws and b = Hi / hs: K[0] *= a, K[1] *= a, K[2] = (a * ((K[2] - xs) + 0.5) - 0.5) + left, K[4] *= b,
 * K[5] = (b * ((K[5] - ys) + 0.5) - 0.5) + top, P likewise; the size is the target's, or the window's without a target.  Without
 * an active resize the matrices come back unchanged with F's size.  Any output pointer may be null.  Fails where rip_query_output
 * fails.  Works on RIP_DEVICE_NONE handles. */
rip_status rip_get_output_camera_info(rip_pipeline* p, int rows, int cols, int channels, const char* encoding, int* height, int* width,
                                      double K[9], double P[12]);
/* Extension beyond the reference: output heads -- several delivered images per frame from one run of the chain (PARITY.md "Output
 * heads").  An output head is one complete set of the output stage's settings: format and normalisation, target size, interpolation,
 * window, fit mode and pad colour.  A handle has n heads, 1 <= n <= RIP_MAX_OUTPUT_HEADS; head 0 is the output of a handle that
 * never asked for more, further heads start at the defaults ("native", no target, no window, "stretch", "linear", pad 114).
 * rip_set_output_heads: sets n.  Heads at and beyond n are reset to the defaults; a selection at or beyond n becomes 0.  Refused
 * with RIP_ERR_INVALID_ARGUMENT outside 1..8 and while ring frames are in flight (as rip_set_ring_depth is).
 * rip_select_output_head: which head every single-output entry addresses from now on -- the setters and getters rip_set / get_
 * output_format, _normalization, _size, _interpolation, _roi, _fit, _pad; the queries rip_query_output, rip_query_output_bytes,
 * rip_get_output_camera_info, rip_get_output_window; and the frame calls rip_apply, rip_apply_device, rip_submit, rip_submit_to
 * (the frame of a ring slot is delivered under the head selected when it was submitted).  An index outside 0..n-1:
 * RIP_ERR_INVALID_ARGUMENT, nothing changed.  With n = 1 and head 0 selected -- the defaults -- every call behaves bit for bit as
 * it did before there were heads.
 * Work on RIP_DEVICE_NONE handles.  Params YAML: the sections `output_1:` .. `output_7:` take exactly the keys of `output:`; after
 * a load n = 1 + the largest k present, sections absent in between hold the defaults and head 0 is selected; a file without such
 * a section gives n = 1.  `output_8:` and above, or an invalid value inside a section: RIP_ERR_INVALID_ARGUMENT, parameters as
 * they were. */
#define RIP_MAX_OUTPUT_HEADS 8
rip_status rip_set_output_heads(rip_pipeline* p, int n);
rip_status rip_get_output_heads(rip_pipeline* p, int* n); /* the pointer may be null */
rip_status rip_select_output_head(rip_pipeline* p, int head);
rip_status rip_get_selected_output_head(rip_pipeline* p, int* head); /* the pointer may be null */
/* One head's buffer of rip_apply_device_heads: d_out, out_step and out_frame_stride as rip_apply_device takes them for that head's
 * settings (0 = tightly packed); d_out NULL: the head is not requested -- it is neither planned nor validated and nothing runs for it. */
typedef struct {
  void* d_out;
  size_t out_step;
  size_t out_frame_stride;
} rip_head_buffer;
/* rip_apply_device with one delivered image per requested head.  The chain, the white-balance statistics, the ccc estimator and the
 * undistortion run ONCE per batch (slice); the ccc Kalman state advances once per frame; the taps, rip_get_white_balance_info and
 * rip_get_ccc_track are those of that one run.  The bytes written into head k's buffer are exactly the bytes rip_apply_device writes
 * into a buffer of the same layout on a handle with the same pipeline settings whose only output has head k's settings, float formats
 * as bit patterns; bytes that call leaves untouched (row padding, plane remainders, gaps between frames) stay untouched here.
 * heads: n_heads entries, n_heads equal to rip_get_output_heads.  Overlapping head buffers are the caller's responsibility.
 * Checked in this order, all before anything is enqueued (the ccc filter does not advance): a null d_in, heads or encoding;
 * n_heads other than the handle's n; no requested head; the frame's own refusals (as rip_apply_device); for each requested head in
 * index order the refusals of its settings in their usual order, then the layout rules of rip_apply_device for its buffer -- the
 * message prefixed "output head <k>: "; more than one requested head on a bgr16 result; taps on a bgr16 result.  n_frames == 0
 * returns RIP_OK.  One requested head takes exactly the launches of rip_apply_device.  With several, among the requested heads that
 * deliver F as it is ("native", no active resize, no window smaller than F), in index order, the first whose buffer address, row
 * pitch and frame stride are all multiples of 16 bytes is written by the chain's last kernel directly and read by the other heads
 * (tight bgr8 rows of 2448, 1920 or 1440 pixels qualify); every other such head costs one copy launch (head_copy_kernel of
 * librip_heads_hip.so); every other head runs its resize / pad / converter launches in index order.  The launch record
 * (rip_debug_launch_log) of a call is the chain's launches of a single run followed per head by that head's. */
rip_status rip_apply_device_heads(rip_pipeline* p, const void* d_in, size_t in_step, size_t in_frame_stride, int n_frames, int rows, int cols,
                                  int channels, const char* encoding, const rip_head_buffer* heads, int n_heads, void* d_tap_debayered,
                                  void* d_tap_color);
/* rip_apply with one delivered image per requested head: uploads the frame once, runs as rip_apply_device_heads does and downloads
 * every requested head tightly packed into outs[k] (NULL: not requested) of out_capacities[k] bytes -- RIP_ERR_CAPACITY, message
 * prefixed "output head <k>: ", where rip_apply gives it.  out_rows / out_cols / out_channels: n_heads entries each with the delivered
 * geometry of the requested heads (0 for the others); each array may be null.  RIP_IMAGE_PROCESSED is empty afterwards -- the
 * delivered buffers are the results -- while the DEBAYERED and COLOR taps are kept as rip_apply keeps them.  Writes no debug dumps
 * whatever rip_set_debug says. */
rip_status rip_apply_heads(rip_pipeline* p, const uint8_t* image, int rows, int cols, int channels, size_t step, const char* encoding,
                           uint8_t* const* outs, const size_t* out_capacities, int n_heads, int* out_rows, int* out_cols, int* out_channels);
/* Test hook: for head `head` (0..n-1, else RIP_ERR_INVALID_ARGUMENT), *table_builds: how often its device tables (the planar formats'
 * table, the resize tables) were built and uploaded since the handle was created -- a steady sequence of identical calls builds each
 * head's tables once; *direct_write / *copied: whether the last frame call that delivered the head had the chain write its buffer
 * directly (also true of a head that delivers F in a single-output call) or copied it from the staging image.  Any pointer may be null. */
rip_status rip_debug_output_head_info(rip_pipeline* p, int head, int* table_builds, int* direct_write, int* copied);
/* Extension beyond the reference: valid-pixel masks (PARITY.md "Rect mask").  Delivered pixels that are not image -- the black border
 * a balance above 0 leaves, the rim where cv::remap blended a source pixel with the border constant, the bands of a letterbox -- are
 * told apart from image by a mask.  mode: "off" (default: every call behaves exactly as without this extension), "coverage" or "valid";
 * any other name, or a null one: RIP_ERR_INVALID_ARGUMENT, nothing changed.
 * The coverage mask M of a frame the plan would undistort is cv::remap(white, map_x, map_y, INTER_LINEAR, BORDER_CONSTANT 0) with
 * `white` an all-255 image of the size that enters the remap (the frame after the flip): rows x cols of the maps, uint8, one channel.
 * It depends on the maps and on that size and on no frame content.  "valid" hands out V = (M == 255) ? 255 : 0: a pixel whose taps
 * outside the source carry at most 64 / 32768 of the weight, so that it differs from a fully interior pixel by at most one level.
 * RIP_IMAGE_RECT_MASK (rip_get_image) is M or V for the last frame call's geometry.
 * The delivered mask M' of an output head, H x W as rip_query_output reports for the head: what that head delivers under the format
 * "native" with the pad (0, 0, 0) for a one-channel frame whose final image is M -- M is all 255 at F's size for a frame that is not
 * undistorted.  So letterbox bands are 0, a window cuts M, and a resize filters M with the head's own filter.  Under "valid" the
 * threshold follows the head's geometry: V' = (M' == 255) ? 255 : 0.  A mask is always uint8, one channel; the head's format and
 * normalisation do not apply.
 * The frame calls do no mask work, whatever the mode: their launches are the same.  Masks are built by the getters, on the handle's
 * stream, and cached on the device -- M per (maps, size entering the remap), M' per head -- until the maps are rebuilt or replaced
 * (calibration, image sizes, balance, fov scale, K, D, model, R, P, rip_init_undistortion, rip_load_params), an output setter of the
 * head is called, or rip_set_output_heads resets the head.
 * Works on RIP_DEVICE_NONE handles.  Params YAML: `undistortion: mask: off | coverage | valid`; an absent key means off; an invalid
 * value fails with RIP_ERR_INVALID_ARGUMENT and leaves the parameters as they were. */
rip_status rip_set_rect_mask(rip_pipeline* p, const char* mode);
rip_status rip_get_rect_mask_mode(const rip_pipeline* p, char* out, size_t capacity); /* NUL-terminated copy */
/* The delivered mask of the selected head for an input frame of that geometry (arguments as for rip_query_output; no frame need have
 * been processed): H * W bytes, tight rows, into out[capacity]; *height / *width (either may be null) receive H and W.  Refused before
 * anything is enqueued, in this order: the mode "off" (RIP_ERR_INVALID_ARGUMENT, the message says so); exactly the refusals of
 * rip_query_output; a capacity below H * W (RIP_ERR_CAPACITY).  out == NULL returns the geometry only and works on RIP_DEVICE_NONE
 * handles; a non-NULL out on such a handle fails with RIP_ERR_DEVICE.  Synchronous. */
rip_status rip_get_output_mask(rip_pipeline* p, int rows, int cols, int channels, const char* encoding, uint8_t* out, size_t capacity,
                               int* height, int* width);
/* The same image where it is cached on the device: *d_mask, rows *pitch bytes apart (a multiple of 16), written in the order of the
 * handle's stream.  It stays valid until the next call that drops that head's cache -- also a mask getter for another geometry or mode
 * under that head -- or destroys the handle.  pitch, height and width may be null. */
rip_status rip_get_output_mask_device(rip_pipeline* p, int rows, int cols, int channels, const char* encoding, const uint8_t** d_mask,
                                      size_t* pitch, int* height, int* width);
/* Test hook: *mask_builds: how often a mask of a frame geometry (M, its thresholded twin, or the all-255 image) was built since the
 * handle was created; *head_builds: how often the delivered mask of head `head` (0..n-1, else RIP_ERR_INVALID_ARGUMENT) was.  A steady
 * sequence of identical getter calls builds each once.  Either pointer may be null. */
rip_status rip_debug_rect_mask_info(rip_pipeline* p, int head, int* mask_builds, int* head_builds);
rip_status rip_set_flip(rip_pipeline* p, int enabled);                            /* hpp:69 */
rip_status rip_set_flip_angle(rip_pipeline* p, int angle);                        /* hpp:70 */
rip_status rip_set_white_balance(rip_pipeline* p, int enabled);                   /* hpp:72 */
rip_status rip_set_white_balance_method(rip_pipeline* p, const char* method);     /* hpp:73 */
rip_status rip_set_white_balance_percentile(rip_pipeline* p, double percentile);  /* hpp:74 */
rip_status rip_set_white_balance_saturation_threshold(rip_pipeline* p, double bright_thr, double dark_thr); /* hpp:75 */
rip_status rip_set_white_balance_temporal_consistency(rip_pipeline* p, int enabled); /* hpp:76 */
rip_status rip_set_color_calibration(rip_pipeline* p, int enabled);               /* hpp:77 */
rip_status rip_set_color_calibration_matrix(rip_pipeline* p, const double* m, int n); /* hpp:78, n == 9 */
rip_status rip_set_color_calibration_bias(rip_pipeline* p, const double* b, int n);   /* hpp:79, n == 3 */
rip_status rip_set_gamma_correction(rip_pipeline* p, int enabled);                /* hpp:83 */
rip_status rip_set_gamma_correction_method(rip_pipeline* p, const char* method);  /* hpp:84 */
rip_status rip_set_gamma_correction_k(rip_pipeline* p, double k);                 /* hpp:85 */
rip_status rip_set_vignetting_correction(rip_pipeline* p, int enabled);           /* hpp:87 */
rip_status rip_set_vignetting_correction_parameters(rip_pipeline* p, double scale, double a2, double a4); /* hpp:88 */
rip_status rip_set_color_enhancer(rip_pipeline* p, int enabled);                  /* hpp:90 */
/* The reference's setters are cross-wired (color_enhancer.cpp:23-33): "hue" scales the V
 * channel and "value" scales H.  Reproduced, so a drop-in caller sees the same pixels. */
rip_status rip_set_color_enhancer_hue_gain(rip_pipeline* p, double gain);         /* hpp:91 */
rip_status rip_set_color_enhancer_saturation_gain(rip_pipeline* p, double gain);  /* hpp:92 */
rip_status rip_set_color_enhancer_value_gain(rip_pipeline* p, double gain);       /* hpp:93 */
rip_status rip_set_undistortion(rip_pipeline* p, int enabled);                    /* hpp:95 */
rip_status rip_set_undistortion_image_size(rip_pipeline* p, int width, int height);     /* hpp:96 */
rip_status rip_set_undistortion_new_image_size(rip_pipeline* p, int width, int height); /* hpp:97 */
rip_status rip_set_undistortion_balance(rip_pipeline* p, double balance);         /* hpp:98 */
rip_status rip_set_undistortion_fov_scale(rip_pipeline* p, double fov_scale);     /* hpp:99 */
rip_status rip_set_undistortion_camera_matrix(rip_pipeline* p, const double* k, int n);            /* hpp:100, n >= 9 */
/* n >= 4; the first min(n, 8) values are kept and the rest taken as 0.  What they mean is the model's business (below). */
rip_status rip_set_undistortion_distortion_coefficients(rip_pipeline* p, const double* d, int n);  /* hpp:101, n >= 4 */
/* Distortion models.  "none": no remap.  "plumb_bob", "radtan", "rational_polynomial": the pinhole (Brown-Conrady) models of
 * ROS camera_calibration / Kalibr -- the new camera matrix follows cv::getOptimalNewCameraMatrix (alpha = balance clamped to
 * [0, 1]: 0 crops to valid pixels, 1 keeps every source pixel) and the maps cv::initUndistortRectifyMap, both restated in
 * double (PARITY.md "Pinhole distortion models"; not pinned against an OpenCV binary):
 *   plumb_bob            D = k1 k2 p1 p2 k3              (5 coefficients reported; k4..k6 taken as 0)
 *   radtan               D = k1 k2 p1 p2, k3 = 0         (5 coefficients reported)
 *   rational_polynomial  D = k1 k2 p1 p2 k3 k4 k5 k6     (8 coefficients reported)
 * Missing trailing coefficients are 0; thin-prism and tilt terms are not supported (the calibration loader refuses a
 * distortion_coefficients list whose values beyond the eighth are not all zero with RIP_ERR_INVALID_ARGUMENT).
 * Every other name -- "equidistant" among them -- builds fisheye (Kannala-Brandt, cv::fisheye) maps from the first four
 * coefficients, as the reference does for any model string. */
rip_status rip_set_undistortion_distortion_model(rip_pipeline* p, const char* model);              /* hpp:102 */
rip_status rip_set_undistortion_rectification_matrix(rip_pipeline* p, const double* r, int n);     /* hpp:103, n >= 9 */
rip_status rip_set_undistortion_projection_matrix(rip_pipeline* p, const double* pm, int n);       /* hpp:104, n >= 12 */

/* ---- getters (hpp:80-81, 109-132; cpp:388-489) ---------------------------------------------- */
int rip_is_debayer_enabled(const rip_pipeline* p);               /* hpp:109 */
int rip_is_flip_enabled(const rip_pipeline* p);                  /* hpp:110 */
int rip_is_white_balance_enabled(const rip_pipeline* p);         /* hpp:111 */
int rip_is_color_calibration_enabled(const rip_pipeline* p);     /* hpp:112 */
int rip_is_gamma_correction_enabled(const rip_pipeline* p);      /* hpp:113 */
int rip_is_vignetting_correction_enabled(const rip_pipeline* p); /* hpp:114 */
int rip_is_color_enhancer_enabled(const rip_pipeline* p);        /* hpp:115 */
int rip_is_undistortion_enabled(const rip_pipeline* p);          /* hpp:116 */
int rip_get_dist_image_height(const rip_pipeline* p);            /* hpp:118 */
int rip_get_dist_image_width(const rip_pipeline* p);             /* hpp:119 */
int rip_get_rect_image_height(const rip_pipeline* p);            /* hpp:126 */
int rip_get_rect_image_width(const rip_pipeline* p);             /* hpp:127 */
/* Strings are copied into out[capacity] (NUL-terminated). */
rip_status rip_get_dist_distortion_model(const rip_pipeline* p, char* out, size_t capacity); /* hpp:120 */
rip_status rip_get_rect_distortion_model(const rip_pipeline* p, char* out, size_t capacity); /* hpp:128 */
/* Matrices are written row-major as float64, like the CV_64F Mats the reference returns:
 * 3x3 -> out[9], 1x4 -> out[4], 3x4 -> out[12]; colour calibration 3x3 / 4x1 (cv::Scalar). */
rip_status rip_get_color_calibration_matrix(const rip_pipeline* p, double out[9]);   /* hpp:80 */
rip_status rip_get_color_calibration_bias(const rip_pipeline* p, double out[4]);     /* hpp:81 */
rip_status rip_get_dist_camera_matrix(const rip_pipeline* p, double out[9]);          /* hpp:121 */
rip_status rip_get_dist_distortion_coefficients(const rip_pipeline* p, double out[4]);/* hpp:122 */
rip_status rip_get_dist_rectification_matrix(const rip_pipeline* p, double out[9]);   /* hpp:123 */
rip_status rip_get_dist_projection_matrix(const rip_pipeline* p, double out[12]);     /* hpp:124 */
rip_status rip_get_rect_camera_matrix(const rip_pipeline* p, double out[9]);          /* hpp:129 */
rip_status rip_get_rect_distortion_coefficients(const rip_pipeline* p, double out[4]);/* hpp:130 */
rip_status rip_get_rect_rectification_matrix(const rip_pipeline* p, double out[9]);   /* hpp:131 */
rip_status rip_get_rect_projection_matrix(const rip_pipeline* p, double out[12]);     /* hpp:132 */
/* Not in the reference: the distortion coefficients in the length the model reports -- *n = 5 for plumb_bob and radtan, 8 for
 * rational_polynomial, 4 for every other model (what the two 4-value getters above return, unchanged).  rect = 0: the
 * coefficients of the distorted camera as the model evaluates them (radtan: k3 = 0); rect = 1: those of the rectified
 * image, n zeros once the undistortion has been initialised.  out = NULL just queries n; RIP_ERR_CAPACITY when
 * capacity < n. */
rip_status rip_get_distortion_coefficients_n(const rip_pipeline* p, int rect, double* out, int capacity, int* n);

/* ---- introspection used by tests / bench (no reference counterpart) --------------------------- */
/* Host copy of the undistortion maps (float32, map_rows x map_cols each); NULL pointers
 * just query the size. */
rip_status rip_get_undistortion_maps(rip_pipeline* p, float* map_x, float* map_y, size_t capacity_floats,
                                     int* map_rows, int* map_cols);
/* Per-frame white-balance results of the most recent device batch (D2H, synchronises):
 * for frame f, out[f*8 ..] = {gain_b, gain_g, gain_r, q8_b, q8_g, q8_r, uv_x, uv_y}. */
rip_status rip_get_white_balance_info(rip_pipeline* p, float* out, int n_frames);
/* The ccc estimator's track over the most recent device batch (D2H, synchronises): for frame f,
 * out[f*4 ..] = {raw_x, raw_y, x, y} -- the argmax of the response (convolutional_color_constancy.cpp:283-299) and the
 * position after the temporal filter that the gains were taken at (:300-340); equal without temporal consistency. */
rip_status rip_get_ccc_track(rip_pipeline* p, int* out, int n_frames);
/* Per-kernel-class timing with HIP events recorded on the handle's stream around each launch
 * (what bench.py's roofline leg reads).  rip_profile_begin arms up to max_records event pairs;
 * rip_profile_end synchronises the stream and returns, per class, the summed elapsed
 * milliseconds and the number of launches recorded. */
enum { RIP_KERNEL_STATS = 0, RIP_KERNEL_CCC = 1, RIP_KERNEL_CHAIN = 2, RIP_KERNEL_REMAP = 3, RIP_KERNEL_COUNT = 4 };
rip_status rip_profile_begin(rip_pipeline* p, int max_records);
rip_status rip_profile_end(rip_pipeline* p, double ms_sum[4], int count[4]);
/* Host-built tables the kernels use (same ids as oracle ripo_table, plus 8: gamma LUT). */
int rip_get_table(rip_pipeline* p, int which, int32_t* out, int capacity);
/* The vignetting mask plane the kernels multiply L by (VignettingCorrectionModule::precomputeVignettingMask,
 * vignetting_correction.cpp:32-63) for a rows x cols frame with the handle's current scale / a2 / a4:
 * rows * cols floats, row-major.  Host computation only; works on RIP_DEVICE_NONE handles. */
rip_status rip_get_vignetting_mask(rip_pipeline* p, int rows, int cols, float* out, size_t capacity_floats);
/* Test hook: the double-double atan the device map builder uses (rip_maps.hip), evaluated on the device for n doubles;
 * the parity tests compare it with libm's over the range fisheye maps reach. */
rip_status rip_debug_atan(rip_pipeline* p, const double* in, double* out, int n);
/* Test hook: the compiled remap plan of the current geometry (compiled now if it is not yet): info = {tiles_x, tiles_y,
 * border pixels, largest LDS footprint of a tile's source rectangle in bytes, largest rectangle width, height, 1 if the
 * plan was compiled on the device, tile width, tile height}.  Needs a loaded calibration and a device. */
rip_status rip_debug_plan_info(rip_pipeline* p, int src_rows, int src_cols, int info[9]);
/* Test hook: the launch record.  While on, every kernel launch of the product path made by a call on this handle (frames,
 * batches, the lazily built maps / plan / tables; not the re-runs of the debug stage dumps, not the probes) appends one line
 *   <kernel> fc=<0|1> grid=<x>,<y> block=<threads> frames=<n>
 * <kernel>: the kernel's name with its template arguments as a demangler prints them, without namespaces, e.g.
 * "chain_fast_kernel<7, 1, 512, false>" (the output stage: "output_convert_kernel<RgbChwF16>", one launch per batch slice); fc: the floating-point model it was compiled under (rip_set_fp_contraction; the
 * twins share a name); frames: the batch the launch serves (0 for the map, plan and table builders).  enable != 0 clears the
 * log and switches it on, 0 switches it off and keeps the text.  Off, a launch pays one null test. */
rip_status rip_debug_launch_log(rip_pipeline* p, int enable);
/* The record as NUL-terminated text.  *needed (optional) receives the bytes it takes, terminator included; a smaller
 * capacity returns RIP_ERR_CAPACITY and copies nothing. */
rip_status rip_debug_get_launch_log(rip_pipeline* p, char* out, size_t capacity, size_t* needed);
/* Test hook: the part of a src_rows x src_cols intermediate image the undistortion reads, as the fused Bayer chain kernel
 * walks it in front of the remap (items of 4 x 2 pixels in its input's coordinates, flipped by flip_angle, 0 or 180):
 * info = {items of the whole frame, items in the footprint, row pairs with a footprint, items per frame the last chain
 * launch of this handle walked (0 before the first)}.  intervals (optional, capacity_pairs >= src_rows / 2): per row pair of
 * the chain's input the items [lo, hi) it walks, (0, 0) for none.  Works on RIP_DEVICE_NONE handles (footprint of the
 * host-built maps); on device handles it compiles the plan as a frame would. */
rip_status rip_debug_chain_footprint(rip_pipeline* p, int src_rows, int src_cols, int flip_angle, int info[4], int* intervals,
                                     int capacity_pairs);
/* Test hook: the narrowing of rip_set_debayer_16bit_range on n values, computed on the host with the launch constants and the
 * arithmetic of the kernel (a multiplication and two shifts instead of the division).  No device, no handle. */
rip_status rip_debug_raw16_narrow(int black, int white, const uint16_t* in, uint8_t* out, size_t n);
/* Test hook: unpacks a packed Bayer frame (rip_apply "Packed Bayer frames": the encoding names the layout; rows of `step`
 * bytes, 0 = tight) into rows x cols uint16 samples, tightly packed, on the host with the extract functions the kernel's byte
 * path uses.  Width rule and pitch check as for rip_apply.  No device, no handle. */
rip_status rip_debug_unpack(const char* encoding, const uint8_t* in, size_t step, int rows, int cols, uint16_t* out);
/* Test hook: the table of a planar output format (rip_set_output_normalization) for the given normalisation: 3 x 256 elements
 * of the format's element type (float, or the uint16 bit patterns of f16 / bf16), plane-major, written to out.  rgb8, mono8 and
 * native have no table: RIP_ERR_INVALID_ARGUMENT, as for an unknown name or an invalid normalisation.  No device, no handle. */
rip_status rip_debug_output_table(const char* name, double divisor, const double mean[3], const double std[3], void* out);
/* Test hook: the tables of the resize stage (rip_set_output_size) from a src_rows x src_cols image to dst_rows x dst_cols, every
 * side in 1..16384 (RIP_ERR_INVALID_ARGUMENT otherwise, or for a null table): xofs[dst_cols] the first tap's column, alpha[2 *
 * dst_cols] the two weights of a column, yofs[2 * dst_rows] the two clamped rows, beta[2 * dst_rows] the two weights of a row,
 * *area2 (optional) = 1 when the 2 x 2 mean replaces them.  No device, no handle. */
rip_status rip_debug_resize_tables(int src_rows, int src_cols, int dst_rows, int dst_cols, int32_t* xofs, int16_t* alpha, int32_t* yofs,
                                   int16_t* beta, int* area2);
/* Test hook: the tables of the resize stage under the "area" interpolation (rip_set_output_interpolation) from a src_rows x src_cols
 * image to dst_rows x dst_cols: every side in 1..16384, no axis enlarged, no factor above 256 (RIP_ERR_INVALID_ARGUMENT otherwise, or
 * for a null table).  Output column x reads the xcount[x] >= 1 consecutive source columns from xfirst[x] on; their float weights
 * follow each other in xweight in output order (those of column x start at the sum of xcount[0 .. x)); xfirst / xcount: dst_cols
 * entries, xweight: room for src_cols + 2 * dst_cols.  Rows alike in yfirst / ycount / yweight.  *whole (optional) = 1 when both
 * factors are whole numbers other than the identity and 2 x 2 -- the kernel then sums blocks and multiplies by *scale (optional) =
 * 1.f / (ky * kx) -- else 0 and *scale = 0.  No device, no handle. */
rip_status rip_debug_resize_area_tables(int src_rows, int src_cols, int dst_rows, int dst_cols, int32_t* xfirst, int32_t* xcount, float* xweight,
                                        int32_t* yfirst, int32_t* ycount, float* yweight, int* whole, float* scale);
/* Test hook: the tables of the resize stage under "linear_aa" or "cubic_aa" (`name`; rip_set_output_interpolation) from a
 * src_rows x src_cols image of `channels` (1 or 3) channels to dst_rows x dst_cols: every side in 1..16384, no factor above 64
 * (RIP_ERR_INVALID_ARGUMENT otherwise, or for another name or a null table).  Output column x reads the xcount[x] >= 1 consecutive
 * source columns from xfirst[x] on; their int16 weights round(w * 2^*xprec) follow each other in xweight in output order, those of
 * column x from xwofs[x] on; xfirst / xcount / xwofs: dst_cols entries, xweight: room for 2 * S * max(src_cols, dst_cols) + dst_cols
 * with S = 1 ("linear_aa") or 2 ("cubic_aa").  Rows alike.  *tile_rows: the kernel's tile height (8, 4, 2 or 1) for that channel
 * count, *lds_rows: the source rows its LDS image holds.  xwofs, ywofs and the last four pointers may be null.  No device, no handle. */
rip_status rip_debug_resize_aa_tables(const char* name, int src_rows, int src_cols, int dst_rows, int dst_cols, int channels, int32_t* xfirst,
                                      int32_t* xcount, int32_t* xwofs, int16_t* xweight, int32_t* yfirst, int32_t* ycount, int32_t* ywofs,
                                      int16_t* yweight, int* xprec, int* yprec, int* tile_rows, int* lds_rows);
/* Test hook: the geometry of the resize stage with a window and a fit mode (PARITY.md "Resize: window and fit") for a final image
 * of cols x rows: roi_xywh as for rip_set_output_roi, (width, height) as for rip_set_output_size, fit as for rip_set_output_fit;
 * src_xywh / dst_xywh as rip_get_output_window gives them.  RIP_ERR_INVALID_ARGUMENT for what those setters refuse, a window outside
 * the image or a null pointer.  No device, no handle. */
rip_status rip_debug_output_window(int cols, int rows, const int roi_xywh[4], int width, int height, const char* fit, int src_xywh[4],
                                   int dst_xywh[4]);
/* Test hook for the debug dumps: writes image (rows x cols x channels bytes, channels 1 or 3 = BGR) to path as the PNG
 * writer of rip_set_debug does, after the reference's min-max normalisation when normalize != 0.  No device needed;
 * p may be NULL. */
rip_status rip_debug_write_png(rip_pipeline* p, const char* path, const uint8_t* image, int rows, int cols, int channels, int normalize);
/* Launch tunables of this handle (development / test hook; no reference counterpart).  The library reads its environment
 * overrides once, in rip_create(); this sets one of them afterwards.  Names: "chain_blocks", "chain_frames", "stats_blocks",
 * "remap_ring", "remap_stages", "remap_per_cu", "remap_frames", "remap_tiled", "ccc_lds_hist_min", "overlap_groups";
 * value 0 restores the built-in default where the tunable has one.  Unknown names: RIP_ERR_INVALID_ARGUMENT. */
rip_status rip_set_tunable(rip_pipeline* p, const char* name, int value);
/* Streaming microbenchmarks on the handle's device and stream (measurement hook, no reference counterpart): what this box's
 * memory system delivers to the access shapes the pipeline's kernels are made of -- bench.py reports them as
 * roofline.empirical beside the 8 TB/s spec figure.  `bytes` = size of the source stream (of the destination for FILL),
 * rounded down to a multiple of 48; the call allocates its buffers, runs one warm-up launch and `reps` timed ones (HIP events
 * on the handle's stream) and returns the BEST launch as GB/s (1e9) of bytes moved, read + written. */
enum {
  RIP_PROBE_COPY = 0,        /* 16 B per lane in, 16 B out (1 : 1) */
  RIP_PROBE_READ = 1,        /* 16 B per lane in, one dword per wave out */
  RIP_PROBE_FILL = 2,        /* 16 B per lane out */
  RIP_PROBE_EXPAND13 = 3,    /* 4 B per lane in, 12 B out: the fused chain's shape */
  RIP_PROBE_EXPAND13_NT = 4, /* the same with non-temporal stores (how the chain writes an image nothing reads again) */
  RIP_PROBE_COPY12 = 5,      /* 12 B per lane in and out: the remap's store shape fed by a contiguous read */
  RIP_PROBE_EXPAND13_WIDE = 6,    /* 16 B per lane in, 48 contiguous B out (three 16-byte stores) */
  RIP_PROBE_EXPAND13_WIDE_NT = 7, /* the same with non-temporal stores */
  RIP_PROBE_READ_NT = 8,          /* read only, eight 16-byte non-temporal loads in flight per lane */
  RIP_PROBE_EXPAND13_COALESCED = 9,    /* 16 B per lane in, three 16-byte stores out, each store instruction of a wave contiguous (1 KB) */
  RIP_PROBE_EXPAND13_COALESCED_NT = 10 /* the same with non-temporal stores */
};
rip_status rip_debug_hbm_probe(rip_pipeline* p, int kind, size_t bytes, int reps, double* gbps);
const char* rip_version(void);

#ifdef __cplusplus
}
#endif
#endif
