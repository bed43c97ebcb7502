"""Builds librip_hip.so (the C-ABI library, include/rip.h) and its kernel libraries -- the table KERNEL_LIBRARIES below: the kernels
of the output stage, the four libraries of the resize stage, the output heads' copy, the valid-pixel masks, the YUV 4:2:0 formats,
CLAHE and the JPEG encoder -- for gfx950 with hipcc.

In-tree build: the .so lands next to this file so it travels with the repo snapshot.
-ffp-contract=off is part of the numerical contract (OpenCV's separate float mul/add)."""
import collections
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "librip_hip.so")
SOURCES = ["rip_chain.hip", "rip_stats.hip", "rip_ccc.hip", "rip_remap.hip", "rip_maps.hip", "rip_fused.hip", "rip_probe.hip", "rip_demosaic.hip", "rip_raw16.hip", "rip_packed.hip", "rip_yaml.cpp", "rip_params.cpp", "rip_output_tables.cpp", "rip_color_tables.cpp", "rip_undistort.cpp", "rip_ccc_model.cpp", "rip_png.cpp", "rip_plan.cpp", "rip_constants.cpp", "rip_batch.cpp", "rip_output_stage.cpp", "rip_ring.cpp", "rip_settings.cpp", "rip_api.cpp"]  # compiled in parallel
HEADERS = ["rip_kernels.hpp", "rip_device.hpp", "rip_chain_dev.hpp", "rip_remap_dev.hpp", "rip_tile_deal.hpp", "rip_round_map.hpp", "rip_tile.hpp", "rip_raw16_dev.hpp", "rip_unpack.hpp", "rip_host.hpp", "rip_launch_info.hpp", "rip_yaml.hpp", "rip_params.hpp", "rip_output_tables.hpp", "rip_color_tables.hpp", "rip_undistort.hpp", "rip_ccc_model.hpp", "rip_png.hpp", "rip_handle.hpp", "rip_output.hpp", "rip_resize.hpp", "rip_area.hpp", "rip_fit.hpp", "rip_aa.hpp", "rip_heads.hpp", "rip_mask.hpp", "rip_yuv.hpp", "rip_clahe.hpp", "rip_jpeg.hpp", os.path.join("..", "..", "include", "rip.h")]
# The kernel libraries: kernels behind one header each, in libraries of their own so that librip_hip.so's kernel table stays
# what tests/variant_cases.py closes over; each library's table is closed by a tests/*_variant_cases.py of its own.
# librip_hip.so -- every build of it: the default one, the sanitizer build and the A/B variants under variants/ -- links against
# these files, in the table's order, and finds them through its $ORIGIN rpath.  A library's interface is its headers alone, so a
# rebuild of it does not ask for a relink of the libraries that use it.  One row each, closed by tests/test_kernel_libraries.py:
#   out    the output stage's kernels (rip_set_output_format) and their one launch function; tests/output_variant_cases.py
#   rsz    the resize stage's kernels (rip_set_output_size); tests/resize_variant_cases.py
#   area   the resize stage's area interpolation (rip_set_output_interpolation); tests/area_variant_cases.py
#   fit    the resize stage's kernels that read a window of the image, and the pad kernel of the letterbox (rip_set_output_roi,
#          rip_set_output_fit); rip_fit.hpp takes its parameter structs from the two headers before it; tests/fit_variant_cases.py
#   aa     the resize stage's antialiased filters (rip_set_output_interpolation "linear_aa" / "cubic_aa"), whole frame and window;
#          its device code is rip_aa_dev.hpp; tests/aa_variant_cases.py
#   heads  head_copy_kernel, the copy that delivers F to a further head that asks for it as it is (rip_apply_device_heads);
#          tests/heads_variant_cases.py
#   mask   rect_mask_kernel, the coverage mask of an undistortion from its maps alone, and mask_threshold_kernel (rip_set_rect_mask,
#          rip_get_output_mask); rip_round_map.hpp is the map quantiser it shares with the remap kernels; tests/mask_variant_cases.py
#   yuv    yuv420_kernel<true / false>, the delivered BGR picture as nv12 / i420 (rip_set_output_format, rip_set_output_yuv_matrix);
#          tests/yuv_variant_cases.py
#   clahe  clahe_lut_kernel and clahe_apply_kernel, cv::CLAHE of a delivered one-channel picture (rip_set_output_clahe); its device
#          code is rip_clahe_dev.hpp; tests/clahe_variant_cases.py
#   jpeg   jpeg_transform_kernel<true / false>, jpeg_size_kernel, jpeg_scan_kernel and jpeg_write_kernel, the delivered picture as a
#          baseline JPEG stream (rip_set_output_format "jpeg", rip_set_output_jpeg); its device code is rip_jpeg_dev.hpp, and it takes
#          the matrix struct of rip_yuv.hpp; tests/jpeg_variant_cases.py
# rip_resize_dev.hpp is the device code and the launch checks the libraries of the resize stage share; rip_launch_info.hpp is the
# launch record every launch function fills.
KernelLibrary = collections.namedtuple("KernelLibrary", "key out sources headers build_dir")
RESIZE_SHARED = ["rip_resize_dev.hpp", "rip_resize.hpp", "rip_area.hpp"]
KERNEL_LIBRARIES = tuple(KernelLibrary(key, os.path.join(HERE, "librip_%s_hip.so" % key), sources, headers + ["rip_launch_info.hpp"], "build_" + key) for key, sources, headers in (
    ("out", ["rip_output.hip"], ["rip_output.hpp"]),
    ("rsz", ["rip_resize.hip"], RESIZE_SHARED),
    ("area", ["rip_area.hip"], RESIZE_SHARED),
    ("fit", ["rip_fit.hip"], ["rip_fit.hpp"] + RESIZE_SHARED),
    ("aa", ["rip_aa.hip"], ["rip_aa.hpp", "rip_aa_dev.hpp"] + RESIZE_SHARED),
    ("heads", ["rip_heads.hip"], ["rip_heads.hpp"]),
    ("mask", ["rip_mask.hip"], ["rip_mask.hpp", "rip_round_map.hpp"]),
    ("yuv", ["rip_yuv.hip"], ["rip_yuv.hpp"]),
    ("clahe", ["rip_clahe.hip"], ["rip_clahe.hpp", "rip_clahe_dev.hpp"]),
    ("jpeg", ["rip_jpeg.hip"], ["rip_jpeg.hpp", "rip_jpeg_dev.hpp", "rip_yuv.hpp"]),
))
# per-source additions.  rip_chain.hip: LLVM's max-ILP machine scheduler -- the fused chain is bound by VALU issue and LDS at
# six waves per SIMD and gains 2.3 % from the extra instruction-level parallelism inside a wave (2.311 -> 2.257 ms per 256
# frames); the same strategy costs the memory-bound remap 3.5 % and the ccc kernels 8 %, so it is not a global flag.
PER_SOURCE_FLAGS = {"rip_chain.hip": ["-mllvm", "-amdgpu-sched-strategy=" + os.environ.get("RIP_CHAIN_SCHED", "max-ilp")] if os.environ.get("RIP_CHAIN_SCHED", "max-ilp") != "default" else []}  # RIP_CHAIN_SCHED: A/B builds of other strategies (tools/ab_chain.py)
# translation units compiled a second time under the contracted floating-point model (rip_device.hpp RIP_FP_CONTRACT; object
# <name>_fc1.o): the kernels rip_set_fp_contraction(1) selects.  -ffp-contract stays off: the fused forms are written out.
FC1_SOURCES = ["rip_chain.hip", "rip_fused.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
         "-fvisibility=hidden", "-fno-slp-vectorize", "-Wall", "-Wno-unused-function", "-D__HIP_PLATFORM_AMD__"]


def hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    raise RuntimeError("hipcc not found")


def kernel_library(key):
    """The row of KERNEL_LIBRARIES with that key."""
    return next(c for c in KERNEL_LIBRARIES if c.key == key)


def kernel_library_up_to_date(key):
    c = kernel_library(key)
    if not os.path.exists(c.out):
        return False
    t = os.path.getmtime(c.out)
    deps = [os.path.join(CSRC, s) for s in c.sources + c.headers] + [os.path.abspath(__file__)]
    return all(os.path.getmtime(d) <= t for d in deps)


def kernel_libraries_up_to_date():
    return all(kernel_library_up_to_date(c.key) for c in KERNEL_LIBRARIES)


def up_to_date():
    if not os.path.exists(OUT) or not kernel_libraries_up_to_date():
        return False
    t = os.path.getmtime(OUT)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS] + [os.path.abspath(__file__)]
    return all(os.path.getmtime(d) <= t for d in deps)


def build_kernel_library(key, force=False, verbose=False):
    """One kernel library, next to librip_hip.so."""
    _, out, sources, _, bdir_name = kernel_library(key)
    if not force and kernel_library_up_to_date(key):
        return out
    bdir = os.path.join(HERE, bdir_name)
    os.makedirs(bdir, exist_ok=True)
    objs = []
    for s in sources:
        obj = os.path.join(bdir, os.path.splitext(s)[0] + ".o")
        cmd = [hipcc()] + FLAGS + os.environ.get("RIP_EXTRA_FLAGS", "").split() + ["-x", "hip", "-c", os.path.join(CSRC, s), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed on %s:\n%s" % (s, r.stdout))
        if verbose and r.stdout.strip():
            print(r.stdout)
        objs.append(obj)
    cmd = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,-soname," + os.path.basename(out), "-o", out] + objs
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("link failed:\n" + r.stdout)
    return out


# --asan: the HOST layer (every .cpp of SOURCES: YAML reader, loaders, table builders, frame ring, copy threads) under
# AddressSanitizer + UndefinedBehaviorSanitizer, compiled with g++ against GCC's runtimes; the device code is compiled by hipcc
# as always.  (Not clang's runtime: the ROCm build of compiler-rt intercepts hsa_amd_memory_pool_allocate for device-side ASan and
# aborts the first HIP allocation of a process on a GPU box -- "allocator is trying to allocate 0x400000 bytes" -- without
# xnack+ code objects.)  tools/README.md "Sanitizer build".
ASAN_OUT = os.path.join(HERE, "librip_hip_asan.so")
ASAN_HOST_CXX = os.environ.get("RIP_ASAN_CXX", "g++")
ASAN_HOST_FLAGS = ["-std=c++17", "-O1", "-g", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fvisibility=hidden", "-D__HIP_PLATFORM_AMD__",
                   "-I/opt/rocm/include", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined,float-cast-overflow",
                   "-fno-omit-frame-pointer", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"]


def _gcc_lib(name):
    r = subprocess.run([ASAN_HOST_CXX, "-print-file-name=" + name], stdout=subprocess.PIPE, text=True)
    return os.path.realpath(r.stdout.strip())


def asan_runtime():
    """Path of GCC's shared ASan runtime (the LD_PRELOAD a python process needs to load librip_hip_asan.so)."""
    return _gcc_lib("libasan.so")


def build(force=False, verbose=False, out=None, extra_flags=None, tag="", asan=False):
    """out / extra_flags / tag: A/B variants for experiments (tools/ab_chain.py), e.g. extra_flags=["-DRIP_X=1"],
    out=".../variants/x.so"; the default build takes no extra flags beyond $RIP_EXTRA_FLAGS."""
    if asan:
        out, tag = out or ASAN_OUT, tag or "_asan"
        if not force and os.path.exists(out) and kernel_libraries_up_to_date() and all(os.path.getmtime(os.path.join(CSRC, d)) <= os.path.getmtime(out) for d in SOURCES + HEADERS):
            return out
    if out is None and not force and up_to_date():
        return OUT
    for c in KERNEL_LIBRARIES:  # every build of librip_hip.so links against all of them; `force` is about the library asked for
        build_kernel_library(c.key, verbose=verbose)
    out = out or OUT
    objs = []
    procs = []
    bdir = os.path.join(HERE, "build" + tag)
    os.makedirs(bdir, exist_ok=True)
    for s, fc in [(s, 0) for s in SOURCES] + [(s, 1) for s in FC1_SOURCES]:
        obj = os.path.join(bdir, os.path.splitext(s)[0] + ("_fc1" if fc else "") + ".o")
        if asan and s.endswith(".cpp"):
            cmd = [ASAN_HOST_CXX] + ASAN_HOST_FLAGS + list(extra_flags or []) + ["-c", os.path.join(CSRC, s), "-o", obj]
        else:
            cmd = [hipcc()] + FLAGS + os.environ.get("RIP_EXTRA_FLAGS", "").split() + list(extra_flags or []) + PER_SOURCE_FLAGS.get(s, []) + (["-DRIP_FP_CONTRACT=1"] if fc else []) + ["-x", "hip", "-c", os.path.join(CSRC, s), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((s, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        objs.append(obj)
    for s, pr in procs:
        log, _ = pr.communicate()
        if pr.returncode != 0:
            raise RuntimeError("hipcc failed on %s:\n%s" % (s, log))
        if verbose and log.strip():
            print(log)
    # the kernel libraries are found next to the library ($ORIGIN) or one directory up (variants/*.so)
    kernel_libs = ["-L" + HERE] + ["-l:" + os.path.basename(c.out) for c in KERNEL_LIBRARIES] + ["-Wl,-rpath,$ORIGIN:$ORIGIN/.."]
    cmd = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs + kernel_libs + ([_gcc_lib("libasan.so"), _gcc_lib("libubsan.so"), "-lstdc++", "-lpthread"] if asan else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("link failed:\n" + r.stdout)
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True, asan="--asan" in sys.argv))
    if "--asan" in sys.argv:
        print("LD_PRELOAD=" + asan_runtime())
