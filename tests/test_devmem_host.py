"""DevBuf / PinnedBuf, the owners of device and pinned memory (rgbd360_amd/csrc/host/devmem.h), without a GPU.

tests/host/devmem_check.cpp is a stand-alone program: it includes the library's internal header, supplies its own
hipMalloc / hipFree / hipHostMalloc / hipHostFree / hipMemsetAsync / hipStreamSynchronize / hipGetErrorString /
ctx_wait / r360_set_error (malloc-backed, with a live-allocation set, a "fail the k-th allocation" switch and a log
of the calls in order) and exits non-zero when an owner leaks, is left dangling by a failed reserve, calls the
allocator for a size it already holds, frees a live buffer without waiting first (or waits for an empty one), zeroes
on a no-op or fails to zero on growth, or frees after it was moved from.  It is compiled with g++ and the address and
undefined-behaviour sanitizers, with no HIP runtime linked, and run as its own process.

The same program links rgbd360_amd/csrc/host/handles.cpp, the memory part of the calibration, the frame, its plane
buffers and its sensor pyramid, and makes every allocator, event, copy and memset call of each creation fail in
turn: the creation returns non-zero with the error set, leaves nothing live and frees nothing twice, and then
succeeds and releases cleanly."""
import os
import subprocess


def test_devmem_owners_under_sanitizers(root, tmp_path):
    rocm = os.environ.get("ROCM") or os.environ.get("ROCM_PATH") or "/opt/rocm"   # the Makefile's ROCM
    exe = tmp_path / "devmem_check"
    p = subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-I{root}/rgbd360_amd/csrc",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-o", str(exe),
                        f"{root}/tests/host/devmem_check.cpp", f"{root}/rgbd360_amd/csrc/host/handles.cpp"],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "devmem ok", (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
