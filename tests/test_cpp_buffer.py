"""The owner of mapped page-locked memory (MappedBuf, bayesiannetwork_amd/csrc/bn_buffer.hpp) checked stand-alone on a CPU:
tests/cpp/test_buffer.cpp includes the header and defines the four HIP calls it makes itself, over malloc / free, so the program
links without the HIP runtime.  It is run as a program of its own, once plainly and once under AddressSanitizer and
UndefinedBehaviorSanitizer.  It checks that a failed allocation and a failed mapping leave the object empty with the block held
before freed exactly once, that the next reserve of the same size allocates again, reserve's growth policy, alloc(0), and that moves
carry host pointer, device alias and capacity and leave the source empty."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesiannetwork_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_mapped_buffer_owner(tmp_path, sanitize):
    exe = str(tmp_path / "test_buffer")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", *flags, "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", CSRC,
           os.path.join(ROOT, "tests", "cpp", "test_buffer.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.stdout.startswith("ok: "), out.stdout
    print(out.stdout.strip())
