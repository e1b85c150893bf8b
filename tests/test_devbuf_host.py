"""DevBuf<T> (csrc/bcp_devbuf.h), the owner of every device buffer of the handle, as a stand-alone host program under
AddressSanitizer and UBSan: tests/c_abi/devbuf_main.cpp puts malloc / free behind hipMalloc / hipFree and links no HIP
library, so what it proves -- growth, reuse, the state after a failed allocation, and every block given back (the leak
check at exit) -- needs no GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for cand in ("g++", "/opt/rocm/llvm/bin/clang++", "clang++"):
        path = shutil.which(cand)
        if path:
            return path
    raise AssertionError("no host C++ compiler found (g++ or ROCm's clang++)")


def test_devbuf_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "devbuf_main")
    cxx = _compiler()
    static_runtime = ["-static-libasan", "-static-libubsan"] if cxx.endswith("g++") else []   # (clang's is static already)
    cmd = [cxx] + static_runtime + ["-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "bc_gym_planning_env_amd", "csrc"),
           os.path.join(ROOT, "tests", "c_abi", "devbuf_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=60)
    assert ran.returncode == 0, ran.stdout
    assert "devbuf ok" in ran.stdout
    for word in ("Sanitizer", "runtime error"):
        assert word not in ran.stdout, ran.stdout
