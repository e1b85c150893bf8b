"""The route decision of the egocentric observation (csrc/bcp_ego_route.h: which kernel a call's shape and the cell-list
facts lead to, the launch shape that goes with it, the sparse route's limit) as a stand-alone host program under
AddressSanitizer and UBSan: tests/c_abi/ego_route_main.cpp includes that header alone -- it has no HIP in it -- and checks
the table of routes, so a router that sent every call to one kernel fails here, without a GPU."""
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


def test_ego_route_table_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "ego_route_main")
    cxx = _compiler()
    static_runtime = ["-static-libasan", "-static-libubsan"] if cxx.endswith("g++") else []   # (clang's is static already)
    cmd = [cxx] + static_runtime + ["-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "bc_gym_planning_env_amd", "csrc"),
           os.path.join(ROOT, "tests", "c_abi", "ego_route_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=60)
    assert ran.returncode == 0, ran.stdout
    assert "ego route ok" in ran.stdout
    for word in ("Sanitizer", "runtime error"):
        assert word not in ran.stdout, ran.stdout
