"""The plan of a map binding (csrc/bcp_field_plan.h: the footprint geometry behind the distance-field classification, and
every shape and size bcp_set_costmaps derives from a binding) as a stand-alone host program under AddressSanitizer and
UBSan: tests/c_abi/field_plan_main.cpp includes that header alone -- it has no HIP in it -- and checks the geometric
claims (outer discs cover the footprint, inner discs lie inside it), the sizes, a table of full plans recorded before
the plan was split off, and the refusal of an oversized footprint, without a GPU."""
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


def test_field_plan_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "field_plan_main")
    cxx = _compiler()
    static_runtime = ["-static-libasan", "-static-libubsan"] if cxx.endswith("g++") else []   # (clang's is static already)
    cmd = [cxx] + static_runtime + ["-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "bc_gym_planning_env_amd", "csrc"),
           os.path.join(ROOT, "tests", "c_abi", "field_plan_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=60)
    assert ran.returncode == 0, ran.stdout
    assert "field plan ok" in ran.stdout
    for word in ("Sanitizer", "runtime error"):
        assert word not in ran.stdout, ran.stdout
