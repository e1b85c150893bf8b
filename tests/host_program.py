"""The one builder and runner of the stand-alone host programs under tests/c_abi/: a host compiler, AddressSanitizer and
UBSan linked statically, a stand-alone executable started with subprocess.run -- nothing is preloaded and no environment
is set.  The *_host tests build their program with build() and start it with run()."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bc_gym_planning_env_amd", "csrc")
# numpy rounds every product and sum on its own: programs that are compared bit for bit with a numpy reference take these
ROUND_EACH = ("-O1", "-ffp-contract=off")


def compiler():
    for cand in ("g++", "/opt/rocm/llvm/bin/clang++", "clang++"):
        path = shutil.which(cand)
        if path:
            return path
    raise AssertionError("no host C++ compiler found (g++ or ROCm's clang++)")


def command(exe, source, includes=(CSRC,), extra_flags=(), opt=ROUND_EACH):
    """The compiler's command line.  source: a file of tests/c_abi/; opt: flags ahead of the sanitizers', extra_flags: flags
    behind them, ahead of one -I per directory of `includes`."""
    cxx = compiler()
    static_runtime = ["-static-libasan", "-static-libubsan"] if cxx.endswith("g++") else []   # (clang's is static already)
    return ([cxx] + static_runtime + ["-std=c++17", "-Wall", "-Werror", "-g"] + list(opt) +
            ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + list(extra_flags) +
            ["-I" + d for d in includes] + [os.path.join(ROOT, "tests", "c_abi", source), "-o", exe])


def build(tmp_path_factory, source, includes=(CSRC,), extra_flags=(), opt=ROUND_EACH):
    """-> the executable built from tests/c_abi/<source>, in a directory of its own"""
    stem = os.path.splitext(source)[0]
    exe = str(tmp_path_factory.mktemp(stem[:-len("_main")] if stem.endswith("_main") else stem) / stem)
    built = subprocess.run(command(exe, source, includes, extra_flags, opt), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           universal_newlines=True, timeout=300)
    assert built.returncode == 0, built.stdout
    return exe


def run(exe, args=(), ok_line=None, timeout=120):
    """Starts the program; it must end with status 0, print ok_line (if one is given) and nothing of a sanitizer's.
    -> the lines of its output"""
    ran = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True,
                         timeout=timeout)
    assert ran.returncode == 0, ran.stdout[-4000:]
    if ok_line is not None:
        assert ok_line in ran.stdout
    for word in ("Sanitizer", "runtime error"):
        assert word not in ran.stdout, ran.stdout[-4000:]
    return ran.stdout.split("\n")
