"""DevBuf<T> (csrc/bcp_devbuf.h), the owner of every device buffer of the handle, as a stand-alone host program under
AddressSanitizer and UBSan: tests/c_abi/devbuf_main.cpp puts malloc / free behind hipMalloc / hipFree and links no HIP
library, so what it proves -- growth, reuse, the state after a failed allocation, and every block given back (the leak
check at exit) -- needs no GPU."""
import host_program


def test_devbuf_under_host_sanitizers(tmp_path_factory):
    exe = host_program.build(tmp_path_factory, "devbuf_main.cpp", opt=(), extra_flags=("-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"))
    host_program.run(exe, (), "devbuf ok", timeout=60)
