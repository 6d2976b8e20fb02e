"""csrc/common.cpp on the host: next_pow2 and the (kernel, device) table of allow_big_lds, in a stand-alone program
(tests/host/common_host_check.cpp, the two HIP calls stubbed).  No GPU.  This is the plain build; the same program under
AddressSanitizer and UBSan is `tools/common_host_check.sh`, run by hand on a CPU machine."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_allow_big_lds_and_next_pow2():
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "common_host_check.sh")], env=dict(os.environ, CXXFLAGS=""),
                         capture_output=True, text=True)
    assert out.returncode == 0 and "common_host_check: ok" in out.stdout, out.stdout + out.stderr
