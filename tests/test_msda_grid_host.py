"""csrc/msda_grid.h on the host: the region-grid chooser of the encoder window kernels in a stand-alone program
(tests/host/msda_grid_host_check.cpp: plain C++, no HIP header) -- never coarser than the windows allow, regions == nry * nrx, the
same answer twice and after eviction from the cache, eight levels accepted, nine levels / a side above 32766 / no CU count "no
table".  No GPU.  This is the plain build; the same program under AddressSanitizer and UBSan is `tools/msda_grid_host_check.sh`,
run by hand on a CPU machine."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_region_grid_chooser_alone():
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "msda_grid_host_check.sh")], env=dict(os.environ, CXXFLAGS=""),
                         capture_output=True, text=True)
    assert out.returncode == 0 and "msda_grid_host_check: ok" in out.stdout, out.stdout + out.stderr
