"""The region geometry of the compact counter-key streams
(cilium_amd/csrc/classify.hpp key_per_block / key_regions), which the IPv4
classify kernel, k_hist and the workspace sizing share: a host program
(tests/c/key_geom_host.cpp) checks, for batch sizes around the wave, workgroup
and device boundaries and for narrow and wide devices, that the regions are
disjoint, inside the sized array, hold every position their wave handles, and
that the count array covers every region.  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_key_region_geometry(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert shutil.which(hipcc), "the HIP compiler the library is built with"
    exe = str(tmp_path / "key_geom_host")
    subprocess.run([hipcc, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function",
                    "-I", os.path.join(ROOT, "cilium_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "c", "key_geom_host.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "key_geom_host: ok" in r.stdout, r.stdout + r.stderr
