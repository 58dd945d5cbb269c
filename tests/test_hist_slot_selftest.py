"""The host self-test's case for the 32-bit histogram slot (classify.hpp
HistSlot, the arithmetic k_hist and k_hist_reduce share): adversarial
length sequences replayed on one slot, recombined sums against plain u64
sums.  No GPU needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hist_slot_case_runs_and_passes():
    csrc = os.path.join(ROOT, "cilium_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-s", "selftest"], check=True)
    r = subprocess.run([os.path.join(csrc, "build", "selftest")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("hist slot")]
    assert len(lines) == 1 and lines[0].endswith(" ok"), r.stdout
