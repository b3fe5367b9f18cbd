"""The pure-host pieces of the stream and torus layer (csrc/sn_stream_groups.hpp: the grouping of a slice, its commit, the pose
rule) run as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer, against the restatement inside
csrc/compat/test/stream_groups_check.cpp.  No GPU and no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPAT = os.path.join(ROOT, "hobot_stereonet_amd", "csrc", "compat")


def test_stream_groups_check_runs_clean_under_the_sanitizers():
    subprocess.check_call(["make", "-C", COMPAT, "-s", "build/stream_groups_check"])
    run = subprocess.run([os.path.join(COMPAT, "build", "stream_groups_check")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "stream_groups_check: ok" in run.stdout

