"""The rules units of the planner stages (csrc/rplgpu_nav_rules.cpp, rplgpu_rollout_rules.cpp, rplgpu_mppi_rules.cpp,
rplgpu_frontier_rules.cpp: E26 - E29) are plain C++, and the one stand-alone program that drives all four accepts every
call it should.  No sanitizer here: tools/dev/plan_rules_asan.cpp's header has that recipe."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "rplidar_ros2_driver_amd" / "csrc"
STAGES = ("nav", "rollout", "mppi", "frontier")


def test_plan_rules_units_are_plain_cpp(tmp_path):
    """The four rules units and tools/dev/plan_rules_asan.cpp build with the system g++ from those five files alone,
    warning-free; the program exits 0 and prints a line per part."""
    rules = [CSRC / f"rplgpu_{s}_rules.cpp" for s in STAGES]
    for unit in rules:
        text = unit.read_text()
        assert "hip/hip_runtime" not in text and "rpl_launch.hpp" not in text, unit.name
    exe = tmp_path / "plan_rules"
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
           f"-I{ROOT / 'include'}", f"-I{CSRC}", *map(str, rules),
           str(ROOT / "tools" / "dev" / "plan_rules_asan.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    for part in ("E26 nav rules", "E27 rollout rules", "E28 mppi rules", "E29 frontier rules"):
        assert f"{part}: passed" in lines, r.stdout
    assert lines[-1] == "all parts passed"
