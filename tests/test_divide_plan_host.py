"""DivideRounds' host plan without a GPU (hgx_divide_plan_host.cpp: coordinate width, rebuild or resume,
the lowest round that can change, the first dirty lastAncestors unit, the lane map, the rebuilt layout's
slots, the round path): tools/divide_plan_check.cpp runs seeded sequences of calls against a direct
statement of each rule and must have met every kind of call."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_divide_plan_stand_alone_check(tmp_path):
    """The plan is plain C++ with no HIP and no context, so a program with its own main checks it
    (built here without a sanitizer; the same program is meant for -fsanitize=address,undefined)."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        assert os.path.exists(hipcc), "no C++ compiler found"
        cxx = hipcc
    exe = str(tmp_path / "divide_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "babble_amd", "csrc"),
                           os.path.join(ROOT, "tools", "divide_plan_check.cpp"),
                           os.path.join(ROOT, "babble_amd", "csrc", "hgx_divide_plan_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) sequences ok: (\d+) calls, rebuilds (\d+) first (\d+) width up (\d+) width down (\d+) outgrown "
                  r"(\d+) incremental off; resumed (\d+) r_lo above 0 (\d+) no old event (\d+) no growth; "
                  r"lane maps (\d+) fit (\d+) over; (\d+) layouts, (\d+) round-path combinations", r.stdout)
    assert m, r.stdout
    (seqs, calls, first, up, down, outgrown, inc_off, r_hi, no_old, no_growth, fit, over, layouts,
     combos) = map(int, m.groups())
    assert seqs >= 400 and calls >= seqs
    assert min(first, up, down, outgrown, inc_off, r_hi, no_old, no_growth, fit, over, layouts, combos) > 0
