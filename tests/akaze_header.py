"""Builds tests/cpp/akaze_plan.cpp -- a host program over sfmlocalization_amd/csrc/akaze_plan.h, the header the library
plans and launches by -- runs it over a list of requests and parses what it prints: the header's constants, and per
request the plan, the detection record and the evolution steps for every number of levels a call can build."""
import os
import shutil
import subprocess
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

Detect = namedtuple("Detect", "rows segs_per_row n_seg seg_chunks scan_two_launches hist_grid_x grad_grid_y hist_grid_y "
                              "nbr_grid desc_grid cand_cap spec_start spec_max")
Step = namedtuple("Step", "resident first last halfsample source fuse n_launch")
# levels: [([w, h, octave, sublevel, sigma_size, nsteps, off], step-time bits)]; evo: {need: (levels built, [Step])}
Plan = namedtuple("Plan", "kind total levels detect evo")
Refused = namedtuple("Refused", "kind level steps")


def build(directory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        raise RuntimeError("no host C++ compiler (g++ / c++) to build tests/cpp/akaze_plan.cpp")
    exe = os.path.join(str(directory), "akaze_plan")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "akaze_plan.cpp")],
                   check=True, timeout=300)
    return exe


def run(exe, requests):
    """-> (constants {name: int}, {(w, h, n_octaves, n_sublevels): Plan or Refused})"""
    r = subprocess.run([exe] + [str(v) for q in requests for v in q], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    constants, plans, cur = None, {}, None
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "constants":
            constants = {k: int(v) for k, v in zip(f[1::2], f[2::2])}
        elif f[0] == "plan":
            cur = Plan("plan", int(f[6]), [], [], {})
            plans[tuple(int(v) for v in f[1:5])] = cur
            assert int(f[5]) >= 1
        elif f[0] == "refused":
            plans[tuple(int(v) for v in f[1:5])] = Refused("refused", int(f[5]), int(f[6]))
        elif f[0] == "level":
            assert int(f[1]) == len(cur.levels)
            cur.levels.append(([int(v) for v in f[2:9]], np.array([int(v, 16) for v in f[9:]], np.uint32)))
        elif f[0] == "detect":
            cur.detect.append(Detect(*[int(v) for v in f[1:]]))
        elif f[0] == "evo":
            steps, n_steps = [], int(f[3])
            cur.evo[int(f[1])] = (int(f[2]), steps, n_steps)
        else:
            assert f[0] == "step", line
            steps.append(Step(bool(int(f[1])), int(f[2]), int(f[3]), bool(int(f[4])), f[5], int(f[6]), int(f[7])))
    for q, p in plans.items():
        if p.kind == "plan":
            assert len(p.detect) == 1 and sorted(p.evo) == list(range(1, len(p.levels) + 1))
            assert all(len(steps) == n_steps for _, steps, n_steps in p.evo.values())
            plans[q] = p._replace(detect=p.detect[0], evo={need: v[:2] for need, v in p.evo.items()})
    assert constants is not None and set(plans) == set(requests)
    return constants, plans
