"""The exact walks' shared heap and small rules (csrc/walk_heap.h, csrc/walk_rules.h) run on the host
under ASan and UBSan (tests/walk_heap_sim.cpp): the integer parent against rint(t / 2) up to 2^20;
seeded FMM-shaped sequences on 9 x 9, 16 x 16 and 7 x 40 grids through a plain live-key heap on
ttn / nsts / btg and through the shared heap with each of its three stores, compared slot by slot
and node by node after every operation; the overflow and dup-cap errors at small capacities; and
the stencil, hand-over, neighbour-order and guess rules against literals.  The sim counts the
events that make the comparison mean something; every count must be above zero."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ali-fmm-and-ray-tracing_amd", "csrc")
EVENTS = ("second_add", "sync_multi", "pop_first", "pop_second", "tail", "root", "err_full", "err_dup")


def test_walk_heap_under_sanitizers(tmp_path):
    exe = str(tmp_path / "walk_heap_sim")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, os.path.join(HERE, "walk_heap_sim.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
    counts = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", r.stdout)}
    assert set(counts) == set(EVENTS), r.stdout
    assert all(counts[k] > 0 for k in EVENTS), r.stdout
