"""The signature window of the source-init kernel (csrc/init_sig.h: clipping at the grid's edges,
grids smaller than the window, the cells' order) run on the host under ASan and UBSan
(tests/init_sig_sim.cpp): sources at the four corners and on each edge, grids of 7 x 40 and 20 x 20,
exact_r 0, 20 and 48; every index in range, the cell count that of the clipped rectangle, the
order deterministic."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ali-fmm-and-ray-tracing_amd", "csrc")


def test_init_sig_window_under_sanitizers(tmp_path):
    exe = str(tmp_path / "init_sig_sim")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, os.path.join(HERE, "init_sig_sim.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
