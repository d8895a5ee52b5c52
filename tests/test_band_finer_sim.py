"""The CPU band model of travel_finer_grid (oracle/band_model.c oband_travel_finer: stage windows
clipped at the grid's edges, the hand-overs, the prefix, the band's lists) run stand-alone on the host
under ASan and UBSan (tests/band_finer_sim.c): 2 x 2 at subgrid 9 from every corner, 12 x 9 with
corner and edge sources at subgrid 3 (with and without stiffness, the far band on and off), 4 x 5
at subgrid 11; every field finite and positive, the refused calls refused."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE = os.path.join(os.path.dirname(HERE), "oracle")


def test_band_finer_model_under_sanitizers(tmp_path):
    exe = str(tmp_path / "band_finer_sim")
    subprocess.run(["gcc", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "band_finer_sim.c"),
                    os.path.join(ORACLE, "band_model.c"), "-o", exe, "-lm", "-lpthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
