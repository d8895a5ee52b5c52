"""Time the K-member band kernel on C4 (128 sources, auto K; 16 sources, auto K) with the phase
profile, and fingerprint the fields (bit-identity across variants).  ALIFMM_LIB selects the library.
python tools/kbench.py NAME  -> one JSON line"""
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ali-fmm-and-ray-tracing_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import _alifmm  # noqa: E402
import workloads as W  # noqa: E402

PH = ["p1_x1", "accept_rim", "claim", "evaluate", "fallback", "commit"]
# BandSrc::sub: [X1 wait, rim read, XCD-local steps x 100, drain before X1]; with the / 100 / steps
# below the third is the fraction of steps whose exchange was XCD-local
SUB = ["x1_wait", "rim_read", "xcd_local_frac", "drain"]


def opt(ctx, name):
    """An option of the last call, None with a library (ALIFMM_LIB) that does not have it."""
    try:
        return round(ctx.get_option(name), 3)
    except _alifmm.AlifmmError:
        return None


def main():
    name = sys.argv[1]
    sizes = [int(a) for a in sys.argv[2:]] or [128, 16]
    ctx = _alifmm.Context(0)
    # ALIFMM_OPT_<NAME>=value options are applied by _alifmm.Context itself
    # the init time is the walk's: the warm-up's hand-overs are not reused, unless
    # ALIFMM_OPT_INIT_REUSE=1 asks for the steady state of repeated calls
    if "ALIFMM_OPT_INIT_REUSE" not in os.environ and opt(ctx, "init_reuse") is not None:
        ctx.set_option("init_reuse", 0)
    vt = W.default_table()
    ctx.set_model(*W.weldlike_model(), vt, vt, W.weldlike_dnx())
    sx, sz = W.c4_sources(128)
    out = {"variant": name}
    for ns in sizes:
        ctx.travel(sx[:ns], sz[:ns], copy_out=False)
        best = None
        for _ in range(2):
            ctx.travel(sx[:ns], sz[:ns], copy_out=False)
            ti, tb, tt = ctx.last_timing()
            best = tb if best is None else min(best, tb)
        sp = np.array([ctx.band_span(i) for i in range(ns)], dtype=np.float64) / 100.0  # us
        span = {"start_spread_us": round(float(sp[:, 0].max() - sp[:, 0].min()), 1),
                "end_spread_us": round(float(sp[:, 1].max() - sp[:, 1].min()), 1),
                "member0_ms_min": round(float((sp[:, 1] - sp[:, 0]).min()) / 1e3, 1),
                "member0_ms_max": round(float((sp[:, 1] - sp[:, 0]).max()) / 1e3, 1)}
        h = hashlib.sha256()
        for i in (0, ns // 2, ns - 1):
            h.update(ctx.get_field(i, 1).tobytes())
        ctx.set_option("prof", 1)
        ctx.travel(sx[:ns], sz[:ns], copy_out=False)
        ctx.set_option("prof", 0)
        p = ctx.band_profile(0)
        st = int(ctx.source_stats(0)[0][3])
        prof = {k: round(p[i] / 100.0 / st, 2) for i, k in enumerate(PH)}
        prof.update({k: round(p[10 + i] / 100.0 / st, 2) for i, k in enumerate(SUB)})
        # list sizes of member 0: mean live close set, accepted and claimed cells per step, max close-set high-water
        prof.update({"live_mean": round(p[6] / st, 1), "acc_mean": round(p[7] / st, 1), "claimed_mean": round(p[8] / st, 1),
                     "close_hi_max": int(p[9]), "steps": st})
        out[str(ns)] = {"k": int(ctx.get_option("last_k")), "band_ms": round(best, 1), "init_ms": round(ti, 1),
                        "init_reused": opt(ctx, "init_reused"), "fill_wait_ms": opt(ctx, "fill_wait_ms"),
                        "fields": h.hexdigest()[:16], "span": span, "us_per_step": prof}
    print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
