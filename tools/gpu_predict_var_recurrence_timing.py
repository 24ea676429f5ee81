"""The two routes to the predictive variance on batched plans side by side: ``predict(xs, return_var=True)`` with
``method="solve"`` (clr_batch_predict_var, O(M N J) per problem) and ``method="recurrence"``
(clr_batch_predict_var_recurrence, O((N + M) J^2)), through the C entries (only xs goes up, only var comes down), in one
process on one plan, alternating, device time from ``solve_device_ms()`` (HIP events around the kernels of the call).

  * BASELINE configs[1] (256 x 1e4 x width 4, lean): the plan's own data times as per-problem points (M = N = 1e4), and
    shared uniform grids of M = 1 .. 1e5 points -- the smallest measured M at which the recurrence wins is the crossover;
  * the headline shape (1024 x 1e5 x width 8, lean): shared grids, the solve route up to M = 64 only (it needs about
    3.5 ms per point there), the recurrence route up to M = 1e4;
  * per-problem UNSORTED points once (configs[1], M = 1e4): wall time against the same points sorted -- the host's
    sort and scatter.
Writes profiles/predict_var_recurrence_timing.txt.  Usage:
    python tools/gpu_predict_var_recurrence_timing.py [--reps K] [--skip-headline]
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from bench import make_inputs
from celerite_amd import batch

LINES = []
ENTRY = {"solve": "clr_batch_predict_var", "recurrence": "clr_batch_predict_var_recurrence"}


def say(text):
    print(text, flush=True)
    LINES.append(text)


def variance(plan, xs, method):
    """(var, wall ms, device ms) of one call of the route's C entry."""
    fn = getattr(batch._load(), ENTRY[method])
    fn.argtypes = [C.c_void_p, C.c_int, batch._dp, C.c_long, batch._dp]
    var = np.empty((plan.B, xs.shape[-1]))
    t0 = time.perf_counter()
    batch._check(fn(plan._h, xs.shape[-1], batch._ptr(xs), 0 if xs.ndim == 1 else xs.shape[1], batch._ptr(var)))
    wall = (time.perf_counter() - t0) * 1e3
    return var, wall, plan.solve_device_ms()


def make_plan(B, N, JR, JC, seed):
    coeffs, t, diag, y = make_inputs(B, N, JR, JC, seed)
    plan = batch.BatchedGP(B, N, JR, JC)
    plan.set_factor_layout("lean")
    plan.set_series(t, diag, y)
    plan.set_coefficients(*coeffs)
    assert (plan.log_likelihood(materialize=True)[3] == 0).all()
    return plan, coeffs, t


def spread(v):
    return "median %9.3f  min %9.3f  max %9.3f" % (np.median(v), np.min(v), np.max(v))


def side_by_side(plan, k0, label, xs, reps, solve_reps=None):
    """Both routes at the points ``xs``, alternating; returns the two median device times (solve: None if not run)."""
    solve_reps = reps if solve_reps is None else solve_reps
    M = xs.shape[-1]
    got = {}
    for method in ("recurrence", "solve"):          # (warm-up of both: buffers, the factor-only state of each)
        if method == "solve" and solve_reps == 0:
            continue
        got[method] = variance(plan, xs, method)[0]
    dev = {"recurrence": [], "solve": []}
    wall = {"recurrence": [], "solve": []}
    for r in range(reps):
        for method in ("recurrence", "solve"):
            if method == "solve" and r >= solve_reps:
                continue
            _, w, d = variance(plan, xs, method)
            wall[method].append(w)
            dev[method].append(d)
    say("  %s, M = %d:" % (label, M))
    say("    recurrence  device ms: %s   wall ms median %9.2f   (%d calls)" % (spread(dev["recurrence"]), np.median(wall["recurrence"]), reps))
    if dev["solve"]:
        say("    solve       device ms: %s   wall ms median %9.2f   (%d calls)" % (spread(dev["solve"]), np.median(wall["solve"]), len(dev["solve"])))
        diff = np.max(np.abs(got["recurrence"] - got["solve"]) / k0[:, None])
        ratio = np.median(dev["solve"]) / np.median(dev["recurrence"])
        say("    solve / recurrence (device, medians) = %.2f x; max |dvar| / k(0) between the routes = %.2e" % (ratio, diff))
        return float(np.median(dev["recurrence"])), float(np.median(dev["solve"]))
    say("    solve       not measured at this M")
    return float(np.median(dev["recurrence"])), None


def crossover(label, rows):
    """rows: (M, recurrence ms, solve ms or None) by ascending M."""
    wins = [M for M, rec, sol in rows if sol is not None and rec < sol]
    loses = [M for M, rec, sol in rows if sol is not None and not rec < sol]
    if not wins:
        say("  %s: the recurrence route does NOT win at any measured M (%s)" % (label, [r[0] for r in rows if r[2] is not None]))
    else:
        say("  %s: crossover -- the smallest measured M at which the recurrence route wins is %d (measured M: %s; it loses at: %s)"
            % (label, min(wins), [r[0] for r in rows if r[2] is not None], loses or "none"))


def grid(t, M):
    lo, hi = float(t.min()), float(t.max())
    return np.linspace(lo - 0.01 * (hi - lo), hi + 0.01 * (hi - lo), M)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-headline", action="store_true")
    args = ap.parse_args()
    say("# predictive variance on batched plans, the two routes: tools/gpu_predict_var_recurrence_timing.py --reps %d" % args.reps)
    say("# Device: HIP events around the kernels of one call (solve_device_ms), the routes alternating in one process on one")
    say("# plan, after a warm-up call of each.  Wall: host time of the call, upload, download and any host sort included.")
    say("device: %s" % (batch.device_info(),))

    B, N, JR, JC = 256, 10000, 0, 2
    plan, coeffs, t = make_plan(B, N, JR, JC, 7)
    k0 = np.sum(coeffs[0], axis=1) + np.sum(coeffs[2], axis=1)
    try:
        say("configs[1]: B = %d, N = %d, width %d, lean factor, chunks %s" % (B, N, JR + 2 * JC, plan.chunks))
        rec, sol = side_by_side(plan, k0, "the data times as points (per problem, sorted)", t, args.reps, min(args.reps, 3))
        say("  M = N = 1e4: the recurrence route is %s than the solve route measured in the same run (%.3f ms against %.3f ms)"
            % ("FASTER" if rec < sol else "NOT faster", rec, sol))
        rows = []
        for M in (1, 2, 4, 8, 16, 32, 100, 1000, 10000, 100000):
            solve_reps = min(args.reps, 3) if M <= 10000 else 1
            rows.append((M,) + side_by_side(plan, k0, "shared uniform grid", grid(t, M), args.reps, solve_reps))
        crossover("configs[1]", rows)
        rng = np.random.RandomState(3)
        own = rng.uniform(t.min(), t.max(), (B, 10000))
        own_sorted = np.sort(own, axis=1)
        w_un, w_so, d_un, d_so = [], [], [], []
        variance(plan, own, "recurrence")
        for _ in range(args.reps):
            v1, w, d = variance(plan, own, "recurrence"); w_un.append(w); d_un.append(d)
            v2, w, d = variance(plan, own_sorted, "recurrence"); w_so.append(w); d_so.append(d)
        order = np.argsort(own, axis=1, kind="stable")
        assert np.array_equal(np.take_along_axis(v1, order, axis=1), v2)
        say("  per-problem UNSORTED points, M = 1e4: wall ms %s; device ms median %.3f" % (spread(w_un), np.median(d_un)))
        say("  the same points sorted:               wall ms %s; device ms median %.3f" % (spread(w_so), np.median(d_so)))
        say("  host sort and scatter (wall, medians): %.2f ms for %d x %d points; the results are the sorted call's, permuted, bit for bit"
            % (np.median(w_un) - np.median(w_so), B, 10000))
    finally:
        plan.close()

    if not args.skip_headline:
        B, N, JR, JC = 1024, 100000, 2, 3
        plan, coeffs, t = make_plan(B, N, JR, JC, 42)
        k0 = np.sum(coeffs[0], axis=1) + np.sum(coeffs[2], axis=1)
        try:
            say("headline: B = %d, N = %d, width %d, lean factor, chunks %s" % (B, N, JR + 2 * JC, plan.chunks))
            rows = []
            for M in (1, 4, 16, 64):
                rows.append((M,) + side_by_side(plan, k0, "shared uniform grid", grid(t, M), args.reps, min(args.reps, 2)))
            rows.append((10000,) + side_by_side(plan, k0, "shared uniform grid", grid(t, 10000), args.reps, 0))
            crossover("headline", rows)
        finally:
            plan.close()
    out = os.path.join(ROOT, "profiles", "predict_var_recurrence_timing.txt")
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
