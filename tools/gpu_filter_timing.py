"""One-step-ahead residuals and causal forecasts on batched plans (clr_batch_one_step_ahead, clr_batch_forecast): what
they cost beside the calls they are the forward half of.

  * ``one_step_ahead()`` beside ``solve()``: device time (``solve_device_ms()``: HIP events around the kernels of the
    call) and wall time, alternating on one plan;
  * ``forecast(xs, return_var=True)`` beside ``predict(xs, return_var=True, method="recurrence")`` at M = 1, 4, 1e4 shared
    points: the forecast's device time beside the sum of the device times of predict's two C calls (the solve inside
    clr_batch_predict -- its scans over the points are not inside those events -- and clr_batch_predict_var_recurrence), and
    the wall time of both Python calls;
at the headline shape (1024 x 1e5 x width 8, lean) and BASELINE configs[1] (256 x 1e4 x width 4, lean).

Every shape is one step: a child process of its own under ``timeout``; a step that fails ends the run.  ``--resources
FILE`` appends FILE (the compiler's register and scratch counts of the width-8 kernels, see tools/README.md) to the record.
Writes profiles/filter_timing.txt.  Usage:
    python tools/gpu_filter_timing.py [--reps K] [--out PATH] [--resources FILE] [--step-timeout SECONDS]
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"headline": (1024, 100000, 2, 3, 42), "configs1": (256, 10000, 0, 2, 7)}


def say(text):
    print(text, flush=True)


def spread(v):
    import numpy as np
    return "median %9.3f  min %9.3f  max %9.3f" % (np.median(v), np.min(v), np.max(v))


def step(name, reps):
    """One shape, in this process."""
    import numpy as np

    from bench import make_inputs
    from celerite_amd import batch

    B, N, JR, JC, seed = SHAPES[name]
    coeffs, t, diag, y = make_inputs(B, N, JR, JC, seed)
    plan = batch.BatchedGP(B, N, JR, JC)
    try:
        plan.set_factor_layout("lean")
        plan.set_series(t, diag, y)
        plan.set_coefficients(*coeffs)
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        say("%s: B = %d, N = %d, width %d, lean factor, chunks %s" % (name, B, N, JR + 2 * JC, plan.chunks))

        def timed(call):
            t0 = time.perf_counter()
            out = call()
            return out, (time.perf_counter() - t0) * 1e3, plan.solve_device_ms()

        x = plan.solve()
        osa = plan.one_step_ahead()                       # (warm-up of both: buffers, the chunk maps)
        quad = np.sum(osa.innovation ** 2 / osa.variance, axis=1)
        say("  sum z^2 / D against y . solve(y) (relative, max over the batch): %.2e"
            % np.max(np.abs(quad - np.sum(y * x, axis=1)) / np.abs(quad)))
        del x, osa
        dev = {"one_step_ahead": [], "solve": []}
        wall = {"one_step_ahead": [], "solve": []}
        for _ in range(reps):
            for key, call in (("one_step_ahead", plan.one_step_ahead), ("solve", plan.solve)):
                _, w, d = timed(call)
                wall[key].append(w)
                dev[key].append(d)
        for key in ("one_step_ahead", "solve"):
            say("  %-16s device ms: %s   wall ms median %9.2f   (%d calls)" % (key + "()", spread(dev[key]), np.median(wall[key]), reps))
        say("  one_step_ahead / solve (device, medians) = %.2f" % (np.median(dev["one_step_ahead"]) / np.median(dev["solve"])))

        lo, hi = float(t.min()), float(t.max())
        for M in (1, 4, 10000):
            xs = np.linspace(lo - 0.01 * (hi - lo), hi + 0.01 * (hi - lo), M) if M > 1 else np.array([0.5 * (lo + hi)])
            plan.forecast(xs, return_var=True)
            plan.predict(xs, return_var=True, method="recurrence")
            fd, fw, pd, pw = [], [], [], []
            for _ in range(reps):
                _, w, d = timed(lambda: plan.forecast(xs, return_var=True))
                fw.append(w)
                fd.append(d)
                plan.predict(xs)
                d1 = plan.solve_device_ms()               # (the solve inside clr_batch_predict)
                _, w, d2 = timed(lambda: plan.predict(xs, return_var=True, method="recurrence"))
                pw.append(w)
                pd.append(d1 + d2)
            say("  M = %d shared points:" % M)
            say("    forecast(xs, return_var=True)                         device ms: %s   wall ms median %9.2f" % (spread(fd), np.median(fw)))
            say("    predict(xs, return_var=True, method='recurrence')     device ms: %s   wall ms median %9.2f   (device: its solve + the variance)" % (spread(pd), np.median(pw)))
            say("    forecast / predict (device, medians) = %.2f" % (np.median(fd) / np.median(pd)))
    finally:
        plan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_timing.txt"))
    ap.add_argument("--resources", default=None)
    ap.add_argument("--step-timeout", type=int, default=400)
    ap.add_argument("--step", choices=sorted(SHAPES), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        step(args.step, args.reps)
        return 0
    lines = ["# one-step-ahead residuals and causal forecasts on batched plans: tools/gpu_filter_timing.py --reps %d" % args.reps,
             "# Device: HIP events around the kernels of one call (solve_device_ms), the calls alternating in one process on one",
             "# plan, after a warm-up call of each.  Wall: host time of the call, uploads and downloads included."]
    for name in ("configs1", "headline"):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        print(done.stdout, end="", flush=True)
        lines.extend(done.stdout.splitlines())
        if done.returncode != 0:
            print("step %s failed with status %d: stopping" % (name, done.returncode), flush=True)
            return done.returncode
    if args.resources:
        lines.append("")
        lines.extend(open(args.resources).read().splitlines())
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
