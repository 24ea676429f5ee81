"""Component separation on batched plans (clr_batch_predict_terms): what it costs beside ``predict`` and the recurrence
variance, on one plan with the routes alternating, at M = 1, 100, 1e4 shared points:

  * ``predict_terms(xs)``                     G = T single-term groups, mean only;
  * ``predict_terms(xs, return_var=True)``    G = T, mean and variance;
  * ``predict(xs)``                           the full kernel's mean: one launch set per problem;
  * ``predict(xs, return_var=True, method="recurrence")``.

Wall time is the host time of the Python call, uploads and downloads included (``predict_terms`` brings G times the
numbers of ``predict`` down).  Device time (``solve_device_ms()``: HIP events) is the whole of ``clr_batch_predict_terms``
-- its solve and its passes --, but of ``predict`` only the solve inside it (its scans over the points are outside those
events) plus, with the variance, ``clr_batch_predict_var_recurrence``: compare the routes by wall time, and read the
device times as what the new passes cost on the device.

BASELINE configs[1] (256 x 1e4 x width 4, lean) and the headline shape (1024 x 1e5 x width 8, lean).  Every shape is one
step: a child process of its own under ``timeout``; a step that fails ends the run.  ``--resources FILE`` appends FILE
(the compiler's register and scratch counts of the width-8 kernels, see tools/README.md) to the record.
Writes profiles/predict_terms_timing.txt.  Usage:
    python tools/gpu_predict_terms_timing.py [--reps K] [--out PATH] [--resources FILE] [--step-timeout SECONDS]
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
        say("%s: B = %d, N = %d, width %d, G = T = %d groups, lean factor, chunks %s" % (name, B, N, JR + 2 * JC, JR + JC, plan.chunks))
        lo, hi = float(t.min()), float(t.max())
        routes = [("predict_terms(xs)", lambda xs: plan.predict_terms(xs)),
                  ("predict_terms(xs, return_var=True)", lambda xs: plan.predict_terms(xs, return_var=True)),
                  ("predict(xs)", lambda xs: plan.predict(xs)),
                  ("predict(xs, return_var=True, method='recurrence')", lambda xs: plan.predict(xs, return_var=True, method="recurrence"))]
        for M in (1, 100, 10000):
            xs = np.linspace(lo - 0.01 * (hi - lo), hi + 0.01 * (hi - lo), M) if M > 1 else np.array([0.5 * (lo + hi)])
            got = [call(xs) for _, call in routes]            # (warm-up of each: buffers, the factor-only state)
            dev_all = np.max(np.abs(got[0].sum(axis=1) - got[2])) / np.max(np.abs(got[2]))
            wall = [[] for _ in routes]
            dev = [[] for _ in routes]
            del got
            for _ in range(reps):
                for k, (_, call) in enumerate(routes):
                    if k == 3:                                # (device: predict's solve + the variance's call)
                        plan.predict(xs)
                        d1 = plan.solve_device_ms()
                    t0 = time.perf_counter()
                    call(xs)
                    wall[k].append((time.perf_counter() - t0) * 1e3)
                    dev[k].append(plan.solve_device_ms() + (d1 if k == 3 else 0.0))
            say("  M = %d shared points (sum of the terms' means against predict, of the largest entry: %.1e):" % (M, dev_all))
            for k, (label, _) in enumerate(routes):
                say("    %-52s wall ms: %s   device ms median %9.3f" % (label, spread(wall[k]), np.median(dev[k])))
            say("    predict_terms(xs) / predict(xs) (wall, medians) = %.2f" % (np.median(wall[0]) / np.median(wall[2])))
            say("    predict_terms with var / predict with var (wall, medians) = %.2f;  device: %.3f ms against %.3f ms"
                % (np.median(wall[1]) / np.median(wall[3]), np.median(dev[1]), np.median(dev[3])))
    finally:
        plan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_terms_timing.txt"))
    ap.add_argument("--resources", default=None)
    ap.add_argument("--step-timeout", type=int, default=400)
    ap.add_argument("--step", choices=sorted(SHAPES), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        step(args.step, args.reps)
        return 0
    lines = ["# component separation on batched plans: tools/gpu_predict_terms_timing.py --reps %d" % args.reps,
             "# Wall: host time of the Python call, uploads and downloads included; the routes alternate in one process on one",
             "# plan, after a warm-up call of each.  Device: HIP events (solve_device_ms) -- the whole of clr_batch_predict_terms,",
             "# but of predict only its solve (+ clr_batch_predict_var_recurrence): its scans over the points are outside them."]
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
