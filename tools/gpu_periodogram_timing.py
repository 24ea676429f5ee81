"""The periodogram under a plan's covariance (clr_batch_periodogram): what a scan of F frequencies costs, against the route
the library offered before it for the same numbers.

At the headline shape (B = 1024, N = 1e5, width 8 = 2 real + 3 complex) and at BASELINE configs[1]'s (B = 256, N = 1e4,
width 4 = 2 complex), after a materialising run, in ONE process per shape:
  * periodogram(omega) with F = 1, 64, 1024 shared frequencies: host wall time and the device time of its kernels
    (clr_batch_get_periodogram_ms);
  * the earlier route, per frequency: set_mean_basis((cos, sin)) -- a (2, N) basis shared by all problems goes up --,
    a materialising evaluation with zero weights and fit_mean_weights().  Timed on a SUBSET of frequencies (--old) and
    scaled linearly to F: said so in the output;
  * a plain evaluation (run_timed) on a plan that never calls the periodogram, before and after the scans of the other
    plan: the evaluation step is untouched.
Each shape runs in a child process of its own under `timeout`, and the first one that fails ends the run.  Usage:
    python tools/gpu_periodogram_timing.py [--old 3] [--commit ID] [--out profiles/periodogram_timing.txt]
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

SHAPES = {"headline": (1024, 100000, 2, 3, "headline 1024 x 1e5 x width 8"),
          "configs1": (256, 10000, 0, 2, "configs[1] 256 x 1e4 x width 4")}
FS = (1, 64, 1024)


def measure(name, n_old):
    from bench import make_inputs
    from celerite_amd import batch

    B, N, JR, JC, label = SHAPES[name]
    print("device: %s" % (batch.device_info(),), flush=True)
    coeffs, t, diag, y = make_inputs(B, N, JR, JC, 42)
    T = float(t.max() - t.min())
    dt = float(np.median(np.diff(t[0])))
    t_ref = float(t.min())

    def plain_step():
        p = batch.BatchedGP(B, N, JR, JC)
        p.set_series(t, diag, y)
        p.set_coefficients(*coeffs)
        p.run_timed(3)
        ms = p.run_timed(10)[0] / 10
        p.close()
        return ms

    before = plain_step()
    plan = batch.BatchedGP(B, N, JR, JC)
    plan.set_series(t, diag, y)
    plan.set_coefficients(*coeffs)
    assert (plan.log_likelihood(True)[3] == 0).all()
    plan.periodogram(np.array([4 * np.pi / T]), t_ref=t_ref)          # (buffers, events)
    new = {}
    for F in FS:
        omega = np.geomspace(4 * np.pi / T, np.pi / dt, F) if F > 1 else np.array([40 * np.pi / T])
        t0 = time.perf_counter()
        pg = plan.periodogram(omega, t_ref=t_ref)
        wall = (time.perf_counter() - t0) * 1e3
        assert (pg.status == 0).all()
        new[F] = (wall, plan.periodogram_ms())
        print("%s: periodogram, F = %d: %.2f ms of host wall time, %.2f ms on the device: %.3f us per (problem, frequency)"
              % (label, F, wall, new[F][1], 1e3 * new[F][1] / (B * F)), flush=True)
    # the earlier route on a few frequencies of the longest list
    sub = omega[np.linspace(0, len(omega) - 1, n_old).astype(int)]
    ll0 = plan.log_likelihood(True)[0]
    old_wall, old_dev, worst = [], [], 0.0
    for w in sub:
        t0 = time.perf_counter()
        arg = w * (t - t_ref)                                             # (every problem has its own times)
        plan.set_mean_basis(np.stack([np.cos(arg), np.sin(arg)], axis=1))
        plan.set_mean_weights(np.zeros((B, 2)))
        plan.log_likelihood(True)
        fit = plan.fit_mean_weights()
        old_wall.append((time.perf_counter() - t0) * 1e3)
        old_dev.append(sum(plan.mean_fit_ms()))
        f = int(np.argmin(np.abs(omega - w)))
        worst = max(worst, float(np.max(np.abs((fit.loglike - ll0) - pg.power[:, f]) / (1 + np.abs(pg.power[:, f])))))
    plan.close()
    ow, od = float(np.median(old_wall)), float(np.median(old_dev))
    print("%s: the earlier route (set_mean_basis((cos, sin)) + a materialising evaluation + fit_mean_weights()), per frequency, "
          "median of %d: %.1f ms of host wall time, of which %.1f ms in fit_mean_weights' kernels; its gain in profiled "
          "log-likelihood and `power` agree to %.1e (1 + |power|)" % (label, len(sub), ow, od, worst), flush=True)
    for F in FS:
        print("%s: F = %d: the earlier route SCALED from those %d frequencies %.0f ms (wall), %.0f ms (fit kernels alone); the new "
              "call %.1fx / %.1fx faster" % (label, F, len(sub), ow * F, od * F, ow * F / new[F][0], od * F / new[F][1]), flush=True)
    after = plain_step()
    print("%s: a plain evaluation on a plan that never scans: %.3f ms before, %.3f ms after the scans" % (label, before, after),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", type=int, default=3, help="frequencies the earlier route is timed on")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "periodogram_timing.txt"))
    ap.add_argument("--timeout", type=int, default=420, help="seconds per shape")
    ap.add_argument("--only", choices=sorted(SHAPES), help="(a child's measurement)")
    args = ap.parse_args()
    if args.only:
        return measure(args.only, args.old)
    commit = args.commit
    if not commit:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    lines = ["# tools/gpu_periodogram_timing.py (MI355X, one GPU): the sinusoid scan under a plan's covariance.",
             "# Host wall time of one call returning synchronised results; device time: HIP events around the call's kernels.",
             "# The earlier route is timed on %d frequencies and scaled linearly to F." % args.old,
             "commit: %s" % commit]
    for only in ("configs1", "headline"):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--only", only,
               "--old", str(args.old)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:       # nothing more is started on the device after a failure
            sys.exit("measurement '%s' ended with status %d" % (only, r.returncode))
        lines += [l for l in r.stdout.splitlines() if l.startswith((SHAPES[only][4], "device:")) and l not in lines]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
