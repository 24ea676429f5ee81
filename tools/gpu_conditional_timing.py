"""The joint posterior at prediction points on batched plans (clr_batch_predict_cov, clr_batch_sample_conditional): what it
costs at M = 10, 100, 1000 shared points (and 1e4 for the draws alone), beside the route a plan offered before:

  * ``predict_cov(xs)``                          (B, M, M);
  * ``sample_conditional(xs, size=1)``, ``(xs, size=16)``   predict's mean plus the device draws;
  * the earlier route, per problem: ``k*`` in NumPy, ``plan.solve(b=k*^T)`` a tile of right-hand sides at a time, the dense
    covariance ``k(x, x') - k*^T K^-1 k*'``, ``np.linalg.cholesky`` of it (+ 1e-8 k(0) I) and ``L n`` for 16 draws.

Device time is ``solve_device_ms()`` of the C entry (HIP events around the kernels of every tile of problems, never the
copies).  "entry wall" is the host time of the C entry alone -- uploads, downloads, sorting and scattering included --,
"call wall" that of the Python method, which for ``sample_conditional`` also runs ``predict`` for the mean (one launch set
per problem: it dominates at these sizes).  The earlier route is timed on a SUBSET of the problems in a plan of their own
(its ``k*`` alone is B x N x M kernel evaluations in NumPy) and scaled by B / subset: the host part scales exactly, the
solve's share is overestimated where the subset leaves the device idle; the subset is printed with every figure.

BASELINE configs[1] (256 x 1e4 x width 4, lean) and the headline shape (1024 x 1e5 x width 8, lean).  Every shape is one
step: a child process of its own under ``timeout``; a step that fails ends the run.  ``--resources FILE`` appends FILE
(the compiler's register and scratch counts of the kernels, see tools/README.md) to the record.
Writes profiles/sample_conditional_timing.txt.  Usage:
    python tools/gpu_conditional_timing.py [--reps K] [--out PATH] [--resources FILE] [--step-timeout SECONDS]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"headline": (1024, 100000, 2, 3, 42), "configs1": (256, 10000, 0, 2, 7)}
SUBSET_CELLS = 1.6e8      # the earlier route's subset: problems x N x M kernel evaluations at most, 16 problems at most


def say(text):
    print(text, flush=True)


def kernel_value(coeffs, p, tau):
    import numpy as np
    ar, cr, ac, bc, cc, dc = [c[p] for c in coeffs]
    tau = np.abs(tau)
    out = np.zeros(tau.shape)
    for a, c in zip(ar, cr):
        out += a * np.exp(-c * tau)
    for a, b, c, d in zip(ac, bc, cc, dc):
        out += np.exp(-c * tau) * (a * np.cos(d * tau) + b * np.sin(d * tau))
    return out


def earlier_route(batch, coeffs, t, diag, y, JR, JC, xs, subset, rng):
    """Seconds for `subset` problems: k*, the solves, the dense covariance, its Cholesky factor and 16 draws."""
    import numpy as np
    N, M = t.shape[1], len(xs)
    sub = tuple(c[:subset] for c in coeffs)
    plan = batch.BatchedGP(subset, N, JR, JC)
    try:
        plan.set_factor_layout("lean")
        plan.set_series(t[:subset], diag[:subset], y[:subset])
        plan.set_coefficients(*sub)
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        plan.solve()                                   # (warm-up: buffers, the chunk maps)
        R = max(1, min(M, int(2.0e8 / (subset * N))))  # right-hand sides per tile
        t0 = time.perf_counter()
        kstar = np.stack([kernel_value(coeffs, p, xs[:, None] - t[p][None, :]) for p in range(subset)])      # (subset, M, N)
        sol = np.empty_like(kstar)
        for m0 in range(0, M, R):
            sol[:, m0:m0 + R] = plan.solve(np.ascontiguousarray(kstar[:, m0:m0 + R]))
        worst = 0.0
        for p in range(subset):
            cov = kernel_value(coeffs, p, xs[:, None] - xs[None, :]) - kstar[p] @ sol[p].T
            k0 = float(np.sum(coeffs[0][p]) + np.sum(coeffs[2][p]))
            Lc = np.linalg.cholesky(0.5 * (cov + cov.T) + 1e-8 * k0 * np.eye(M))
            draws = rng.standard_normal((16, M)) @ Lc.T
            worst = max(worst, float(np.max(np.abs(draws))))
        return time.perf_counter() - t0, R
    finally:
        plan.close()


def step(name, reps):
    """One shape, in this process."""
    import numpy as np

    from bench import make_inputs
    from celerite_amd import batch

    B, N, JR, JC, seed = SHAPES[name]
    coeffs, t, diag, y = make_inputs(B, N, JR, JC, seed)
    lib = batch._load()
    ip = C.POINTER(C.c_int)
    rng = np.random.RandomState(1)
    plan = batch.BatchedGP(B, N, JR, JC)
    try:
        plan.set_factor_layout("lean")
        plan.set_series(t, diag, y)
        plan.set_coefficients(*coeffs)
        assert (plan.log_likelihood(materialize=True)[3] == 0).all()
        say("%s: B = %d, N = %d, width %d, lean factor, chunks %s" % (name, B, N, JR + 2 * JC, plan.chunks))
        lo, hi = float(t.min()), float(t.max())
        k0 = float(np.sum(coeffs[0][0]) + np.sum(coeffs[2][0]))
        draw_dev, ratio = {}, {}
        for M in (10, 100, 1000, 10000):
            xs = np.linspace(lo - 0.01 * (hi - lo), hi + 0.01 * (hi - lo), M)
            say("  M = %d shared points:" % M)
            rows = []
            if M <= 1000:
                if 8.0 * B * M * M > 4.0e9:
                    say("    predict_cov: not measured (a host array of %.1f GB)" % (8e-9 * B * M * M))
                else:
                    cov = np.empty((B, M, M))

                    def entry_cov():
                        batch._check(lib.clr_batch_predict_cov(plan._h, M, batch._ptr(xs), 0, batch._ptr(cov)))
                    rows.append(("predict_cov(xs)", entry_cov, lambda: plan.predict_cov(xs)))
            for size in (1, 16):
                n = rng.standard_normal((B, size, M))
                dr, st = np.empty((B, size, M)), np.empty(B, dtype=np.int32)

                def entry_draw(size=size, n=n, dr=dr, st=st):
                    batch._check(lib.clr_batch_sample_conditional(plan._h, M, batch._ptr(xs), 0, size, batch._ptr(n), 1e-8 * k0, 1e-10,
                                                                  batch._ptr(dr), st.ctypes.data_as(ip)))
                    assert (st == 0).all()
                rows.append(("sample_conditional(xs, size=%d)" % size, entry_draw,
                             lambda size=size, n=n: plan.sample_conditional(xs, size=size, normals=n, regularize=1e-8 * k0)))
            for label, entry, call in rows:
                entry()                                   # (warm-up: buffers, the factor-only state)
                dev, ewall, cwall = [], [], []
                for _ in range(reps if M < 10000 else max(1, reps // 2)):
                    t0 = time.perf_counter()
                    entry()
                    ewall.append((time.perf_counter() - t0) * 1e3)
                    dev.append(plan.solve_device_ms())
                    t0 = time.perf_counter()
                    call()
                    cwall.append((time.perf_counter() - t0) * 1e3)
                say("    %-34s device ms median %10.3f   entry wall ms median %10.1f   call wall ms median %10.1f"
                    % (label, np.median(dev), np.median(ewall), np.median(cwall)))
                if label.endswith("size=16)"):
                    draw_dev[M] = (np.median(dev), np.median(ewall), np.median(cwall))
            cov = None
            if M <= 1000:
                subset = int(max(1, min(16, B, SUBSET_CELLS // (N * M))))
                sec, R = earlier_route(batch, coeffs, t, diag, y, JR, JC, xs, subset, rng)
                scaled = sec * 1e3 * B / subset
                d16 = draw_dev[M]
                say("    earlier route (k*, solve in tiles of %d, dense cov, cholesky, 16 draws): %.1f ms for %d problems -> %.0f ms scaled to %d"
                    % (R, sec * 1e3, subset, scaled, B))
                say("    earlier route / sample_conditional(size=16): %.1f x by the call's wall time, %.1f x by the entry's"
                    % (scaled / d16[2], scaled / d16[1]))
                ratio[M] = scaled / d16[2]
            else:
                say("    earlier route: not measured (a dense %d x %d factorisation and N x M kernel evaluations per problem)" % (M, M))
        wins = [M for M in sorted(ratio) if all(ratio[m] > 1.0 for m in ratio if m >= M)]
        say("  the new route is the faster one from M = %s on (by the call's wall time; measured at M = %s)"
            % (wins[0] if wins else "none of the measured", ", ".join(str(m) for m in sorted(ratio))))
        if 1000 in draw_dev and 10000 in draw_dev:
            a, b = draw_dev[1000], draw_dev[10000]
            say("  sample_conditional(size=16) from M = 1000 to 10000: device %.1f x, entry wall %.1f x, call wall %.1f x"
                % (b[0] / a[0], b[1] / a[1], b[2] / a[2]))
    finally:
        plan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_conditional_timing.txt"))
    ap.add_argument("--resources", default=None)
    ap.add_argument("--step-timeout", type=int, default=400)
    ap.add_argument("--step", choices=sorted(SHAPES), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        step(args.step, args.reps)
        return 0
    lines = ["# joint posterior at prediction points on batched plans: tools/gpu_conditional_timing.py --reps %d" % args.reps,
             "# device: HIP events around the kernels of every tile of problems (solve_device_ms); entry wall: the C entry alone,",
             "# copies, sorting and scattering included; call wall: the Python method (sample_conditional: + predict for the mean).",
             "# The earlier route runs on a subset of the problems in a plan of its own and is scaled by B / subset."]
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
