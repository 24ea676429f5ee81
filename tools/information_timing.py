"""The information matrix on batched plans (clr_batch_information): what it costs.

At the headline shape (1024 x 1e5 x width 8) and at BASELINE configs[1] (256 x 1e4 x width 4), in ONE process and on one
build: ``information()`` -- host wall time of the synchronous call (median) and its device time
(``clr_batch_get_information_ms``: HIP events from its evaluation to its last Gram pass) -- beside
``grad_log_likelihood()`` in reverse mode and in ``set_grad_mode("forward")``.  The forward-mode gradient is the
yardstick: it does the same base and tangent work once, the information matrix twice (the tangent start states, then the
rows) plus the rows' trip through HBM and the Gram pass.
One series, B = 1, N = 1e5: the chunk-parallel route beside the sequential form forced by ``set_exact``.
Writes profiles/information_timing.txt (the headline step against the parent commit is appended by hand from
``bench.py --gpus 1`` runs of both builds).  Usage:
    python tools/information_timing.py [--reps K] [--skip-headline]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from bench import make_inputs
from celerite_amd import batch

LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def timed(fn, reps):
    walls, extra = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        e = fn()
        walls.append((time.perf_counter() - t0) * 1e3)
        extra.append(e)
    return float(np.median(walls)), float(np.median(extra))


def shape(label, B, N, JR, JC, seed, reps):
    coeffs, t, diag, y = make_inputs(B, N, JR, JC, seed)
    plan = batch.BatchedGP(B, N, JR, JC)
    try:
        plan.set_series(t, diag, y)
        plan.set_coefficients(*coeffs, jitter=0.01)
        M = 1 + 2 * JR + 4 * JC
        say("%s: B = %d, N = %d, width %d (%d real + %d complex), %d directions, scan chunks %s"
            % (label, B, N, JR + 2 * JC, JR, JC, M, plan.chunks))
        info, st = plan.information()          # (warm-up: buffers)
        assert (st == 0).all()
        d = np.sqrt(np.einsum("bii->bi", info))
        say("  smallest eigenvalue at unit diagonal over the batch: %.2e" % min(np.linalg.eigvalsh(info[b] / np.outer(d[b], d[b])).min() for b in range(min(B, 64))))
        wall, dev = timed(lambda: (plan.information(), plan.information_device_ms())[1], reps)
        say("  information():                         wall %9.2f ms, device %9.2f ms" % (wall, dev))
        out = {"information": dev}
        for mode in ("reverse", "forward"):
            plan.set_grad_mode(mode)
            plan.grad_log_likelihood()
            w, _ = timed(lambda: (plan.grad_log_likelihood(), 0.0)[1], reps)
            say("  grad_log_likelihood(), %-7s mode:    wall %9.2f ms" % (mode, w))
            out[mode] = w
        plan.set_grad_mode("reverse")
        say("  information() wall / forward-mode gradient wall = %.2f; / reverse-mode gradient wall = %.2f"
            % (wall / out["forward"], wall / out["reverse"]))
    finally:
        plan.close()


def one_series(N, JR, JC, seed, reps):
    coeffs, t, diag, y = make_inputs(1, N, JR, JC, seed)
    plan = batch.BatchedGP(1, N, JR, JC)
    try:
        plan.set_series(t, diag, y)
        plan.set_coefficients(*coeffs, jitter=0.01)
        say("one series: B = 1, N = %d, width %d, scan chunks %s" % (N, JR + 2 * JC, plan.chunks))
        a, _ = plan.information()
        wall, dev = timed(lambda: (plan.information(), plan.information_device_ms())[1], reps)
        say("  information(), chunk-parallel route:   wall %9.2f ms, device %9.2f ms" % (wall, dev))
        plan.set_exact(True)
        b, _ = plan.information()
        wall_s, dev_s = timed(lambda: (plan.information(), plan.information_device_ms())[1], max(1, reps // 2))
        say("  information(), sequential form:        wall %9.2f ms, device %9.2f ms (%.1f x the chunk-parallel route)"
            % (wall_s, dev_s, dev_s / dev))
        d = np.sqrt(np.diag(a[0]))
        say("  the two routes differ by %.2e of sqrt(I_ii I_jj)" % np.max(np.abs(a[0] - b[0]) / np.outer(d, d)))
    finally:
        plan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-headline", action="store_true")
    args = ap.parse_args()
    say("# the information matrix on batched plans: tools/information_timing.py --reps %d" % args.reps)
    say("# Wall: host time of the synchronous call, downloads included (median).  Device: HIP events on the plan's stream.")
    say("device: %s" % (batch.device_info(),))
    shape("configs[1]", 256, 10000, 0, 2, 7, args.reps)
    one_series(100000, 2, 3, 42, args.reps)
    if not args.skip_headline:
        shape("headline", 1024, 100000, 2, 3, 42, args.reps)
    out = os.path.join(ROOT, "profiles", "information_timing.txt")
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
