"""``run_timed(K, relayout_each_step=False)`` at the headline shape and at BASELINE configs[1] (the one-launch path: the
shape where host work between launches would show) on the build in the current directory; argv: a label and a run
number for the output line.  Run alternately on two builds (profiles/step_launcher_timing.txt)."""
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import bench  # noqa: E402
from celerite_amd import batch  # noqa: E402

label, rnd = sys.argv[1], sys.argv[2]
assert os.path.dirname(os.path.dirname(os.path.abspath(batch.__file__))) == os.getcwd(), batch.__file__
for name, B, N, JR, JC, seed, K in (("headline_b1024_n1e5_w8", 1024, 100000, 2, 3, 42, 100),
                                    ("config1_b256_n1e4_w4", 256, 10000, 0, 2, 7, 4000)):
    coeffs, t, diag, y = bench.make_inputs(B, N, JR, JC, seed=seed)
    plan = batch.BatchedGP(B, N, JR, JC)
    plan.set_series(t, diag, y)
    plan.set_coefficients(*coeffs)
    plan.log_likelihood()
    plan.run_timed(max(K // 10, 5), relayout_each_step=False)
    plan.results()
    tot, per = plan.run_timed(K, relayout_each_step=False)
    plan.results()
    print("run_timed %s %s %s K=%d total_ms=%.4f per_step_ms=%.5f small=%s kernel=%s" % (
        label, rnd, name, K, tot, tot / K, plan.small_mode_active(), plan.summarize_kernel()), flush=True)
    plan.close()
