"""Workload for `rocprofv3 --kernel-trace --stats`: every route of tests/test_gpu_step_launcher.py -- each through
``enqueue`` and through ``run_timed(2)`` -- on the build in the current directory.  Two builds launch the same kernels
when tools/rocpd_kernel_counts.py prints the same table for both (profiles/step_launcher_kernel_counts.txt).  With
``--plan-reuse``: the sequences of tests/test_gpu_plan_reuse.py behind them -- every change of an input or a setting
between two evaluations of one plan (profiles/plan_state_kernel_counts.txt) -- without its last case, which is wrong
on builds before the plan's copies of the series kept their own staleness."""
import os
import sys

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import test_gpu_step_launcher as T  # noqa: E402
from celerite_amd import batch  # noqa: E402

assert os.path.dirname(os.path.dirname(os.path.abspath(batch.__file__))) == os.getcwd(), batch.__file__
for n in (24, 1):
    T.test_narrow_scan_single_wave_summarize(n)
T.test_role_split_summarize(1, "role split")
T.test_role_split_summarize(2, "role split, lazy decay")
T.test_warm_path_and_its_fallback_scan("some fall back")
T.test_warm_path_and_its_fallback_scan("all fall back")
T.test_one_launch_path()
for a in ((2, 7, 3000, 5), (10, 11, 3000, 5), (8, 20, 6000, 5), (0, 24, 6000, 1)):
    T.test_wide_plans(*a)
for a in ((0, 4, 2, 1500, False), (0, 4, 2, 1500, True), (2, 1, 3, 700, False)):
    T.test_general_terms(*a)
T.test_widths_65_to_128()
T.test_materialising_narrow_plan("reference")
T.test_materialising_narrow_plan("lean")
T.test_materialising_wide_plan()
T.test_deferred_level1_problems_on_a_narrow_plan()
T.test_deferred_level1_problems_on_a_wide_plan()
T.test_mean_set_after_the_series(6, 1, dict(nchunk=64, kernel="role split, lazy decay"))
T.test_mean_set_after_the_series(2, 1, dict(nchunk=24))
for w in ("narrow scan", "one launch", "wide"):
    T.test_profile_of_enqueued_evaluations(w)
if "--plan-reuse" in sys.argv[1:]:
    import test_gpu_plan_reuse as R  # noqa: E402
    for route in list(R.ROUTES) + [r + ", materialising" for r in R.MATERIALISING]:
        for change in R.CHANGES:
            R.test_reused_plan_equals_fresh_plan(route, change)
    for first in ("dense", "not dense"):
        R.test_coefficient_draw_switches_the_summarize_kernel(first)
print("routes ok")
