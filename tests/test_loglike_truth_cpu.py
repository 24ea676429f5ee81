# -*- coding: utf-8 -*-
"""The reference side of tests/test_gpu_loglike_truth.py, without a device: for every case that module uses
(tests/_loglike_truth.py, ``CASES``) the double oracle and the binary128 recurrence alone must already satisfy what the
GPU tests rely on --

  * every adversarial batch has at least 8 judgeable problems (oracle status OK, truth finite and non-zero), every other
    case judges all of its problems (the warm-start batch with one indefinite problem: all the others);
  * the yardstick Y = max(worst e_ref, sqrt(N) 2^-53) is at most 1e-12 on the benign and structured families other than
    G5, so that no device bar there is looser than 3e-11 (G5 and the adversarial family carry their recorded e_ref, no
    cap);
  * the series of the lazy-regime and decay-factor cases sit where their names say.

Recorded here (worst Y per group; the end-of-session table prints them again):
  synthetic bench / accuracy, every shape and size   5.9e-14   (real terms only; 8.6e-15 .. 3.7e-14 with complex terms)
  synthetic bench, b_comp = 0                         3.4e-14
  G1 .. G4                                            7.1e-15 (the floor at N = 4099)
  G5 large phase                                      log det 1.6e-13, quadratic form 3.6e-12 (no cap)
  F0 .. F5 at (2,3) (0,4) (1,3) (2,1) (0,2)           7.6e-13   (F1 eps = 1e-6 at (0, 4), quadratic form; next: the same
                                                                family at (0, 2) 3.4e-13, F3 with a gap at (2, 1) 2.4e-13)
  lazy edges, decay-factor regimes                    1.1e-14, 1.0e-14
  warm start, route 1, ragged                         1.4e-14, 1.1e-14, 7.5e-14
  adversarial(32, 2000, seed 3), 24 shapes            8 .. 29 judgeable; worst e_ref 8.6e-12
No case exceeds the 1e-12 cap.
"""
import numpy as np
import pytest

import _loglike_truth as T
from _cases import ALL_WIDTH_SHAPES, within

Y_CAP = 1e-12


def _group(key):
    """(test case, line of the end-of-session table) a case is checked and reported under."""
    if key[0] == "syn":
        return "synthetic (%d, %d)" % key[2:4], "synthetic, %d complex terms" % key[3]
    if key[0] == "adv":
        return "adversarial (%d, %d)" % key[1:3], "adversarial"
    name = {"syn b=0": "synthetic, b_comp = 0", "G": "G families", "F": "F families", "lazy edge": "lazy edges",
            "lazy edge, every step": "lazy edges, every step", "exp": "decay-factor regimes", "warm": "warm start", "route 1": "route 1", "ragged": "ragged"}[key[0]]
    return (name + " (%d, %d)" % key[-2:] if key[0] in ("syn b=0", "F", "lazy edge, every step") else name), name


GROUPS = sorted({_group(k)[0] for k in T.CASES})


@pytest.mark.parametrize("group", GROUPS)
def test_reference_side_of_every_case(group):
    keys = [k for k in T.CASES if _group(k)[0] == group]
    assert keys
    for key in keys:
        name = _group(key)[1]
        r = T.reference(key)
        n = int(r.judgeable.sum())
        e = r.e_ref[:, r.judgeable]
        assert n >= T.must_judge(key, r), (key, n, r.s0)
        assert np.all(np.isfinite(e)), (key, e)
        Y = r.yardstick()[:, r.judgeable]
        print("%s: %d of %d judgeable; e_ref log det %.1e .. %.1e, quadratic form %.1e .. %.1e; Y %.1e / %.1e" %
              (key, n, len(r.s0), e[0].min(), e[0].max(), e[1].min(), e[1].max(), Y[0].max(), Y[1].max()))
        if r.kind == "benign":
            within("log-likelihood truth: yardstick Y of the double oracle, %s" % name, Y.max(), Y_CAP, key)
        else:  # G5 and the adversarial family carry their recorded e_ref: no cap
            within("log-likelihood truth: e_ref of the double oracle, %s (recorded, no cap)" % name, e.max(), 1.0, key)


def test_every_adversarial_shape_is_registered():
    assert sorted(k[1:] for k in T.CASES if k[0] == "adv") == sorted(ALL_WIDTH_SHAPES)
    assert T.reference(("adv", 0, 4)).judgeable.sum() >= T.ADV_MIN_JUDGED


def test_lazy_edge_cases_sit_at_their_fraction_of_the_limit():
    for key in [k for k in T.CASES if k[0] == "lazy edge"]:
        _, which, frac, JR, JC = key
        cmax, dmax, dxmax = T.host_bounds(T.case_of(key))
        c, d = cmax * dxmax / T.LAZY_C_LIMIT, dmax * dxmax / T.LAZY_D_LIMIT
        assert abs((c if which == "c" else d) - frac) < 1e-9, (key, c, d)
        assert (d if which == "c" else c) < 0.9, (key, c, d)          # the other product stays inside the regime


def test_every_step_lazy_edge_cases_sit_just_below_the_limit():
    for key in [k for k in T.CASES if k[0] == "lazy edge, every step"]:
        case = T.case_of(key)
        cmax, dmax, _ = T.host_bounds(case)
        dx = np.diff(case["t"], axis=1)
        x = cmax * dx / T.LAZY_C_LIMIT if key[1] == "c" else dmax * dx / T.LAZY_D_LIMIT
        other = dmax * dx / T.LAZY_D_LIMIT if key[1] == "c" else cmax * dx / T.LAZY_C_LIMIT
        assert 0.89 < x.min() and x.max() < 1.0 and other.max() < 0.9, (key, x.min(), x.max(), other.max())


def test_decay_factor_cases_sit_in_their_regime():
    for key in [k for k in T.CASES if k[0] == "exp"]:
        case = T.case_of(key)
        cmax = T.host_bounds(case)[0]
        x = cmax * np.diff(case["t"], axis=1)
        if key[1] == "tiny":
            assert 0.89 * T.EXP_TINY_LIMIT < x.min() and x.max() < T.EXP_TINY_LIMIT
        elif key[1] == "small":
            assert 0.89 * T.EXP_SMALL_LIMIT < x.min() and x.max() < T.EXP_SMALL_LIMIT
        else:
            above = x >= T.EXP_TINY_LIMIT
            assert (above.sum(axis=1) == 2).all() and (x >= T.EXP_SMALL_LIMIT).sum() == len(x)
            # both long steps lie inside a chunk of the 37-chunk plan (111 samples each), at different steps of it
            L = -(-T.STRUCT_N // 37)
            at = np.flatnonzero(above[0]) + 1
            assert all(a % L not in (0, L - 1) for a in at) and at[0] % L != at[1] % L


def test_ragged_lengths_cover_the_spread_and_both_ends():
    n = T.ragged_lengths()
    N = T.RAGGED_N
    assert n.max() == N and n.min() == N // 10 and np.sum((n >= N // 2) & (n < N)) == len(n) - 2
    assert np.array_equal(T.reference(("ragged", 2, 3)).n, n)


def test_large_t_truth_and_twin():
    """t ~ 3e8: the log-likelihood with phases fl(d t), in binary128 and in double; d t far above the fast-trig limit."""
    case = T.large_t_case()
    assert np.max(case["d_comp"]) * np.max(case["t"]) >= 1e9
    truth, twin = T.large_t_reference()
    assert np.all(np.isfinite(truth)) and np.all(truth != 0)
    within("log-likelihood truth: double twin at t ~ 3e8 (recorded)", np.max(np.abs(twin - truth) / np.abs(truth)), 1e-6)
