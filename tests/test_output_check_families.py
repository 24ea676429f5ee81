# -*- coding: utf-8 -*-
"""CPU only: the adversarial families of the output check (tests/_cases.py; exercised on the device by
tests/test_gpu_output_check.py).  Each family has the property that makes it adversarial by construction, is positive
definite in the oracle, and the double oracle stays within a stated distance of the binary128 recurrence -- the yardstick
the device's factor is measured with."""
import numpy as np
import pytest

from oracle import ref
from _cases import (OUTPUT_CHECK_SETTLED, OUTPUT_CHECK_WIDTHS, coeffs_of, output_check_bucket, output_check_case,
                    output_check_cases, output_check_truth, within)

E_, E2_ = np.empty(0), np.empty((0, 0))
CASES = sorted(output_check_cases())

# double oracle against binary128, per family: (W per row of the row's largest, D relative, log det relative, solve of
# the largest, dot_solve relative).  F1 at eps = 1e-9 puts the second half of the series at t ~ 6e8, where a double
# carries the sample spacing to a few per cent only: the recurrence in double is that far from the one in binary128.
BOUNDS = {
    "F1 eps=1e-09": (3e-4, 1e-8, 2e-12, 1e-7, 1e-9),
    "F1 eps=1e-06": (3e-7, 3e-11, 1e-13, 3e-11, 1e-12),
    "F1 eps=0.001": (5e-10, 5e-12, 1e-13, 5e-12, 1e-13),
    "F2": (1e-8, 1e-10, 1e-13, 1e-10, 1e-12),
}
DEFAULT_BOUNDS = (5e-11, 2e-11, 2e-13, 1e-11, 5e-13)    # F0, F3, F4, F5


def _family(name):
    return name.rsplit(" w", 1)[0]


@pytest.mark.parametrize("name", CASES)
def test_family_has_its_adversarial_property(name):
    c = output_check_case(name)
    fam, t, N = _family(name), c["t"], len(c["t"])
    assert N >= 8192 and np.all(np.diff(t) >= 0)     # (F1 at eps = 1e-9: samples closer than a double's spacing at 6e8 coincide)
    a, cc, d = c["a_comp"], c["c_comp"], c["d_comp"]
    if fam.startswith("F1"):
        eps = float(fam.split("=")[1])
        k = np.arange(len(d))
        assert np.allclose(d / d[0] - 1.0, eps * k, rtol=1e-6, atol=1e-15)
        gap = t[N // 2] - t[N // 2 - 1]
        assert abs(gap * eps * d[0] - 1.0) < 1e-3
        assert np.all(np.exp(-cc * gap) >= 1e-2)                           # the gap does not erase the state
        assert np.allclose((d - d[0]) * gap, k, rtol=1e-6, atol=1e-6)      # phase differences jump by k radians
        span = t[N // 2 - 1] - t[0]
        assert np.max(np.abs(d - d[0])) * span < 1e-6 * max(1.0, eps * 1e7)  # ... and barely turn before it
    elif fam == "F2":
        d0 = d[0]
        assert np.allclose(d, d0 * np.arange(1, len(d) + 1))
        g = N // 2
        grid = np.abs(np.sin(np.outer(d, t[:g])))
        within("output-check families: F2 |sin(d_k t_n)| on the grid", np.max(grid), 1e-10, name)
        assert np.max(np.abs(np.sin(np.outer(d, t[g:])))) > 0.9           # probed on the irregular part
        assert np.max(cc) * np.pi / d0 < 1e-3                               # no forgetting within a chunk
    elif fam.startswith("F3"):
        assert np.all(a == a[0]) and np.all(cc == cc[0]) and np.all(d == d[0])
        dt = np.diff(t)
        if "gap" in fam:
            assert np.argmax(dt) == N // 2 - 1 and dt[N // 2 - 1] > 1e4 * np.median(dt)
            dt = np.delete(dt, N // 2 - 1)
        assert np.max(np.abs(dt - dt[0])) <= 1e-12 * t[-1]                  # one cadence: one transfer map
    elif fam == "F4":
        assert abs(a[-1] / a[0] - 1e-8) < 1e-20 and np.all(a[:-1] == a[0]) and np.all(d[:-1] == d[0])
        assert d[-1] * t[-1] < 2e-8
        # the property itself, on the oracle's factor: the tiny term's sine row (the last row of W) stays below 1e-6 of
        # the largest |W| of every block of 48 samples -- the shortest chunk the wide solver makes -- so of every chunk
        r = ref.RefSolver()
        r.compute(0.0, *coeffs_of(c), E_, E2_, E2_, t, c["diag"])
        W = r.state()[6]
        worst = max(np.max(np.abs(W[-1, n0:n0 + 48])) / np.max(np.abs(W[:, n0:n0 + 48])) for n0 in range(0, N, 48))
        within("output-check families: F4 sine row of the tiny term against the chunk's largest |W|", worst, 1e-6, name)
        assert np.max(np.abs(W[-1])) > 0
    elif fam == "F5":
        assert np.all(c["b_comp"] != 0) and np.all(np.abs(c["b_comp"] * d) <= a * cc)
        assert np.sum(d != 1.6) >= 3
    else:
        assert fam == "F0"          # the benchmark's log parameters (examples/benchmark/run.py:80-84) as coefficients
        assert np.allclose(c["a_real"], np.e) and np.allclose(c["c_real"], np.exp(0.1)) and np.allclose(a, np.exp(0.1))
        assert np.allclose(cc, np.exp(2.0)) and np.allclose(d, np.exp(1.6)) and np.all(c["b_comp"] == 0)


def test_every_bucket_and_entry_point_has_a_settled_case():
    """tests/test_gpu_output_check.py asserts, for the case named here per padded bucket and entry point, that the output
    check settles it (level 1) and the sequential fallback does not (level 2)."""
    for JR, JC in OUTPUT_CHECK_WIDTHS:
        for entry in ("hint", "nohint", "plan"):
            bucket = output_check_bucket(JR + 2 * JC)
            name = OUTPUT_CHECK_SETTLED[(bucket, entry)]
            assert name in CASES
            c = output_check_case(name)
            assert output_check_bucket(len(c["a_real"]) + 2 * len(c["a_comp"])) == bucket
    assert len(OUTPUT_CHECK_SETTLED) == 3 * len(OUTPUT_CHECK_WIDTHS)


@pytest.mark.parametrize("name", CASES)
def test_family_is_positive_definite_and_the_double_oracle_is_near_binary128(name):
    c = output_check_case(name)
    r = ref.RefSolver()
    r.compute(0.0, *coeffs_of(c), E_, E2_, E2_, c["t"], c["diag"])       # (raises where the reference would)
    _, _, J, ld, _, _, W, D = r.state()
    assert np.all(D > 0)
    Wq, Dq, xq, ldq, qq = output_check_truth(name)
    assert np.all(Dq > 0)
    b_row, b_d, b_ld, b_x, b_q = BOUNDS.get(_family(name), DEFAULT_BOUNDS)
    rm = np.max(np.abs(Wq), axis=1)
    within("output-check families: double oracle vs binary128, W per row (of the row's largest)",
           np.max(np.max(np.abs(W - Wq), axis=1) / rm), b_row, name)
    within("output-check families: double oracle vs binary128, D (relative)", np.max(np.abs(D - Dq) / np.abs(Dq)), b_d, name)
    within("output-check families: double oracle vs binary128, log det (relative)", abs(ld - ldq) / abs(ldq), b_ld, name)
    x = r.solve(c["y"])[:, 0]
    within("output-check families: double oracle vs binary128, solve (of the largest)", np.max(np.abs(x - xq)) / np.max(np.abs(xq)), b_x, name)
    within("output-check families: double oracle vs binary128, dot_solve (relative)", abs(r.dot_solve(c["y"]) - qq) / abs(qq), b_q, name)
