# -*- coding: utf-8 -*-
"""`-m gpu`: what the lazy role-split summarize (widths 7 and 8, csrc/clr_split_kernels.h) leaves out when the plan allows
it -- the per-lane sample index behind the pivot flag, the ``b_comp`` terms of the features when every ``b_comp`` is
zero -- against the general kernel of the same build
(``CLR_SPLIT_GENERIC``) and against the CPU oracle.  Small series: 3 problems, ~720 samples, one wave of chunks."""
import functools

import numpy as np
import pytest

from celerite_amd import batch
from oracle import ref
from _cases import synthetic, coeffs_of

pytestmark = pytest.mark.gpu
REL = 1e-10
B = 3
SHAPES = [(2, 3), (1, 3)]   # width 8 and width 7


@functools.lru_cache(maxsize=None)
def dense_case(N, JR, JC):
    """The bench family squeezed until it is densely sampled for the lazy kernels (max c dx < 2^-7, max d dx < 2^-5)."""
    case = synthetic(B, N, JR, JC, "bench", seed=100 * N + 10 * JR + JC)
    case["t"] = case["t"] * 0.03
    return case


def oracle(case):
    return ref.batch_log_likelihood(0.0, *coeffs_of(case), case["t"], case["diag"], case["y"])


def run(case, nchunk, generic, want_chunks=None):
    """``(logdet, quad, status, variant)`` of the forced lazy role-split kernel; ``generic``: the value of CLR_SPLIT_GENERIC."""
    N = case["t"].shape[1]
    plan = batch.BatchedGP(B, N, case["a_real"].shape[1], case["a_comp"].shape[1])
    batch.set_option("CLR_SPLIT_GENERIC", generic)
    try:
        plan.set_chunks(nchunk)
        plan.set_series(case["t"], case["diag"], case["y"])
        plan.set_coefficients(*coeffs_of(case))
        plan.set_summarize_mode(2)
        assert plan.summarize_kernel() == "role split, lazy decay"
        if want_chunks is not None:
            assert plan.chunks == want_chunks
        variant = plan.split_variant()
        ll, ld, q, st = plan.log_likelihood()
        return ld, q, st, variant
    finally:
        batch.set_option("CLR_SPLIT_GENERIC", None)
        plan.close()


def rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


# (chunk lengths are rounded up to a multiple of 8.)  N = 720 in 5 chunks of 144: blocks [0, 64), [64, 128), [128, 144) per
# chunk, none of them padded; N = 717: the last chunk holds 141 samples, its final block ends in three padded steps; 13
# chunks of 56: one block per chunk, shorter than a renormalisation block (and the last chunk ends in 8 padded steps)
BLOCK_CLASSES = [(720, 5, (5, 144)), (717, 5, (5, 144)), (720, 13, (13, 56))]


@pytest.mark.parametrize("JR,JC", SHAPES)
@pytest.mark.parametrize("N,nchunk,chunks", BLOCK_CLASSES)
def test_block_classes_equal_the_general_kernel(N, nchunk, chunks, JR, JC):
    """Every class of renormalisation block -- first (n = 0 inside), interior, padded last, shorter than a block -- gives
    the bits of the general kernel, and both are the oracle's numbers.  ``b_comp`` is
    zero here, so the default path is the ``b_comp == 0`` kernel and the other one is not."""
    case = dict(dense_case(N, JR, JC))
    case["b_comp"] = np.zeros_like(case["b_comp"])
    l0, d0, q0, s0 = oracle(case)
    ld, q, st, v = run(case, nchunk, None, chunks)
    ldg, qg, stg, vg = run(case, nchunk, "1", chunks)
    assert v == dict(b_zero=True) and vg == dict(b_zero=False)
    assert np.array_equal(ld, ldg) and np.array_equal(q, qg) and np.array_equal(st, stg)
    for a, b_, s in ((ld, q, st), (ldg, qg, stg)):
        assert np.array_equal(s, s0) and np.all(s0 == 0)
        assert rel(a, d0) <= REL and rel(b_, q0) <= REL


# a strongly negative diagonal at one sample of problem 1.  N = 717 in 5 chunks of 144: inside an interior block (chunk 2,
# step 70), in the series' first block at n = 1, and in the padded last block (chunk 4, step 130).  N = 1056 in 66 chunks
# of 16 -- two waves of chunks -- at step 0 of chunk 64: lane 0 of the SECOND wave at i = 0, which is not n = 0
FLAG_PLACES = [(717, 5, (5, 144), 2 * 144 + 70), (717, 5, (5, 144), 1), (717, 5, (5, 144), 4 * 144 + 130),
               (1056, 66, (66, 16), 64 * 16)]


@pytest.mark.parametrize("JR,JC", SHAPES)
@pytest.mark.parametrize("N,nchunk,chunks,n_bad", FLAG_PLACES)
def test_pivot_flags_in_every_block_class(N, nchunk, chunks, n_bad, JR, JC):
    """The pivot test no longer computes the lane's sample index: a pivot that is not positive must still be reported
    wherever it sits, and only for the problem that has it -- the status is the oracle's on both paths."""
    case = dict(dense_case(N, JR, JC))
    case["diag"] = case["diag"].copy()
    case["diag"][1, n_bad] = -1e3
    l0, d0, q0, s0 = oracle(case)
    assert s0[1] != 0 and s0[0] == 0 and s0[2] == 0
    for generic in (None, "1"):
        ld, q, st, v = run(case, nchunk, generic, chunks)
        assert np.array_equal(st, s0), (generic, st, s0)
        ok = s0 == 0
        assert rel(ld[ok], d0[ok]) <= REL and rel(q[ok], q0[ok]) <= REL


@pytest.mark.parametrize("JR,JC", SHAPES)
def test_first_pivot_is_left_to_the_oracles_rule(JR, JC):
    """n = 0 is the one sample the pivot test skips (as the reference does): with a strongly negative diagonal THERE the
    status of every problem is still the oracle's, whatever that is, on both paths."""
    case = dict(dense_case(717, JR, JC))
    case["diag"] = case["diag"].copy()
    case["diag"][1, 0] = -1e3
    l0, d0, q0, s0 = oracle(case)
    assert s0[0] == 0 and s0[2] == 0
    for generic in (None, "1"):
        ld, q, st, v = run(case, 5, generic, (5, 144))
        assert np.array_equal(st, s0), (generic, st, s0)
        ok = np.array([True, False, True])
        assert rel(ld[ok], d0[ok]) <= REL and rel(q[ok], q0[ok]) <= REL
        # (the reference does not test its first pivot: the log of a negative one makes its log-determinant NaN)
        assert np.isnan(ld[1]) == np.isnan(d0[1])
        if not np.isnan(d0[1]):
            assert abs(ld[1] - d0[1]) <= REL * abs(d0[1])


@pytest.mark.parametrize("JR,JC", SHAPES)
def test_b_comp_zero_nonzero_and_mixed(JR, JC):
    """The ``b_comp == 0`` kernel is chosen only when EVERY ``b_comp`` of the batch is exactly zero; it gives the general
    kernel's numbers (the sign of an exact zero apart), and every batch is within 1e-10 of the oracle."""
    base = dense_case(720, JR, JC)
    zero = np.zeros_like(base["b_comp"])
    mixed = base["b_comp"].copy()
    mixed[0] = 0.0
    mixed[2, 1:] = 0.0
    for name, b_comp, want in (("zero", zero, True), ("nonzero", base["b_comp"], False), ("mixed", mixed, False)):
        case = dict(base)
        case["b_comp"] = b_comp
        l0, d0, q0, s0 = oracle(case)
        ld, q, st, v = run(case, 5, None, (5, 144))
        assert v["b_zero"] == want, name
        assert np.array_equal(st, s0) and rel(ld, d0) <= REL and rel(q, q0) <= REL, name
        if name == "zero":
            ldg, qg, stg, vg = run(case, 5, "1", (5, 144))
            assert not vg["b_zero"]
            assert np.array_equal(ld, ldg) and np.array_equal(q, qg) and np.array_equal(st, stg)
