# -*- coding: utf-8 -*-
"""No GPU: the algebra of ``BatchedGP.periodogram`` in NumPy -- the dense reference of tests/_periodogram_ref.py against an
independent route (whiten with the Cholesky factor of ``K``, ordinary least squares), the host's small solve on the
reference's bordered matrices --, the front end's argument checks, and the new symbols.

Largest deviations seen: dense reference against whitened least squares, power 3.5e-16 q/2 and coef 3.7e-15 sqrt(q / G_ii)
(bars 1e-11: two dense routes in double precision at kappa(K) of a few hundred); ``clr_gram_solve`` against
``np.linalg.solve``, coef 6.0e-17 kappa sqrt(q / G_ii), cov 5.7e-16 kappa / sqrt(G_ii G_jj), q - quad against twice the
power 8.3e-17 q (bars 1e-14: a few dozen roundings of a 3 x 3 solve)."""
import inspect
import types

import numpy as np
import pytest

import __graft_entry__
from celerite_amd import batch
from _cases import synthetic, coeffs_of, within
import _periodogram_ref as pref

SYMBOLS = ["clr_batch_periodogram", "clr_batch_set_periodogram_tile", "clr_batch_get_periodogram_ms", "clr_sharded_periodogram",
           "clr_sharded_set_periodogram_tile", "clr_sharded_get_periodogram_ms", "clr_batch_debug_get_periodogram_block"]


def small_case(JR=2, JC=1, family="accuracy", N=200, seed=3):
    case = synthetic(2, N, JR, JC, family, seed=seed)
    return case, [pref.dense_K(coeffs_of(case, p), case["t"][p], case["diag"][p]) for p in range(2)]


@pytest.mark.parametrize("family", ["bench", "accuracy"])
@pytest.mark.parametrize("offset", [False, True])
def test_the_dense_reference_agrees_with_whitened_least_squares(offset, family):
    """``L = cholesky(K)``, ``X~ = L^-1 X``, ``r~ = L^-1 r``: ``lstsq(X~, r~)`` gives the coefficients, and ``power`` is the
    drop in chi^2 / 2 from the model without the sinusoid (nothing, or the offset alone) to the one with it."""
    case, Ks = small_case(family=family)
    for p, K in enumerate(Ks):
        t, r = case["t"][p], case["y"][p]
        omega = pref.scan_frequencies(t)
        fit = pref.dense_periodogram(K, t, r, omega, t_ref=t[0], offset=offset)
        L = np.linalg.cholesky(K)
        rw = np.linalg.solve(L, r)
        q = rw @ rw
        for f, w in enumerate(omega):
            Xw = np.linalg.solve(L, pref.columns(t, w, t[0], offset))
            coef, res, _, _ = np.linalg.lstsq(Xw, rw, rcond=None)
            chi2_with = np.sum((rw - Xw @ coef) ** 2)
            if offset:
                c0 = np.linalg.lstsq(Xw[:, :1], rw, rcond=None)[0]
                chi2_without = np.sum((rw - Xw[:, :1] @ c0) ** 2)
            else:
                chi2_without = q
            within("periodogram reference vs whitened least squares: power, of q / 2",
                   abs(fit.power[f] - 0.5 * (chi2_without - chi2_with)) / (0.5 * q), 1e-11, (p, f))
            scale = np.sqrt(q / np.diag(fit.gram[f])[:-1])
            within("periodogram reference vs whitened least squares: coef, of sqrt(q / G_ii)",
                   np.max(np.abs(fit.coef[f] - coef) / scale), 1e-11, (p, f))
            assert abs(fit.gram[f, -1, -1] - q) <= 1e-12 * q


@pytest.mark.parametrize("offset", [False, True])
def test_the_host_small_solve_reproduces_the_reference(offset):
    case, Ks = small_case(JR=1, JC=2)
    for p, K in enumerate(Ks):
        t, r = case["t"][p], case["y"][p]
        fit = pref.dense_periodogram(K, t, r, pref.scan_frequencies(t), t_ref=t[0], offset=offset)
        w, cov, quad, ld, st = batch.gram_solve(fit.gram)
        assert (st == 0).all()
        q = fit.gram[:, -1, -1]
        g = np.stack([np.diag(S)[:-1] for S in fit.gram])
        within("clr_gram_solve vs np.linalg.solve: coef sqrt(G_ii), of kappa sqrt(q)",
               np.max(np.abs(w - fit.coef) * np.sqrt(g) / (fit.kappa * np.sqrt(q))[:, None]), 1e-14, p)
        within("clr_gram_solve vs np.linalg.solve: cov sqrt(G_ii G_jj), of kappa",
               np.max(np.abs(cov - fit.cov) * np.sqrt(g[:, :, None] * g[:, None, :]) / fit.kappa[:, None, None]), 1e-14, p)
        # the profiled quadratic form is q less twice the power of the fit without an offset
        if not offset:
            within("q - quad vs 2 power, of q", np.max(np.abs((q - quad) - 2.0 * fit.power) / q), 1e-14, p)


@pytest.mark.parametrize("cls", [batch.BatchedGP, batch.ShardedBatchedGP])
def test_argument_errors_come_before_the_library_is_touched(cls):
    """On a stub that is no plan (no handle: anything past the checks fails otherwise)."""
    stub = types.SimpleNamespace(B=3, N=10)
    for bad in (np.zeros((2, 4)), np.zeros((4, 3)), np.zeros((3, 2, 2))):
        with pytest.raises(ValueError, match="dimension mismatch"):
            cls.periodogram(stub, bad)
    for bad in (np.array([1.0, np.nan]), np.array([[1.0, np.inf]] * 3)):
        with pytest.raises(ValueError, match="finite"):
            cls.periodogram(stub, bad)
    with pytest.raises(ValueError, match="t_ref"):
        cls.periodogram(stub, np.ones(2), t_ref=np.nan)
    for bad in (-1e-3, 1.0, np.nan):
        with pytest.raises(ValueError, match="min_pivot"):
            cls.periodogram(stub, np.ones(2), min_pivot=bad)
    sig = inspect.signature(cls.periodogram)
    assert list(sig.parameters) == ["self", "omega", "offset", "t_ref", "min_pivot", "return_gram"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [False, 0.0, 1e-10, False]
    assert list(inspect.signature(cls.set_periodogram_tile).parameters) == ["self", "frequencies"]
    assert hasattr(cls, "periodogram_ms")


def test_the_result_type_and_its_host_side_properties():
    a, phi = 0.5, 0.3
    for row in ([a * np.cos(phi), -a * np.sin(phi)], [7.0, a * np.cos(phi), -a * np.sin(phi)]):
        c = np.array(row)[None, None, :]
        pg = batch.Periodogram(np.zeros((1, 1)), c, None, np.zeros((1, 1), dtype=np.int32), None)
        assert pg._fields == ("power", "coef", "cov", "status", "gram")
        assert abs(pg.amplitude[0, 0] - a) < 1e-15 and abs(pg.phase[0, 0] - phi) < 1e-15


def test_the_new_symbols_are_declared_and_exported():
    declared = __graft_entry__.declared_symbols()
    lib = batch._load()
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
