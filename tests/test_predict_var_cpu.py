# -*- coding: utf-8 -*-
"""The batched predictive variance on the host side: the ABI entries the header declares and the library exports, and
the Python signatures that reach them."""
import inspect

from celerite_amd import batch


def test_predict_var_entry_points_are_declared_and_exported():
    import __graft_entry__ as entry

    names = entry.declared_symbols()
    lib = batch._load()
    for s in ("clr_batch_predict_var", "clr_batch_set_predict_tile", "clr_sharded_predict_var"):
        assert s in names and hasattr(lib, s), s


def test_predict_takes_return_var_defaulting_to_false():
    for cls in (batch.BatchedGP, batch.ShardedBatchedGP):
        par = inspect.signature(cls.predict).parameters
        assert "return_var" in par and par["return_var"].default is False, cls


def test_set_predict_tile_exists():
    par = inspect.signature(batch.BatchedGP.set_predict_tile).parameters
    assert "points" in par and par["points"].default == 0
