"""The table-family records (nvrx_straggler/table_families.py) that robust, peer, pace, pace-per-group and node scores share:
the records against the C bindings -- symbols, arity and argument types, in each family's own argument order --, the by-name
methods of the backend, the workspace and the rings, and how a copied-out block is cut into arrays.  No device is needed."""
import ctypes

import numpy as np
import pytest

FAMILY_NAMES = ("robust", "peer", "pace", "pace_group", "node")
R, N_RANKS, K, S, G = 8, 3, 5, 2, 2
KS = K + S


def _families():
    from nvrx_straggler import table_families

    return table_families.FAMILIES


def _bindings():
    from nvrx_straggler import _native

    return {name: argtypes for name, _, argtypes in _native.SYMBOLS}


def test_the_records_are_the_five_families_in_the_order_they_run_in():
    from nvrx_straggler import table_families

    assert tuple(f.name for f in table_families.FAMILIES) == FAMILY_NAMES
    assert table_families.BY_NAME.keys() == set(FAMILY_NAMES)
    assert [f.slot for f in table_families.FAMILIES] == ["robust", "peer", "pace", "pace", "node"]  # pace_group shares pace's
    assert [f.name for f in table_families.SLOTS] == ["robust", "peer", "pace", "node"]  # settle_readers' order


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_both_c_symbols_exist_and_take_the_arguments_the_record_builds(name):
    """The argument tuple as ``HipBackend._table_step`` builds it -- head, the groups' lead, ``rank_args``, d_out, tail -- has
    the arity the binding declares, an int where it declares ``c_int``, a float where ``c_float``, an address where
    ``c_void_p``."""
    from nvrx_straggler import _native, table_families

    fam, bindings = table_families.BY_NAME[name], _bindings()
    assert fam.c_score in bindings and fam.c_report in bindings
    params = tuple(0.5 if p == "floor_rel" else 3 for p in fam.params)
    lead = () if not fam.groups else (0x3000, G, 4) if fam.max_size else (0x3000, G)
    middle = lead + fam.rank_args(0, N_RANKS, params) + (0x4000,)
    desc = ctypes.pointer(_native.ReportDesc())
    for symbol, args in ((fam.c_score, (0x2000, R, K, S) + middle + (None,)), (fam.c_report, (0x1000, desc) + middle)):
        argtypes = bindings[symbol]
        assert len(args) == len(argtypes), (symbol, len(args), len(argtypes))
        for i, (arg, ctype) in enumerate(zip(args, argtypes)):
            if ctype is ctypes.c_int:
                assert type(arg) is int, (symbol, i, arg)
            elif ctype is ctypes.c_float:
                assert type(arg) is float, (symbol, i, arg)
            elif ctype is ctypes.c_void_p:
                assert arg is None or type(arg) is int, (symbol, i, arg)
            else:
                assert ctype is ctypes.POINTER(_native.ReportDesc) and arg is desc, (symbol, i, arg)
    # the order is the record's, not a guess: the rank range sits where the header puts it
    at = fam.c_args.index("first_rank")
    assert fam.c_args[at + 1] == "n_ranks" and fam.rank_args(11, 12, params)[at : at + 2] == (11, 12)
    assert (at == len(fam.params)) == (name == "node") and (at == 0) == (name != "node")
    assert tuple(v for i, v in enumerate(fam.rank_args(11, 12, params)) if i not in (at, at + 1)) == params


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_the_backend_the_workspace_and_the_rings_have_the_methods_by_name(name):
    from nvrx_straggler import table_families
    from nvrx_straggler.backend import HipBackend, HipRings, TableScores, Workspace

    fam = table_families.BY_NAME[name]
    for cls, method in ((HipBackend, name + "_score"), (HipBackend, name + "_copy_out"), (HipRings, "report_" + name),
                        (Workspace, fam.slot + "_buffers"), (Workspace, fam.slot + "_settle")):
        assert callable(getattr(cls, method)), (cls.__name__, method)
    for cls, method in ((HipBackend, "_table_score"), (HipBackend, "table_copy_out"), (HipRings, "_table_report"),
                        (Workspace, "table_buffers"), (Workspace, "table_settle")):
        assert callable(getattr(cls, method)), (cls.__name__, method)

    class Counting:
        calls = []

    def copy_out(handle):
        Counting.calls.append(handle)
        return ("records",)

    be = Counting()
    setattr(be, name + "_copy_out", copy_out)  # (an instance attribute, as the tests that count copy-outs replace it)
    buf = type("Buf", (), {"data_ptr": lambda self: 0x4000})()
    params = tuple(range(20, 20 + len(fam.params)))
    t = TableScores(be, fam, buf, G if fam.groups else 0, K, S, 1, N_RANKS, params)
    assert (t.first_rank, t.n_ranks, t.K, t.S, t.G, t.d_ptr) == (1, N_RANKS, K, S, G if fam.groups else 0, 0x4000)
    assert tuple(getattr(t, p) for p in fam.params) == params
    with pytest.raises(AttributeError):
        t.no_such_parameter
    assert t.records() == ("records",) and t.records() == ("records",) and Counting.calls == [t]  # by name, once
    assert t.backend is None and t._keep is None


# (shape, dtype, offset in words) of every array, as include/nvrx_straggler.h lays the blocks out
LAYOUTS = {
    "robust": (((KS, 4), np.uint32, 0), ((N_RANKS, 2, 1 + S), np.float32, 4 * KS)),
    "peer": (((G, KS, 4), np.uint32, 0), ((N_RANKS, 1 + S), np.float32, 4 * G * KS)),
    "pace": (((KS, 4), np.uint32, 0), ((N_RANKS, 2, 8), np.uint32, 4 * KS)),
    "pace_group": (((G, KS, 4), np.uint32, 0), ((N_RANKS, 2, 8), np.uint32, 4 * G * KS)),
    "node": (((G, KS, 4), np.uint32, 0), ((KS, 4), np.uint32, 4 * G * KS), ((G, 2, 8), np.uint32, 4 * G * KS + 4 * KS),
             ((N_RANKS, 2, 8), np.uint32, 4 * G * KS + 4 * KS + 16 * G)),
}


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_a_block_is_cut_into_the_arrays_the_header_promises(name):
    from nvrx_straggler import _native, table_families

    fam = table_families.BY_NAME[name]
    words = fam.n_words(G, N_RANKS, K, S)
    assert words == getattr(_native, name + "_words")(*((G,) if fam.groups else ()), N_RANKS, K, S)
    host = np.arange(words, dtype=np.uint32)
    arrays = fam.cut(host, G, N_RANKS, K, S)
    assert len(arrays) == len(LAYOUTS[name])
    end = 0
    for arr, (shape, dtype, offset) in zip(arrays, LAYOUTS[name]):
        assert arr.shape == shape and arr.dtype == dtype, (name, arr.shape, arr.dtype)
        flat = arr.view(np.uint32).reshape(-1)
        assert flat[0] == offset and (flat == np.arange(offset, offset + flat.size)).all(), (name, offset)  # [0, ..., 0] first
        assert arr[(0,) * arr.ndim].view(np.uint32) == offset
        assert not np.shares_memory(arr, host)  # private copies
        end = offset + flat.size
    assert end == words  # the arrays are the whole block
