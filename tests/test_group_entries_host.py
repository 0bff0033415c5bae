"""The entry points that drive several handles at once refuse a NULL handle list, n < 1 and a
NULL member with CMDG_ERR_INVALID before they look at anything else (include/cmdg.h, the
paragraph on multi-handle entries).  Every other argument is valid, so the refusal comes from the
handle checks alone.  It needs no GPU."""
import ctypes as C

import pytest

INVALID = -1
N = 2
_KEEP = []     # host memory behind the pointers below, alive for the module


def _mem():
    """a non-NULL host pointer; a refused call never dereferences it"""
    m = (C.c_double * 8)()
    _KEEP.append(m)
    return C.addressof(m)


def _list(*ptrs):
    """a C array of N pointers (None: NULL), as a void *"""
    arr = (C.c_void_p * N)(*ptrs)
    _KEEP.append(arr)
    return C.cast(arr, C.c_void_p)


def _arr():
    return _list(*[_mem() for _ in range(N)])


def _handle_lists():
    """(list, n, reason): a NULL list, n < 1, NULL members, a NULL member after a non-NULL one"""
    return [(None, N, "NULL list"), (_arr(), 0, "n < 1"), (_list(None, None), N, "NULL members"),
            (_list(_mem(), None), N, "NULL last member")]


@pytest.fixture(scope="module")
def L(cm):
    return cm._lib.lib()


@pytest.fixture(scope="module")
def desc(cm):
    """valid descriptors and a tableau"""
    tab = (C.c_double * 5)(0.0, 0.5, 1.0, 0.5, 0.25)
    red = cm._lib.CmdgReduceDesc()
    red.op, red.nstate = cm._lib.RED_SUM, 1
    oc = cm._lib.CmdgOceanCouplingDesc()
    oc.nvertelem, oc.H = 1, 1.0
    o1 = cm._lib.CmdgOcean01Desc()
    o1.nvertelem, o1.H = 1, 1.0
    _KEEP.extend([tab, red, oc, o1])
    return dict(tab=C.cast(tab, C.c_void_p), red=C.byref(red), oc=C.byref(oc), o1=C.byref(o1))


def test_group_entries_refuse_bad_handle_lists(L, desc):
    a, tab = _arr, desc["tab"]
    for h, n, why in _handle_lists():
        calls = {
            "cmdg_comm_connect_local": lambda: L.cmdg_comm_connect_local(h, n),
            "cmdg_group_rhs": lambda: L.cmdg_group_rhs(h, n, a(), a(), 0.0, 1.0, 0.0),
            "cmdg_group_halo": lambda: L.cmdg_group_halo(h, n, a(), 5),
            "cmdg_group_lsrk_run": lambda: L.cmdg_group_lsrk_run(h, n, a(), a(), 0.0, 1.0, 1, 1,
                                                                 tab, tab, tab),
            "cmdg_group_reduce": lambda: L.cmdg_group_reduce(h, n, desc["red"], a(), None, _mem()),
        }
        for name, call in calls.items():
            assert call() == INVALID, (name, why)


def test_split_explicit_group_steps_refuse_bad_handle_lists(L, desc):
    a, tab = _arr, desc["tab"]
    for h, n, why in _handle_lists():
        for slow, fast, which in ((h, a(), "slow"), (a(), h, "fast")):
            assert L.cmdg_group_split_explicit_step(
                slow, fast, n, desc["oc"], 1, a(), a(), a(), a(), a(), 0.0, 1.0, 1.0, 1,
                tab, tab, tab) == INVALID, ("split_explicit", which, why)
            assert L.cmdg_group_split_explicit01_step(
                slow, fast, n, desc["o1"], a(), a(), a(), a(), a(), 0.0, 1.0, 1.0, 1,
                tab, tab, tab) == INVALID, ("split_explicit01", which, why)


def test_ocean_pair_calls_refuse_null_handles(L, desc):
    """the two-engine calls: a NULL slow or fast handle"""
    for slow, fast in ((None, None), (None, _mem()), (_mem(), None)):
        assert L.cmdg_ocean_initialize_states(slow, fast, desc["oc"]) == INVALID
        assert L.cmdg_ocean_tendency_from_slow_to_fast(slow, fast, desc["oc"], _mem()) == INVALID
        assert L.cmdg_ocean_reconcile_from_fast_to_slow(slow, fast, desc["oc"], _mem(),
                                                        _mem()) == INVALID
