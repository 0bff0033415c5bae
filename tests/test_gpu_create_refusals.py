"""What ``cmdg_create`` and ``cmdg_create_dgfv`` refuse before they read a grid table, with the status
and the whole ``cmdg_last_error(NULL)`` string: an order outside the compiled set for each of the
twelve laws ``cmdg_create`` serves, an unknown physics id, the ESDG law through ``cmdg_create``, a
Roe flux on a law other than the dry atmosphere, and a DGFVModel of a law other than
AdvectionDiffusion.  The descriptors carry ``physics_id``, ``dim``, ``N``, ``nf_first`` and the
parameter block alone; no grid is allocated.  (The one check ahead of these is that a device is
visible, hence the mark.)

The strings are the literals of the create path as it stood before the laws moved into one table
(csrc/create.hip LAWS): a refusal is part of the C ABI, callers match on it."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
RUSANOV, ROE = 0, 2
NONE_LOADED = "; plug-ins: none loaded"

# physics id, iparam (leading entries), the family's refusal of polynomial order 9
ORDER_REFUSALS = [
    (1, (1,), "AdvectionDiffusion: polynomial order not compiled in (have N = 1..7)"),
    (2, (), "DryAtmos: polynomial order not compiled in (have N = 2..6)"),
    (3, (), "HydrostaticBoussinesq: polynomial order not compiled in (have N = 2..5)"),
    (4, (), "PressureGradientModel: polynomial order not compiled in (have N = 1..7)"),
    (5, (), "ShallowWaterModel: polynomial order not compiled in (have N = 2..5)"),
    (6, (), "MoistAtmos: polynomial orders compiled in: N = 4, 6"),
    (7, (), "SplitExplicit01 laws: polynomial order not compiled in (have N = 4)"),
    (8, (), "SplitExplicit01 laws: polynomial order not compiled in (have N = 4)"),
    (9, (), "SplitExplicit01 laws: polynomial order not compiled in (have N = 4)"),
    (10, (1, 1), "AtmosAcousticGravityLinearModel: polynomial order not compiled in (have N = 4, 5)"),
    (11, (), "AtmosAcousticGravityLinearModel (EquilMoist): polynomial order not compiled in (have N = 4, 6)"),
    (13, (0, 1), "AtmosAcousticLinearModel: polynomial order not compiled in (have N = 4)"),
]


def _desc(cm, physics_id, N, iparam=(), nf_first=RUSANOV, stacked=0):
    d = cm._lib.CmdgDesc()          # (zeroed: every pointer NULL, no elements)
    d.dim = 3
    d.N[0], d.N[1], d.N[2] = N
    d.physics_id = physics_id
    for i, v in enumerate(iparam):
        d.iparam[i] = v
    d.nf_first = nf_first
    d.stacked = stacked
    return d


def _last_error(cm):
    return cm._lib.lib().cmdg_last_error(None).decode()


def _plugin_suffix():
    """``create_handle`` asks the loaded plug-ins before it refuses a law or an order.  None of these
    descriptors is served by a plug-in and none draws a reason from one, so the message ends in
    "none loaded" unless the session has loaded one (tests/test_gpu_plugins.py), and in nothing then."""
    with open("/proc/self/maps") as f:
        return "" if "cmdg_plugin_" in f.read() else NONE_LOADED


def _refused(cm, d, fv=None):
    L = cm._lib.lib()
    h = C.c_void_p(0xdead)
    rc = L.cmdg_create(C.byref(d), C.byref(h)) if fv is None else L.cmdg_create_dgfv(C.byref(d), C.byref(fv), C.byref(h))
    assert h.value is None, "a refused create leaves *out NULL"
    return rc, _last_error(cm)


@pytest.mark.parametrize("physics_id,iparam,message", ORDER_REFUSALS, ids=[str(r[0]) for r in ORDER_REFUSALS])
def test_order_outside_the_compiled_set(cm, torch, physics_id, iparam, message):
    rc, err = _refused(cm, _desc(cm, physics_id, (9, 9, 9), iparam))
    print(physics_id, rc, repr(err))
    assert rc == UNSUPPORTED
    assert err == message + _plugin_suffix()


def test_unknown_physics_id(cm, torch):
    rc, err = _refused(cm, _desc(cm, 99, (4, 4, 4)))
    print(rc, repr(err))
    assert rc == UNSUPPORTED
    assert err == "unknown physics_id" + _plugin_suffix()


def test_esdg_law_through_cmdg_create(cm, torch):
    rc, err = _refused(cm, _desc(cm, 12, (4, 4, 4)))
    print(rc, repr(err))
    assert rc == INVALID
    assert err == ("cmdg_create: the DryAtmosModel of the entropy-stable discretisation has no DGModel passes: "
                   "use cmdg_create_esdg")


def test_roe_flux_on_another_law(cm, torch):
    rc, err = _refused(cm, _desc(cm, 1, (4, 4, 4), (1, 1, 1), nf_first=ROE))
    print(rc, repr(err))
    assert rc == UNSUPPORTED
    assert err == "Roe / HLLC / LMARS numerical fluxes are methods of the dry atmosphere law only"


def test_dgfv_of_another_law(cm, torch):
    fv = cm._lib.CmdgFvDesc(reconstruction=cm._lib.FV_CONSTANT, width=0, limiter=0, nvertelem=2, periodicstack=0)
    rc, err = _refused(cm, _desc(cm, 3, (4, 4, 0), stacked=1), fv)
    print(rc, repr(err))
    assert rc == UNSUPPORTED
    assert err == "cmdg_create_dgfv: the finite-volume passes are compiled for the AdvectionDiffusion law only"
