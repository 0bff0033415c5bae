"""cmdg-mi355x: MI355X-native DG right-hand side + explicit LSRK time stepping for
ClimateMachine-style balance laws.  Import through
``cmdg_loader`` (alias ``climatemachine_jl_amd``).

``mesh`` and ``balancelaws`` are host-only (numpy).  ``dgmodel`` / ``odesolvers``
need torch (device memory) and ``libcmdg.so`` (the hand-written HIP kernels); they
are imported lazily so that the host-side pieces work without a GPU."""
from . import atmos, balancelaws, esdg, mesh, moist, ocean, ocean01  # noqa: F401

__all__ = ["mesh", "balancelaws", "atmos", "esdg", "moist", "ocean", "ocean01", "dgmodel", "odesolvers", "systemsolvers", "plugins",
           "reductions", "fvreconstructions", "diagnostics", "weightedsum", "norm", "dot", "euclidean_distance", "mapreduce", "ConsCallback"]

# MPIStateArrays reductions (reductions.py), exported by name; loaded on first use like dgmodel
_REDUCTIONS = ("weightedsum", "norm", "dot", "euclidean_distance", "mapreduce", "group_weightedsum",
               "group_norm", "group_dot", "group_euclidean_distance", "group_mapreduce", "ConsCallback")


def __getattr__(name):
    import importlib
    if name in ("dgmodel", "odesolvers", "_lib", "plugins", "reductions", "systemsolvers", "fvreconstructions",
                "diagnostics"):
        return importlib.import_module("." + name, __name__)
    if name in _REDUCTIONS:
        return getattr(importlib.import_module(".reductions", __name__), name)
    raise AttributeError(name)
