"""A kernel is instantiated where a handle of that engine class can launch it (DESIGN.md "Which
kernels a unit holds"): read off the symbol tables of the objects the build leaves in csrc/
(scripts/kernel_inventory.py).  No GPU, no launch."""
import collections
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "climatemachine.jl_amd", "csrc")
PASS_KERNELS = ("k_tendency", "k_gradients", "k_divgrad", "k_gradlap")
TRUE = ("true", "(bool)1")


def _inventory_module():
    spec = importlib.util.spec_from_file_location("kernel_inventory",
                                                  os.path.join(ROOT, "scripts", "kernel_inventory.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def units():
    """{unit: [(kernel template, template arguments, hash of the code bytes)]} of every object"""
    ki = _inventory_module()
    inv = ki.inventory(CSRC)
    assert "engine_esdg" in inv and "engine_atmos_fv" in inv and "engine_atmos" in inv, \
        "the build leaves its objects in csrc/: %s" % sorted(inv)
    names = ki.demangle(sorted({k.symbol for _t, ks in inv.values() for k in ks}))
    out = {}
    for unit, (_text, kernels) in inv.items():
        out[unit] = [(ki.template_of(names[k.symbol]), ki.template_args(names[k.symbol]), k.code)
                     for k in kernels if "<" in names[k.symbol]]
    # (the tables are read: the unit of the dry atmosphere does hold the four pass kernels)
    assert {t for t, _a, _c in out["engine_atmos"]} >= set(PASS_KERNELS)
    return out


def test_esdg_unit_holds_no_dg_pass_kernel(units):
    held = sorted({t for t, _a, _c in units["engine_esdg"] if t in PASS_KERNELS})
    assert held == [], held
    assert any(t == "k_esdg_tendency" for t, _a, _c in units["engine_esdg"])


def test_dgfv_unit_holds_the_one_tendency_variant_and_no_hyperdiffusion(units):
    kernels = units["engine_atmos_fv"]
    assert not [t for t, _a, _c in kernels if t in ("k_divgrad", "k_gradlap")]
    tendency = [a for t, a, _c in kernels if t == "k_tendency"]
    assert tendency, "a DGFVModel handle launches the horizontal tendency kernel"
    # k_tendency<P, NQ, NQV, LSRK, USE_GF, RECV, GARG_OUT, GARG_REFRESH>
    for a in tendency:
        assert a[3] not in TRUE and a[5] not in TRUE, a


@pytest.mark.parametrize("kernel,use_gf", [("k_tendency", 4), ("k_gradients", 3)])
def test_no_unit_holds_identical_copies_that_differ_in_use_gf_alone(units, kernel, use_gf):
    copies = []
    for unit, kernels in units.items():
        seen = collections.defaultdict(set)  # (the other arguments, code) -> USE_GF values
        for t, a, code in kernels:
            if t == kernel:
                seen[(tuple(a[:use_gf] + a[use_gf + 1:]), code)].add(a[use_gf])
        copies += [(unit,) + key[0] for key, gf in seen.items() if len(gf) > 1]
    assert copies == [], copies[:5]
